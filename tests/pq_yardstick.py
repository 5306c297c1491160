"""numpy restatement of the product-quantised index's contract (include/lrx.h), with the loops over i and m written out so
that every sum runs in the contract's order (numpy's pairwise summation would not):

    code[m]      = argmin_j sum_i (x[m dsub + i] - C[m][j][i])^2     fp64 subtract, square, add in order over i; ties to the lower j
    LUT[q][m][j] = (float) sum_i (double) q[m dsub + i] * (double) C[m][j][i]
    s(q, r)      = ((0.f + LUT[q][0][c0]) + LUT[q][1][c1]) + ...     fp32 adds in ascending m
    top-k        score descending, ties to the lower row, (-FLT_MAX, -1) padding

plus a CPU k-means with the index's training rules (sampling, initialisation, fp64 sums, faiss's split of empty clusters)."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
KSUB = 256


def encode(x, C):
    """x fp32 [n, d], C fp32 [M, 256, dsub] -> uint8 [n, M]."""
    n = x.shape[0]
    M, _, dsub = C.shape
    out = np.empty((n, M), np.uint8)
    for m in range(M):
        acc = np.zeros((n, KSUB), np.float64)
        for i in range(dsub):
            t = x[:, m * dsub + i].astype(np.float64)[:, None] - C[m, :, i].astype(np.float64)[None, :]
            acc = acc + t * t
        out[:, m] = np.argmin(acc, axis=1)          # first minimum: the lower j
    return out


def lut(q, C):
    """q fp32 [Q, d] -> fp32 [Q, M, 256]."""
    M, _, dsub = C.shape
    out = np.empty((q.shape[0], M, KSUB), np.float32)
    for m in range(M):
        acc = np.zeros((q.shape[0], KSUB), np.float64)
        for i in range(dsub):
            acc = acc + q[:, m * dsub + i].astype(np.float64)[:, None] * C[m, :, i].astype(np.float64)[None, :]
        out[:, m] = acc.astype(np.float32)
    return out


def scores(L, codes):
    """L fp32 [Q, M, 256], codes uint8 [n, M] -> fp32 [Q, n]."""
    s = np.zeros((L.shape[0], codes.shape[0]), np.float32)
    for m in range(L.shape[1]):
        s = s + L[:, m, codes[:, m]]
    return s


def scores_torch(L, codes):
    """The same sequential fp32 adds with torch tensors (on the GPU for large shards: elementwise IEEE adds, no reassociation)."""
    import torch
    s = torch.zeros(L.shape[0], codes.shape[0], dtype=torch.float32, device=L.device)
    c = codes.long()
    for m in range(L.shape[1]):
        s = s + L[:, m, c[:, m]]
    return s


def topk(S, k):
    """S [Q, n] -> (D fp32 [Q, k], I int64 [Q, k]): descending, ties to the lower row, (-FLT_MAX, -1) padding."""
    Q, n = S.shape
    kk = min(k, n)
    D = np.full((Q, k), -FLT_MAX, np.float32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        o = np.argsort(-S[i], kind="stable")[:kk]
        D[i, :kk], I[i, :kk] = S[i, o], o
    return D, I


def search(q, C, codes, k):
    return topk(scores(lut(q, C), codes), k)


def objective(x, C, codes):
    """sum over rows and sub-spaces of the squared distance to the assigned centroid (fp64)."""
    M, _, dsub = C.shape
    rec = C[np.arange(M)[None, :], codes.astype(np.int64)].reshape(x.shape[0], M * dsub)
    return float(((x.astype(np.float64) - rec.astype(np.float64)) ** 2).sum())


def kmeans(x, M, niter=25, seed=1234, max_points_per_centroid=256):
    """The index's training on the CPU: at most 256 x 256 rows sampled with np.random.default_rng(seed), per sub-space 256 distinct
    sampled rows as the start, Lloyd iterations with fp64 sums in row order, empty clusters split as faiss does."""
    n, d = x.shape
    dsub = d // M
    rng = np.random.default_rng(seed)
    if n > KSUB * max_points_per_centroid:
        x = x[np.sort(rng.permutation(n)[:KSUB * max_points_per_centroid])]
        n = x.shape[0]
    xs = x.reshape(n, M, dsub)
    init = np.stack([rng.permutation(n)[:KSUB] for _ in range(M)])
    C = np.stack([xs[init[m], m] for m in range(M)]).astype(np.float32)
    eps = np.float32(1.0 / 1024.0)
    for _ in range(niter):
        codes = encode(x, C)
        new = np.empty_like(C)
        for m in range(M):
            sums = np.zeros((KSUB, dsub), np.float64)
            np.add.at(sums, codes[:, m].astype(np.int64), xs[:, m].astype(np.float64))
            cnt = np.bincount(codes[:, m], minlength=KSUB)
            new[m] = np.where(cnt[:, None] > 0, sums / np.maximum(cnt, 1)[:, None], C[m]).astype(np.float32)
            for ci in range(KSUB):
                if cnt[ci]:
                    continue
                cj = 0
                while True:
                    if rng.random() < (float(cnt[cj]) - 1.0) / float(max(n - KSUB, 1)):
                        break
                    cj = (cj + 1) % KSUB
                sign = np.where(np.arange(dsub) % 2 == 0, np.float32(1), np.float32(-1))
                new[m, ci] = new[m, cj] * (np.float32(1) + sign * eps)
                new[m, cj] = new[m, cj] * (np.float32(1) - sign * eps)
                cnt[ci] = cnt[cj] // 2
                cnt[cj] -= cnt[ci]
        C = new
    return C


def prototype_corpus(n, d, M, n_proto=64, noise=0.01, seed=0):
    """Rows built from n_proto prototypes per sub-space plus small Gaussian noise."""
    rng = np.random.default_rng(seed)
    dsub = d // M
    protos = rng.standard_normal((M, n_proto, dsub)).astype(np.float32)
    pick = rng.integers(0, n_proto, size=(n, M))
    x = protos[np.arange(M)[None, :], pick].reshape(n, d) + noise * rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32)


def recall_at(I_got, I_want, k):
    return float(np.mean([len(set(I_got[i, :k].tolist()) & set(I_want[i, :k].tolist())) / k for i in range(I_got.shape[0])]))
