"""Numpy yardstick of the inverted-file flat index (lightretriever_amd/ivf.py, lrx_ivf_flat_ip_search): k-means with the
index's rules, the cell of a row, a brute-force search over the probed cells with fp64 scores rounded once, and the 'IwFl' file writer --
written for clarity, not speed.  The GPU tests compare the library with it; the CPU tests check it on its own."""
import struct

import numpy as np

FLT_MAX = np.finfo(np.float32).max
NITER, MAX_POINTS_PER_CENTROID, SEED = 10, 256, 1234
EPS = np.float32(1.0 / 1024.0)


# ---- k-means ------------------------------------------------------------------------------------------------------------------------
def sample_and_init(x: np.ndarray, nlist: int, seed: int = SEED):
    """(rng, the training rows, the initial centroids): at most 256 * nlist rows sampled without replacement (row numbers sorted), then nlist
    distinct rows of the sample -- two draws of one np.random.default_rng(seed), in that order."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    if n < nlist:
        raise ValueError(f"{n} training rows < nlist={nlist}")
    rng = np.random.default_rng(seed)
    max_pts = nlist * MAX_POINTS_PER_CENTROID
    if n > max_pts:
        x = x[np.sort(rng.permutation(n)[:max_pts])]
        n = max_pts
    return rng, x, x[rng.permutation(n)[:nlist]].copy()


def assign_l2(x: np.ndarray, cent: np.ndarray) -> np.ndarray:
    """argmax_j (x . c_j - |c_j|^2 / 2) in fp64, ties to the lower j: the nearest centroid in L2."""
    c = cent.astype(np.float64)
    return np.argmax(x.astype(np.float64) @ c.T - 0.5 * (c * c).sum(axis=1)[None, :], axis=1)


def split_empty(c: np.ndarray, counts: np.ndarray, n: int, rng):
    """faiss Clustering's rule for empty cells (in place, fp32): copy a cell drawn with probability (size - 1) / (n - K), perturb the two copies
    by +-1/1024 per coordinate (even coordinates up for the new one, odd down), split the count."""
    K = c.shape[0]
    sign = np.where(np.arange(c.shape[1]) % 2 == 0, np.float32(1), np.float32(-1))
    for ci in range(K):
        if counts[ci] != 0:
            continue
        cj = 0
        while True:
            if rng.random() < (float(counts[cj]) - 1.0) / float(max(n - K, 1)):
                break
            cj = (cj + 1) % K
        c[ci] = c[cj] * (np.float32(1) + sign * EPS)
        c[cj] = c[cj] * (np.float32(1) - sign * EPS)
        counts[ci] = counts[cj] // 2
        counts[cj] -= counts[ci]


def lloyd(x: np.ndarray, cent: np.ndarray, niter: int, rng) -> np.ndarray:
    """niter Lloyd iterations from `cent`: assignment, fp64 means in row order, empty cells split."""
    x = np.asarray(x, np.float32)
    cent = np.asarray(cent, np.float32).copy()
    K = cent.shape[0]
    for _ in range(niter):
        a = assign_l2(x, cent)
        counts = np.bincount(a, minlength=K).astype(np.int64)
        sums = np.zeros((K, x.shape[1]), np.float64)
        np.add.at(sums, a, x.astype(np.float64))
        new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], cent.astype(np.float64)).astype(np.float32)
        if (counts == 0).any():
            split_empty(new, counts, x.shape[0], rng)
        cent = new
    return cent


def kmeans(x: np.ndarray, nlist: int, niter: int = NITER, seed: int = SEED) -> np.ndarray:
    rng, xs, cent = sample_and_init(x, nlist, seed)
    return lloyd(xs, cent, niter, rng)


def objective(x: np.ndarray, cent: np.ndarray) -> float:
    """The L2 k-means objective in fp64: sum over the rows of the squared distance to the nearest centroid."""
    x, c = np.asarray(x, np.float64), np.asarray(cent, np.float64)
    d2 = (x * x).sum(axis=1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(axis=1)[None, :]
    return float(np.maximum(d2.min(axis=1), 0.0).sum())


# ---- cells and search ------------------------------------------------------------------------------------------------------------------
def exact_scores(q: np.ndarray, X: np.ndarray) -> np.ndarray:
    """fp32 [len(X)]: the fp64 sum of the products of the fp32 elements, rounded once -- the flat index's score."""
    if len(X) == 0:
        return np.zeros(0, np.float32)
    return np.sum(np.asarray(X, np.float32).astype(np.float64) * np.asarray(q, np.float32).astype(np.float64)[None, :], axis=1).astype(np.float32)


def assign_cells(x: np.ndarray, cent: np.ndarray) -> np.ndarray:
    """The cell of every row: its best centroid by exact inner product, ties to the lower cell."""
    return np.array([int(np.argmax(exact_scores(r, cent))) for r in np.asarray(x, np.float32)], dtype=np.int64)


def probe_lists(q: np.ndarray, cent: np.ndarray, nprobe: int) -> np.ndarray:
    """int64 [Q, nprobe]: each query's nprobe best cells by exact inner product, best first, ties to the lower cell."""
    out = np.empty((len(q), nprobe), np.int64)
    for i, r in enumerate(np.asarray(q, np.float32)):
        s = exact_scores(r, cent)
        out[i] = np.lexsort((np.arange(len(s)), -s.astype(np.float64)))[:nprobe]
    return out


def cell_order(cells: np.ndarray, nlist: int):
    """(row_ids, list_off) of rows with the given cells stored cell by cell, ascending original row inside a cell (a stable sort)."""
    row_ids = np.argsort(cells, kind="stable").astype(np.int64)
    list_off = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=nlist))]).astype(np.int64)
    return row_ids, list_off


def search(q, X, list_off, row_ids, probes, k: int, id_base: int = 0, row_map=None, max_scan_rows=None):
    """(D f32[Q,k], I i64[Q,k]): per query the rows of the cells probes[i] names (X fp32 [n, d] stored cell by cell, cell c = positions
    [list_off[c], list_off[c + 1]), row_ids: position -> original row, None = the position; an entry < 0 or >= nlist is skipped, a cell named
    twice counts once), scored exactly, the best k by score descending, ties to the lower ORIGINAL row, (-FLT_MAX, -1) padding.  A query whose
    cells hold more than max_scan_rows (when given) is all padding.  Ids: id_base + row, or row_map[row]."""
    q, X = np.asarray(q, np.float32), np.asarray(X, np.float32)
    list_off, probes = np.asarray(list_off, np.int64), np.asarray(probes, np.int64)
    nlist = len(list_off) - 1
    row_ids = np.arange(len(X), dtype=np.int64) if row_ids is None else np.asarray(row_ids, np.int64)
    Q = q.shape[0]
    D = np.full((Q, k), -FLT_MAX, np.float32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        cells, seen = [], set()
        for c in probes[i].tolist():
            if 0 <= c < nlist and c not in seen:
                seen.add(c)
                cells.append(c)
        pos = np.concatenate([np.arange(list_off[c], list_off[c + 1]) for c in cells] + [np.zeros(0, np.int64)]).astype(np.int64)
        if max_scan_rows is not None and pos.size > max_scan_rows:
            continue
        rows = row_ids[pos]
        sc = exact_scores(q[i], X[pos])
        order = np.lexsort((rows, -sc.astype(np.float64)))[:k]
        D[i, :order.size] = sc[order]
        I[i, :order.size] = (id_base + rows[order]) if row_map is None else np.asarray(row_map, np.int64)[rows[order]]
    return D, I


def overlap(I: np.ndarray, I_ref: np.ndarray) -> np.ndarray:
    """Per query: how many of I_ref's valid ids I holds."""
    return np.array([len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) for a, b in zip(np.asarray(I), np.asarray(I_ref))])


# ---- the file ----------------------------------------------------------------------------------------------------------------------------
def ivf_file_bytes(centroids, list_sizes, rows, row_ids, nprobe: int = 1, is_trained: bool = True) -> bytes:
    """faiss's 'IwFl' record, field by field (index_io.py's head describes it)."""
    cent = np.ascontiguousarray(centroids, "<f4")
    sizes = [int(s) for s in list_sizes]
    nlist, d, ntotal = len(sizes), cent.shape[1], sum(sizes)
    rows, row_ids = np.ascontiguousarray(rows, "<f4").reshape(ntotal, d), np.ascontiguousarray(row_ids, "<i8")

    def header(fourcc, n, trained):
        return struct.pack("<4siqqqBi", fourcc, d, n, 1 << 20, 1 << 20, int(trained), 0)
    out = [header(b"IwFl", ntotal, is_trained), struct.pack("<QQ", nlist, nprobe)]
    out += [header(b"IxFI", cent.shape[0], True), struct.pack("<Q", cent.size), cent.tobytes()]
    out += [struct.pack("<B", 0), struct.pack("<Q", 0)]
    out += [b"ilar", struct.pack("<QQ", nlist, 4 * d)]
    non0 = [c for c in range(nlist) if sizes[c]]
    if len(non0) > nlist // 2:
        out += [b"full", struct.pack("<Q", nlist)] + [struct.pack("<Q", s) for s in sizes]
    else:
        out += [b"sprs", struct.pack("<Q", 2 * len(non0))] + [struct.pack("<QQ", c, sizes[c]) for c in non0]
    a = 0
    for c in non0:
        out += [rows[a:a + sizes[c]].tobytes(), row_ids[a:a + sizes[c]].tobytes()]
        a += sizes[c]
    return b"".join(out)


# ---- the clustered corpus of the nesting and training tests ------------------------------------------------------------------------------
def clustered_corpus(n: int = 20000, d: int = 128, n_clusters: int = 200, seed: int = 7, noise: float = 0.3):
    """(rows fp32 [n, d], queries fp32 [32, d]): Gaussian clusters around n_clusters random centres, queries drawn near corpus rows."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d))
    x = (centres[rng.integers(0, n_clusters, n)] + noise * rng.standard_normal((n, d))).astype(np.float32)
    q = (x[rng.integers(0, n, 32)] + 0.1 * rng.standard_normal((32, d))).astype(np.float32)
    return x, q
