"""numpy restatement of the binary flat index's contract (include/lrx.h):

    bits          bit j = 1 iff x[j] > threshold[j] (strict; NaN -> 0); threshold a scalar or [d]      np.where(x > threshold, 1, 0)
    bytes         np.packbits order: dimension 8 i + b is bit 7 - b of byte i
    h(q, r)       = popcount(bits(q) XOR bits(r))
    Hamming top-k ascending h, ties to the lower row; D int32, I int64; (2^31 - 1, -1) padding
    rerank        candidates = Hamming top-min(binary_k, n); s(q, r) = (float) sum_j (double) q[j] * (bit ? +1 : -1), fp64 accumulation, one rounding;
                  top-k of the candidates by s descending, ties to the lower row; (-FLT_MAX, -1) padding

The fp64 sum is numpy's (pairwise); tests that compare score BITS draw the queries from a grid on which every partial sum is exact, so the
order of the additions cannot matter (see grid_queries)."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
INT_MAX = 2 ** 31 - 1
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def bits(x, threshold=0):
    """x [n, d] -> uint8 0 / 1 [n, d]."""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(x) > threshold, 1, 0).astype(np.uint8)


def pack(x, threshold=0):
    """x [n, d] (d % 8 == 0) -> uint8 [n, d / 8]."""
    return np.packbits(bits(x, threshold), axis=1)


def hamming(qb, xb, block=1 << 16):
    """packed uint8 [Q, d / 8], [n, d / 8] -> int32 [Q, n]."""
    out = np.empty((qb.shape[0], xb.shape[0]), np.int32)
    for s in range(0, xb.shape[0], block):
        x = xb[s:s + block]
        for i in range(qb.shape[0]):
            out[i, s:s + block] = _POP8[np.bitwise_xor(x, qb[i][None, :])].sum(axis=1, dtype=np.int32)
    return out


def hamming_topk(H, k):
    """H int [Q, n] -> (D int32 [Q, k], I int64 [Q, k]): ascending, ties to the lower row, (2^31 - 1, -1) padding."""
    Q, n = H.shape
    kk = min(k, n)
    D = np.full((Q, k), INT_MAX, np.int32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        o = np.argsort(H[i], kind="stable")[:kk]
        D[i, :kk], I[i, :kk] = H[i, o], o
    return D, I


def rerank_scores(q, xb_rows):
    """q fp32 [d], packed candidate rows uint8 [c, d / 8] -> fp32 [c]: (float) of the fp64 sum of +-q."""
    sign = np.unpackbits(xb_rows, axis=1).astype(np.float64) * 2.0 - 1.0
    return (sign * q.astype(np.float64)[None, :]).sum(axis=1).astype(np.float32)


def search(q, xb, k, binary_k=1000, threshold=0, H=None):
    """q fp32 [Q, d], xb packed uint8 [n, d / 8] -> (D fp32 [Q, k], I int64 [Q, k]) of the rerank search."""
    q = np.asarray(q, np.float32)
    H = hamming(pack(q, threshold), xb) if H is None else H
    _, C = hamming_topk(H, min(binary_k, xb.shape[0]))
    Q = q.shape[0]
    D = np.full((Q, k), -FLT_MAX, np.float32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        c = np.sort(C[i])                                   # ascending rows: a stable sort by score then keeps the lower row first
        s = rerank_scores(q[i], xb[c])
        o = np.argsort(-s.astype(np.float64), kind="stable")[:k]
        D[i, :len(o)], I[i, :len(o)] = s[o], c[o]
    return D, I


def grid_queries(rng, Q, d):
    """Multiples of 2^-10 with |q| <= 4: every fp64 partial sum of up to 2^40 such terms is exact, so the rerank score does not depend on the
    order of the additions and its fp32 rounding is the same everywhere."""
    return (rng.integers(-4096, 4097, size=(Q, d)) / 1024.0).astype(np.float32)
