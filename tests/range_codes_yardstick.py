"""numpy restatement of the range search over the quantised and sparse indexes (include/lrx.h: lrx_sq_fp16_ip_range_search,
lrx_pq_ip_range_search, lrx_range_impact_search): per index the score its top-k search reports, then ONE keep rule --

    fp16-SQ   s(q, r) = np.float32(np.dot(q as fp64, code row r as fp64))
    PQ        s(q, r) = pq_yardstick.scores: ((0.f + LUT[0][c0]) + LUT[1][c1]) + ... in fp32
    impact    s(q, r) = np.float32(S), S the exact integer score of impact_yardstick; only hits (S >= 1) can be kept

    a row is in the result iff s > radius (and it is a hit, for the impact index); rows ascend inside a query;
    (lims int64 [Q + 1], D fp32 [lims[Q]], I int64 [lims[Q]]), I = id_base + row."""
import numpy as np

import impact_yardstick
import pq_yardstick


def sq_fp16_scores(q, codes):
    """q fp32 [Q, d], codes fp16 [n, d] -> fp32 [Q, n]: fp64 products and sums, one rounding."""
    return np.dot(np.asarray(q, np.float32).astype(np.float64), np.asarray(codes, np.float16).astype(np.float64).T).astype(np.float32)


def pq_scores(q, C, codes):
    """q fp32 [Q, d], C fp32 [M, 256, dsub], codes uint8 [n, M] -> fp32 [Q, n]."""
    return pq_yardstick.scores(pq_yardstick.lut(q, C), codes)


def impact_scores(yard: impact_yardstick.Yardstick, queries):
    """queries [(term ids, counts), ...] -> int64 [Q, n], the exact integer scores."""
    return np.stack([yard.scores(t, c) for t, c in queries]) if len(queries) else np.zeros((0, yard.n), np.int64)


def keep(S, radius, hits=None):
    """S fp32 [Q, n] -> (lims, D, I) of the rows with S > radius (and hits[q, r], when given), ascending rows per query."""
    S = np.asarray(S, np.float32)
    mask = S > np.float32(radius) if np.isfinite(radius) else (S > radius)
    if hits is not None:
        mask = mask & hits
    lims = np.zeros(S.shape[0] + 1, np.int64)
    lims[1:] = np.cumsum(mask.sum(axis=1))
    qi, rows = np.nonzero(mask)                      # row-major: queries ascending, rows ascending inside a query
    return lims, S[qi, rows], rows.astype(np.int64)


def range_dense(S, radius, id_base=0):
    lims, D, I = keep(S, radius)
    return lims, D, I + id_base


def range_impact(S_int, radius, id_base=0):
    """S_int int64 [Q, n] -> the hits (S >= 1) whose np.float32(S) is > radius."""
    S_int = np.asarray(S_int, np.int64)
    lims, D, I = keep(S_int.astype(np.float32), radius, hits=S_int >= 1)
    return lims, D, I + id_base


def brute_force(S, radius, hits=None, id_base=0):
    """The same rule as a double loop (the yardstick's own check)."""
    lims, D, I = [0], [], []
    for qi in range(len(S)):
        for r in range(len(S[qi])):
            if S[qi][r] > radius and (hits is None or hits[qi][r]):
                D.append(S[qi][r])
                I.append(id_base + r)
        lims.append(len(I))
    return np.asarray(lims, np.int64), np.asarray(D, np.float32), np.asarray(I, np.int64)
