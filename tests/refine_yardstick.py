"""Numpy yardstick of the exact re-ranking (lightretriever_amd/refine.py, lrx_flat_ip_rerank / lrx_sq_fp16_ip_rerank): the exact
score, the top k of a caller's candidate rows with the skip / duplicate / tie / padding rules, and faiss's k_base -- written for clarity, not
speed.  The GPU tests compare the library with it bit for bit; the CPU tests check it against plain double loops on 50 rows."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
MAX_K_BASE = 2048                # the most candidates per query the rerank takes


def exact_score(q: np.ndarray, x: np.ndarray) -> np.float32:
    """The score every search path reports for (query q, row x): the fp64 sum of the products of the fp32 elements, rounded once to fp32."""
    return np.float32(np.sum(q.astype(np.float64) * x.astype(np.float64)))


def exact_scores(q: np.ndarray, X: np.ndarray, rows) -> np.ndarray:
    """exact_score(q, X[r]) for every r of `rows`, fp32 [len(rows)]."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0:
        return np.zeros(0, np.float32)
    return np.sum(X[rows].astype(np.float64) * q.astype(np.float64)[None, :], axis=1).astype(np.float32)


def k_base(k: int, k_factor: float) -> int:
    """faiss IndexRefine::search: k_base = idx_t(k * k_factor)."""
    return int(k * k_factor)


def rerank(q: np.ndarray, X: np.ndarray, cand: np.ndarray, k: int, id_base: int = 0, row_map=None, n_rows=None):
    """(D f32[Q,k], I i64[Q,k]): per query the candidates cand[i] (row numbers; an entry < 0 or >= n_rows -- default: len(X) -- is skipped, a
    row named twice counts twice) scored exactly over the rows X (fp32 [n, d]; for an fp16 store: the decoded codes), the best k by score
    descending, ties to the lower row, (-FLT_MAX, -1) padding.  Ids: id_base + row, or row_map[row]."""
    q, X, cand = np.asarray(q, np.float32), np.asarray(X, np.float32), np.asarray(cand, np.int64)
    n_rows = X.shape[0] if n_rows is None else n_rows
    Q = q.shape[0]
    D = np.full((Q, k), -FLT_MAX, np.float32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        rows = cand[i][(cand[i] >= 0) & (cand[i] < n_rows)]
        sc = exact_scores(q[i], X, rows)
        order = np.lexsort((rows, -sc.astype(np.float64)))[:k]            # primary: score descending; then the lower row
        D[i, :order.size] = sc[order]
        I[i, :order.size] = (id_base + rows[order]) if row_map is None else np.asarray(row_map, np.int64)[rows[order]]
    return D, I


def recall(I: np.ndarray, I_ref: np.ndarray) -> float:
    """Mean share of I_ref's valid ids per query that I holds."""
    hit = [len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(int((b >= 0).sum()), 1) for a, b in zip(np.asarray(I), np.asarray(I_ref))]
    return float(np.mean(hit))
