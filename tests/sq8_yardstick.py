"""numpy restatement of the 8-bit scalar-quantised index's contract (include/lrx.h, lrx_sq8_ip_search): faiss
IndexScalarQuantizer(d, QT_8bit | QT_8bit_uniform, METRIC_INNER_PRODUCT) with the range statistic RS_minmax (argument 0).  train / encode /
decode are fp32 with one numpy operation per rounding (numpy never contracts), scores are fp64 sums rounded once, top-k is the PQ
yardstick's (score descending, ties to the lower row, (-FLT_MAX, -1) padding)."""
import numpy as np

from pq_yardstick import topk  # noqa: F401  (re-exported: the selection rule is the same)

F32 = np.float32
QT_8BIT, QT_8BIT_UNIFORM = 0, 2


def train(x: np.ndarray, uniform: bool = False) -> np.ndarray:
    """-> trained = vmin ++ vdiff (2 d floats; 2 for the uniform quantiser).  NaN is ignored (fmin / fmax), -0 counts as +0; a range with
    no value that is not NaN gets vmin = vdiff = 0."""
    x = np.asarray(x, dtype=F32)
    if x.shape[0] < 1:
        raise ValueError("train: 0 rows")
    axis = None if uniform else 0
    with np.errstate(all="ignore"):
        vmin = np.atleast_1d(np.fmin.reduce(x, axis=axis) + F32(0)).astype(F32)
        vmax = np.atleast_1d(np.fmax.reduce(x, axis=axis) + F32(0)).astype(F32)
    empty = np.isnan(vmin)
    vmin, vmax = np.where(empty, F32(0), vmin).astype(F32), np.where(empty, F32(0), vmax).astype(F32)
    return np.concatenate([vmin, (vmax - vmin).astype(F32)])


def _split(trained: np.ndarray, d: int):
    t = np.asarray(trained, dtype=F32)
    if t.size == 2:
        return np.full(d, t[0], F32), np.full(d, t[1], F32)
    assert t.size == 2 * d
    return t[:d], t[d:]


def encode(x: np.ndarray, trained: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=F32)
    vmin, vdiff = _split(trained, x.shape[1])
    with np.errstate(all="ignore"):
        t = ((x - vmin).astype(F32) / np.where(vdiff != 0, vdiff, F32(1))).astype(F32)
        t = np.where(vdiff != 0, t, F32(0)).astype(F32)
        t = np.where(t >= 0, t, F32(0)).astype(F32)                # below the range, and NaN
        t = np.where(t > 1, F32(1), t).astype(F32)
        return (F32(255) * t).astype(F32).astype(np.int32).astype(np.uint8)     # truncation


def decode(codes: np.ndarray, trained: np.ndarray) -> np.ndarray:
    codes = np.asarray(codes)
    vmin, vdiff = _split(trained, codes.shape[1])
    t = ((codes.astype(F32) + F32(0.5)).astype(F32) / F32(255)).astype(F32)
    return (vmin + (t * vdiff).astype(F32)).astype(F32)


def scores(q: np.ndarray, codes: np.ndarray, trained: np.ndarray) -> np.ndarray:
    """s(q, r) = (float) sum_i (double) q_i (double) y_r,i over the decoded rows."""
    return (np.asarray(q, dtype=np.float64) @ decode(codes, trained).astype(np.float64).T).astype(F32)


def search(q: np.ndarray, codes: np.ndarray, trained: np.ndarray, k: int):
    return topk(scores(q, codes, trained), k)
