"""Numpy fp64 yardstick of the PCA pre-transform (lightretriever_amd/transform.py): the training of PCAMatrix, the linear map
y = A x + b, and the composition IndexPreTransform(PCAMatrix, flat) -- written for clarity, not speed.  The GPU tests compare the library with
it under bounds derived from the fp32 arithmetic of the library; the CPU tests check it against plain double loops on 50 rows."""
import numpy as np

SEED = 1234                      # PCAMatrix.SEED
MAX_POINTS_PER_D = 1000          # PCAMatrix.max_points_per_d


def subsample(n: int, d_in: int, max_points_per_d: int = MAX_POINTS_PER_D, seed: int = SEED):
    """Row numbers the training uses, ascending: all of them, or max_points_per_d * d_in drawn without replacement."""
    cap = max_points_per_d * d_in
    if n <= cap:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).permutation(n)[:cap])


def covariance(x: np.ndarray):
    """-> (mean [d], C [d, d]) in fp64: C = X^T X / n - mean mean^T (the biased covariance, as faiss computes it)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    return mean, x.T @ x / n - np.outer(mean, mean)


def fix_signs(vecs: np.ndarray) -> np.ndarray:
    """Rows = eigenvectors: each one's largest-magnitude component (the lowest index on ties) is made positive."""
    vecs = np.array(vecs, copy=True)
    j = np.argmax(np.abs(vecs), axis=1)
    neg = vecs[np.arange(vecs.shape[0]), j] < 0
    vecs[neg] *= -1
    return vecs


def train(x: np.ndarray, d_out: int, eigen_power: float = 0.0, max_points_per_d: int = MAX_POINTS_PER_D, seed: int = SEED) -> dict:
    """-> dict(rows, mean, C, eigenvalues [d_in], PCAMat [d_in, d_in] (rows = eigenvectors), A [d_out, d_in], b [d_out]), everything fp64."""
    x = np.asarray(x)
    n, d_in = x.shape
    rows = subsample(n, d_in, max_points_per_d, seed)
    mean, C = covariance(x[rows])
    lam, V = np.linalg.eigh(C)
    order = np.argsort(-lam, kind="stable")
    lam, pcamat = lam[order], fix_signs(V[:, order].T)
    A = pcamat[:d_out].copy()
    if eigen_power != 0:
        A *= (lam[:d_out] ** eigen_power)[:, None]
    return dict(rows=rows, mean=mean, C=C, eigenvalues=lam, PCAMat=pcamat, A=A, b=-A @ mean)


def apply(x: np.ndarray, A: np.ndarray, b=None) -> np.ndarray:
    """y = x A^T + b in fp64."""
    y = np.asarray(x, dtype=np.float64) @ np.asarray(A, dtype=np.float64).T
    return y if b is None else y + np.asarray(b, dtype=np.float64)


def reverse(y: np.ndarray, A: np.ndarray, b) -> np.ndarray:
    """(y - b) A in fp64: the inverse of apply on the row space of an orthonormal A."""
    return (np.asarray(y, dtype=np.float64) - np.asarray(b, dtype=np.float64)) @ np.asarray(A, dtype=np.float64)


def apply_bound(x: np.ndarray, A: np.ndarray, b=None) -> np.ndarray:
    """Elementwise bound of |fp32 chain - fp64| for y = A x + b computed as ONE fp32 accumulator per output that starts at b and takes K = d_in
    products: each step rounds at most twice (the product, the sum; a fused multiply-add rounds once), each rounding is relative 2^-24 of a
    partial result that is at most |b| + sum |a||x| in magnitude, so the error is at most 2 K 2^-24 (1 + o(1)) of that sum in ANY order of the
    steps; (K + 1) 2^-23 leaves the o(1) its room."""
    x, A = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(A, dtype=np.float64))
    s = x @ A.T
    if b is not None:
        s = s + np.abs(np.asarray(b, dtype=np.float64))
    return (A.shape[1] + 1) * 2.0 ** -23 * s


def topk(scores: np.ndarray, k: int, id_base: int = 0):
    """The flat index's rule over a [Q, n] score matrix: score descending, ties to the lower row, (-FLT_MAX, -1) padding."""
    Q, n = scores.shape
    D = np.full((Q, k), -np.finfo(np.float32).max, dtype=np.float32)
    I = np.full((Q, k), -1, dtype=np.int64)
    for qi in range(Q):
        order = np.lexsort((np.arange(n), -scores[qi].astype(np.float64)))[:k]
        D[qi, :order.size] = scores[qi, order]
        I[qi, :order.size] = order + id_base
    return D, I


def pre_transform_search(q: np.ndarray, x: np.ndarray, A: np.ndarray, b, k: int):
    """IndexPreTransform(PCAMatrix, IndexFlatIP) in fp64: the top-k of <A q + b, A x_r + b>."""
    return topk(apply(q, A, b) @ apply(x, A, b).T, k)


def planted(n: int, d: int = 256, top: int = 64, seed: int = 0) -> np.ndarray:
    """The planted-spectrum corpus of the tests: `top` directions of scale 4 .. 2, the others 0.5 .. 0.05, in a rotated basis, plus a mean of
    0.3 N(0, 1); fp32 [n, d]."""
    rng = np.random.default_rng(seed)
    scale = np.concatenate([np.linspace(4.0, 2.0, top), np.linspace(0.5, 0.05, d - top)])
    basis, _ = np.linalg.qr(rng.standard_normal((d, d)))
    mean = 0.3 * rng.standard_normal(d)
    return ((rng.standard_normal((n, d)) * scale) @ basis.T + mean).astype(np.float32)
