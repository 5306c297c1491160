"""PCA pre-transform: the faiss.PCAMatrix and faiss.IndexPreTransform surfaces the reference uses (retriever/faiss_search.py:512-565), over
lrx_linear_transform -- the exact fp32 linear map y = A x + b on the f32-input MFMA (csrc/lrx_transform.hip).

    pca = PCAMatrix(2048, 256); pca.train(x)                       # deterministic: the same rows give the same bits
    idx = PreTransformIndex(pca, FlatIPIndex(256)); idx.add(x)     # the kernel writes the reduced rows straight into the base's slot
    D, I = idx.search(q, 100)                                      # = base.search(pca.apply(q), 100)

Every row added and every query goes through one kernel whose result for a row depends on that row alone, so PreTransformIndex(T, B) returns
exactly what B returns when it is fed T.apply(x) and searched with T.apply(q): the base's score contract holds over the reduced rows."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .index import FlatIPIndex, PQIndex, SQ8Index, SQFp16Index, _as_rows, _check_range


def _ld(t: torch.Tensor) -> int:
    """Row stride of a 2-D tensor whose columns are contiguous (a single row may report any stride)."""
    return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]


def linear_transform(x: torch.Tensor, A: torch.Tensor, b: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = A x[r] + b (lrx_linear_transform): x fp32 [n, d_in] on the device with contiguous columns (rows may be strided), A fp32
    [d_out, d_in] contiguous, b fp32 [d_out] or None; out: fp32 [n, d_out] with contiguous columns (rows may be strided), allocated when
    None.  d_in % 8 == 0, 8 <= d_in <= 8192."""
    if x.dtype != torch.float32 or A.dtype != torch.float32 or x.ndim != 2 or A.ndim != 2 or x.shape[1] != A.shape[1] or not x.is_cuda:
        raise ValueError(f"linear_transform: x fp32 [n, d_in] and A fp32 [d_out, d_in] on the device, got {tuple(x.shape)} {x.dtype} / {tuple(A.shape)} {A.dtype}")
    if not A.is_contiguous() or (b is not None and (b.dtype != torch.float32 or b.numel() != A.shape[0] or not b.is_contiguous())):
        raise ValueError("linear_transform: A [d_out, d_in] and b [d_out] must be contiguous fp32")
    if x.shape[0] > 0 and x.stride(1) != 1:
        x = x.contiguous()
    n, d_out = x.shape[0], A.shape[0]
    if out is None:
        out = torch.empty(n, d_out, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.ndim != 2 or out.shape != (n, d_out) or out.device != x.device or (n > 0 and out.stride(1) != 1):
        raise ValueError(f"linear_transform: out must be fp32 [{n}, {d_out}] on {x.device} with contiguous columns")
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().lrx_linear_transform(_lib.ptr(x), n, _ld(x), _lib.ptr(A), _lib.ptr(b), x.shape[1], d_out, _lib.ptr(out), _ld(out),
                                                   _lib.current_stream()))
    return out


class PCAMatrix:
    """faiss.PCAMatrix(d_in, d_out, eigen_power, random_rotation): attributes is_trained, mean [d_in], eigenvalues [d_in] (descending), PCAMat
    [d_in, d_in] (rows = eigenvectors), A [d_out, d_in], b [d_out] -- fp32 device tensors once trained -- and train / apply / apply_into /
    reverse_transform / copy_from.

    train(x): at most max_points_per_d (1000) x d_in rows (sampled without replacement with np.random.default_rng(SEED), row numbers sorted,
    as PQIndex.train samples); the column mean in fp64; the Gram matrix X^T X from lrx_linear_transform over row chunks of <= 4096 (x = A =
    the transposed chunk, so K = the chunk's rows), the chunk results added in fp64 in chunk order; C = G / n - mean mean^T in fp64;
    torch.linalg.eigh in fp64 on the host; eigenvalues descending; each eigenvector's sign fixed so that its largest-magnitude component
    (lowest index on ties) is positive.  PCAMat = the eigenvectors rounded to fp32; A = PCAMat[:d_out], each row scaled in fp64 by
    eigenvalue^eigen_power (the fp32 eigenvalue) when eigen_power != 0 and rounded once; b = -A mean in fp64 (the fp32 A, the fp64 mean),
    rounded once.  No RNG beyond the sample, no vendor BLAS, no atomics: the same rows give the same bits.  The matrix is not faiss's bit
    for bit (its LAPACK and summation order differ); the subspace is the same.
    random_rotation=True is refused (faiss's RNG cannot be matched).  d_in % 8 == 0, 8 <= d_in <= 8192 (the kernel's K)."""
    SEED = 1234
    GRAM_CHUNK = 4096

    def __init__(self, d_in: int, d_out: int, eigen_power: float = 0.0, random_rotation: bool = False, device: Optional[torch.device] = None):
        if random_rotation:
            raise NotImplementedError("PCAMatrix: random_rotation is not served (faiss's random rotation cannot be reproduced)")
        if d_out > d_in or d_out < 1:
            raise ValueError(f"PCAMatrix: d_out={d_out} must be in 1 .. d_in={d_in}")
        if d_in % 8 != 0 or not 8 <= d_in <= 8192:
            raise ValueError(f"PCAMatrix: d_in={d_in} must be a multiple of 8 (8 .. 8192)")
        self.d_in, self.d_out = int(d_in), int(d_out)
        self.eigen_power, self.random_rotation = float(eigen_power), False
        self.max_points_per_d = 1000
        self.device = device
        self.is_trained = False
        self.mean = self.eigenvalues = self.PCAMat = self.A = self.b = None
        self._At = None                     # A^T padded to a multiple of 8 columns: the matrix of reverse_transform

    def _device(self) -> torch.device:
        if self.device is None:
            _lib.require_gpu()
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def _rows(self, x, where: str, d: Optional[int] = None) -> torch.Tensor:
        x = _as_rows(x, self.d_in if d is None else d, where).to(device=self._device(), dtype=torch.float32)
        return x if x.shape[0] == 0 or x.stride(1) == 1 else x.contiguous()

    # -- training ------------------------------------------------------------------------------------------------
    def sample_rows(self, n: int) -> Optional[np.ndarray]:
        """The sorted row numbers train() keeps of n rows, or None when it keeps them all."""
        cap = self.max_points_per_d * self.d_in
        if n <= cap:
            return None
        return np.sort(np.random.default_rng(self.SEED).permutation(n)[:cap])

    def gram(self, x: torch.Tensor):
        """(column sums fp64 [d_in], X^T X fp64 [d_in, d_in]) of fp32 device rows x: per chunk of <= GRAM_CHUNK rows one lrx_linear_transform
        call whose K is the chunk's rows (zero rows pad it to a multiple of 8: they add exact zeros), added in fp64 in chunk order."""
        d = self.d_in
        s = torch.zeros(d, dtype=torch.float64, device=x.device)
        G = torch.zeros(d, d, dtype=torch.float64, device=x.device)
        for r0 in range(0, x.shape[0], self.GRAM_CHUNK):
            xc = x[r0:r0 + self.GRAM_CHUNK]
            m = xc.shape[0]
            xt = torch.zeros(d, -(-m // 8) * 8, dtype=torch.float32, device=x.device)
            xt[:, :m] = xc.t()
            s += xc.sum(dim=0, dtype=torch.float64)
            G += linear_transform(xt, xt).double()
        return s, G

    def train(self, x):
        if x.ndim != 2 or x.shape[1] != self.d_in:
            raise ValueError(f"PCAMatrix.train: expected [n,{self.d_in}], got {tuple(x.shape)}")
        n = x.shape[0]
        if n < self.d_out:
            raise ValueError(f"PCAMatrix.train: {n} training rows < d_out={self.d_out}")
        rows = self.sample_rows(n)
        if rows is not None:
            x = x[torch.from_numpy(rows).to(x.device)] if isinstance(x, torch.Tensor) else x[rows]
            n = rows.size
        x = self._rows(x, "PCAMatrix.train: ")
        s, G = self.gram(x)
        mean = (s / n).cpu()
        C = G.cpu() / n - torch.outer(mean, mean)
        lam, V = torch.linalg.eigh(C)                                    # ascending, eigenvectors in columns
        lam, vecs = lam.flip(0), V.flip(1).t().contiguous()              # descending, eigenvectors in rows
        j = vecs.abs().argmax(dim=1)                                     # (the first of equal maxima)
        vecs = vecs * torch.where(vecs[torch.arange(self.d_in), j] < 0, -1.0, 1.0).to(vecs.dtype)[:, None]
        dev = self._device()
        self.mean = mean.float().to(dev)
        self.eigenvalues = lam.float().to(dev)
        self.PCAMat = vecs.float().to(dev)
        A = self.PCAMat[:self.d_out].double()
        if self.eigen_power != 0:
            A = A * (self.eigenvalues[:self.d_out].double() ** self.eigen_power)[:, None]
        self.A = A.float().contiguous()
        self.b = (-(self.A.double().cpu() * mean[None, :]).sum(dim=1)).float().to(dev)   # (a plain fp64 sum per row: no BLAS)
        self._At = None
        self.is_trained = True

    def copy_from(self, other: "PCAMatrix") -> "PCAMatrix":
        """Take over `other`'s trained state (its tensors are shared: they are never written in place).  Returns self."""
        if (other.d_in, other.d_out) != (self.d_in, self.d_out):
            raise ValueError(f"PCAMatrix.copy_from: {other.d_in} -> {other.d_out} does not match {self.d_in} -> {self.d_out}")
        self.eigen_power, self.max_points_per_d, self.is_trained = other.eigen_power, other.max_points_per_d, other.is_trained
        self.device = other.device if other.device is not None else self.device
        self.mean, self.eigenvalues, self.PCAMat, self.A, self.b, self._At = other.mean, other.eigenvalues, other.PCAMat, other.A, other.b, other._At
        return self

    # -- the map -------------------------------------------------------------------------------------------------
    def _need_trained(self, who: str):
        if not self.is_trained:
            raise RuntimeError(f"PCAMatrix.{who}: the transform is not trained (call train() first)")

    def apply(self, x) -> torch.Tensor:
        """faiss apply: x [n, d_in] (torch on any device, or numpy) -> fp32 device tensor [n, d_out] = x A^T + b."""
        self._need_trained("apply")
        return linear_transform(self._rows(x, "PCAMatrix.apply: "), self.A, self.b)

    def apply_into(self, x, out: torch.Tensor) -> torch.Tensor:
        """apply() written into `out` (fp32 device [n, d_out], rows may be strided): an index slot."""
        self._need_trained("apply_into")
        return linear_transform(self._rows(x, "PCAMatrix.apply_into: "), self.A, self.b, out=out)

    def reverse_transform(self, y) -> torch.Tensor:
        """faiss reverse_transform: y [n, d_out] -> fp32 device tensor [n, d_in] = (y - b) A, through the same kernel with A^T.  Exact inverse
        on A's row space while A is orthonormal, so it is refused when eigen_power != 0."""
        self._need_trained("reverse_transform")
        if self.eigen_power != 0:
            raise ValueError("PCAMatrix.reverse_transform: A is not orthonormal when eigen_power != 0")
        k8 = -(-self.d_out // 8) * 8                                     # (the kernel's K is a multiple of 8: zero columns add exact zeros)
        if self._At is None:
            self._At = torch.zeros(self.d_in, k8, dtype=torch.float32, device=self.A.device)
            self._At[:, :self.d_out] = self.A.t()
        y = self._rows(y, "PCAMatrix.reverse_transform: ", self.d_out)
        z = torch.zeros(y.shape[0], k8, dtype=torch.float32, device=y.device)
        z[:, :self.d_out] = y - self.b
        return linear_transform(z, self._At)

    # -- persistence (index_io.pre_transform_prefix) ----------------------------------------------------------------
    def state(self) -> dict:
        vec = {k: (getattr(self, k).cpu().numpy() if self.is_trained else np.zeros(0, np.float32)) for k in ("mean", "eigenvalues", "PCAMat", "A", "b")}
        return dict(d_in=self.d_in, d_out=self.d_out, eigen_power=self.eigen_power, random_rotation=False, is_trained=self.is_trained, **vec)

    @classmethod
    def from_state(cls, st: dict, device: Optional[torch.device] = None) -> "PCAMatrix":
        pca = cls(st["d_in"], st["d_out"], st["eigen_power"], st["random_rotation"], device=device)
        if st["is_trained"]:
            dev = pca._device()
            for k in ("mean", "eigenvalues", "PCAMat", "A", "b"):
                setattr(pca, k, torch.from_numpy(np.array(st[k], dtype=np.float32)).to(dev).contiguous())
            pca.is_trained = True
        return pca


BASES = (FlatIPIndex, SQFp16Index, SQ8Index, PQIndex)


class PreTransformIndex:
    """faiss.IndexPreTransform(transform, base_index) for one PCAMatrix: d = d_in; ntotal, device and id_base are the base's; is_trained
    reflects both parts.  Bases: FlatIPIndex, SQFp16Index, SQ8Index, PQIndex (anything else: TypeError).  Scores, ties and padding are the
    base's contract over the reduced rows transform.apply(x), searched with transform.apply(q) -- bit for bit what the base returns when it is
    handed those rows itself.
    add(x): the kernel writes the reduced rows straight into base.append_slot(n), then base.commit(n).  append_slot(n) / commit(n): the slot is
    this index's own transient fp32 staging of width d_in (what an encoder writes into); commit() trains whatever is untrained on the staged
    rows, transforms them into the base's slot, commits the base and releases the staging.  NOT thread-safe (the base's rule)."""

    def __init__(self, transform: PCAMatrix, base_index):
        if not isinstance(transform, PCAMatrix):
            raise TypeError(f"PreTransformIndex: transform must be a PCAMatrix, got {type(transform).__name__}")
        if not isinstance(base_index, BASES):
            raise TypeError(f"PreTransformIndex: base index {type(base_index).__name__} is not served (only {', '.join(c.__name__ for c in BASES)})")
        if base_index.d != transform.d_out:
            raise ValueError(f"PreTransformIndex: the base's d={base_index.d} is not the transform's d_out={transform.d_out}")
        self.transform, self.index = transform, base_index
        self.d = transform.d_in
        if transform.device is None:
            transform.device = base_index.device
        self._stage = None

    ntotal = property(lambda self: self.index.ntotal)
    device = property(lambda self: self.index.device)
    is_trained = property(lambda self: bool(self.transform.is_trained and getattr(self.index, "is_trained", True)))

    @property
    def id_base(self):
        return self.index.id_base

    @id_base.setter
    def id_base(self, v):
        self.index.id_base = v

    def _rows(self, x, where: str) -> torch.Tensor:
        return self.transform._rows(x, where)

    def train(self, x):
        """Trains the transform if it is untrained, then the base -- on apply(x) -- if it is untrained."""
        if not self.transform.is_trained:
            self.transform.train(x)
        if not getattr(self.index, "is_trained", True):
            self.index.train(self.transform.apply(x))

    def _add_rows(self, x: torch.Tensor):
        n = x.shape[0]
        if n:
            self.transform.apply_into(x, self.index.append_slot(n))
            self.index.commit(n)

    def add(self, x):
        """faiss add(x f32[n, d_in]); raises before train(), as faiss does."""
        if not self.is_trained:
            raise RuntimeError("PreTransformIndex.add: the index is not trained (call train() first)")
        self._add_rows(self._rows(x, "add: "))

    def append_slot(self, n_rows: int) -> torch.Tensor:
        """A transient fp32 staging view [n, d_in] for the next n rows: write them, then commit(n)."""
        if self._stage is None or self._stage.shape[0] < n_rows:
            self._stage = None
            self._stage = torch.empty(n_rows, self.d, dtype=torch.float32, device=self.device)
        return self._stage[:n_rows]

    def commit(self, n_rows: int):
        if n_rows > 0:
            if self._stage is None or n_rows > self._stage.shape[0]:
                raise ValueError(f"commit({n_rows}): only {0 if self._stage is None else self._stage.shape[0]} staged rows")
            rows = self._stage[:n_rows]
            if not self.is_trained:
                self.train(rows)
            self._add_rows(rows)
        self._stage = None                             # staging released (stream-ordered by the allocator)

    def search(self, q, k: int, **kwargs):
        """base.search(transform.apply(q), k, **kwargs)."""
        return self.index.search(self.transform.apply(self._rows(q, "search: ")), k, **kwargs)

    def range_search(self, q, radius: float):
        """base.range_search(transform.apply(q), radius); a base without range search raises its own error."""
        return self.index.range_search(self.transform.apply(self._rows(q, "range_search: ")), radius)

    def reset(self):
        """faiss reset(): drops the rows, keeps the training of both parts."""
        self.index.reset()
        self._stage = None

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """The base's rows [i0, i0 + n) (decoded where it stores codes) through transform.reverse_transform: fp32 device [n, d_in]."""
        _check_range(i0, n, self.ntotal)
        rows = self.index.reconstruct_n(i0, n) if hasattr(self.index, "reconstruct_n") else self.index.vectors[i0:i0 + n]
        return self.transform.reverse_transform(rows)

    # -- persistence (faiss.write_index / read_index of an IndexPreTransform, see index_io.py) ------------------------
    def save(self, fname: str, prefix: bytes = b"", append: bool = False):
        """prefix / append, load's offset / end: the record inside an enclosing one (RefineFlatIndex.save)."""
        from .index_io import write_pre_transform
        write_pre_transform(fname, self.transform.state(), self.ntotal, self.is_trained,
                            lambda f, pre: self.index.save(f, prefix=pre, append=append), prefix=prefix)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, offset: int = 0, end: Optional[int] = None) -> "PreTransformIndex":
        from .index_io import FOURCC_FLAT_IP, FOURCC_PQ, QT_FP16, read_pre_transform
        st, base = read_pre_transform(fname, offset, end)
        if base["fourcc"] == FOURCC_FLAT_IP:
            base_cls = FlatIPIndex
        elif base["fourcc"] == FOURCC_PQ:
            base_cls = PQIndex
        else:
            base_cls = SQFp16Index if base["qtype"] == QT_FP16 else SQ8Index
        index = base_cls.load(fname, device=device, id_base=id_base, offset=base["offset"], end=end)
        if index.ntotal != base["ntotal"]:
            raise ValueError(f"{fname}: the pre-transform header says {base['ntotal']} rows, its base index holds {index.ntotal}")
        return cls(PCAMatrix.from_state(st, device=index.device), index)
