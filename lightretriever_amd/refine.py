"""Exact re-ranking over a lossy index: the faiss.IndexRefineFlat / faiss.IndexRefine surface, over lrx_flat_ip_rerank / lrx_sq_fp16_ip_rerank
(csrc/lrx_search_rerank.h).

    idx = RefineFlatIndex(PQIndex(2048, 128), k_factor=4); idx.train(x); idx.add(x)
    D, I = idx.search(q, 100)            # the 400 best rows by PQ score, rescored from the fp32 rows: the best 100 of them

search() takes k_base = int(k * k_factor) candidates from the base index, rescores exactly those rows from a full-precision copy (the refine
store) and returns the best k: scores are the store's own bits -- FlatIPIndex's (float) of the fp64 sum of the fp32 products, or SQFp16Index's
over its codes -- in descending order, ties to the lower row, (-FLT_MAX, -1) padding.  With k_base >= ntotal the result IS the store's search."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .index import FlatIPIndex, PQIndex, SQ8Index, SQFp16Index, _as_rows, _check_range, _workspace
from .ivfpq import IVFPQIndex
from .ivfsq import IVFSQIndex
from .ivfsq8 import IVFSQ8Index
from .transform import PreTransformIndex

BASES = (PQIndex, SQ8Index, SQFp16Index, PreTransformIndex, IVFPQIndex, IVFSQIndex, IVFSQ8Index)
STORES = (FlatIPIndex, SQFp16Index)
MAX_K_BASE = 2048         # candidates per query the rerank takes: the most any base search delivers

_CAPTURE_WS_ERROR = ("RefineFlatIndex.search under graph capture: the rerank workspace must exist before the capture starts -- run one eager "
                     "search with the same number of queries and k first")


def k_base_of(k: int, k_factor: float) -> int:
    """faiss's rule (IndexRefine::search): k_base = idx_t(k * k_factor)."""
    return int(k * k_factor)


def check_k_factor(k_factor) -> float:
    k_factor = float(k_factor)
    if not k_factor >= 1:
        raise ValueError(f"RefineFlatIndex: k_factor={k_factor} must be >= 1")
    return k_factor


def check_k_base(k: int, k_factor: float, who: str = "RefineFlatIndex.search") -> int:
    """k_base for (k, k_factor), or ValueError when it is past what the rerank takes."""
    if k < 1:
        raise ValueError(f"{who}: k={k} must be >= 1")
    kb = k_base_of(k, k_factor)
    if kb > MAX_K_BASE:
        raise ValueError(f"{who}: k_base = int(k * k_factor) = int({k} * {k_factor}) = {kb} > {MAX_K_BASE} (the limit of the base searches and the rerank)")
    return kb


def rerank(q: torch.Tensor, store, cand: torch.Tensor, k: int, id_base: int = 0, row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None):
    """(D f32[Q,k], I i64[Q,k]): the exact top k of the candidate rows cand (int64 [Q, n_cand] device, rows may be strided; < 0 skipped,
    >= store.ntotal skipped and counted in lrx_device_error_count) under `store`'s score -- a FlatIPIndex (fp32 rows) or an SQFp16Index (codes).
    q: fp32 [Q, d] contiguous on the store's device.  ws_slots: a dict that keeps the workspace between calls (key "_ws")."""
    lib = _lib.lib()
    Q, n_cand = cand.shape
    D = torch.empty(Q, k, dtype=torch.float32, device=q.device)
    I = torch.empty(Q, k, dtype=torch.int64, device=q.device)
    if Q == 0:
        return D, I
    ws = _workspace({} if ws_slots is None else ws_slots, "_ws", int(lib.lrx_ip_rerank_workspace_bytes(Q, n_cand, k)), q.device,
                    None if ws_slots is None else _CAPTURE_WS_ERROR)
    ld_cand = cand.stride(0) if Q > 1 else n_cand
    tail = (_lib.ptr(q), Q, _lib.ptr(cand), n_cand, ld_cand, k, int(id_base), _lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(),
            _lib.current_stream())
    if isinstance(store, SQFp16Index):
        _lib.check(lib.lrx_sq_fp16_ip_rerank(_lib.ptr(store._xb), store.ntotal, store.d, *tail))
    else:
        x = store._x
        _lib.check(lib.lrx_flat_ip_rerank(_lib.ptr(x) if x.shape[0] else None, store.ntotal, x.stride(0) if x.shape[0] > 1 else store.d, store.d, *tail))
    return D, I


class RefineFlatIndex:
    """faiss.IndexRefineFlat(base_index) / faiss.IndexRefine(base_index, refine_index): d, ntotal, device, is_trained (the base's), id_base
    (applied to the results only), k_factor; train / add / reset / reconstruct_n / append_slot / commit / search / save / load.
    base_index: a PQIndex, SQ8Index, SQFp16Index, PreTransformIndex, IVFPQIndex, IVFSQIndex or IVFSQ8Index with id_base 0 (this index owns the id offset); anything else:
    TypeError.  refine_index (the store): None -- a fresh FlatIPIndex(d) WITHOUT its fp16 shadow (the rows are gathered, never streamed:
    4 B/element, not 6) -- or a FlatIPIndex, or an SQFp16Index (2 B/element: faiss IndexRefine(base, IndexScalarQuantizer(QT_fp16))); same d
    (a PreTransformIndex's d is d_in) and the same ntotal as the base.  k_factor >= 1.
    Memory: the base's + the store's + the rerank workspace (8 bytes per candidate; lrx_ip_rerank_workspace_bytes).
    append_slot(n) is the store's own slot (for a flat store the final fp32 rows, so an encoder writes them in place); commit(n) trains the
    base on those rows if it is untrained, adds them to the base, then commits the store -- the same bits as add().  NOT thread-safe."""

    def __init__(self, base_index, refine_index=None, k_factor: float = 1.0):
        if not isinstance(base_index, BASES):
            raise TypeError(f"RefineFlatIndex: base index {type(base_index).__name__} is not served (only {', '.join(c.__name__ for c in BASES)})")
        if refine_index is not None and not isinstance(refine_index, STORES):
            raise TypeError(f"RefineFlatIndex: refine index {type(refine_index).__name__} is not served (only {', '.join(c.__name__ for c in STORES)})")
        self.k_factor = check_k_factor(k_factor)
        if base_index.id_base != 0:
            raise ValueError(f"RefineFlatIndex: the base index's id_base={base_index.id_base} must be 0 (set id_base on the RefineFlatIndex)")
        if refine_index is None:
            refine_index = FlatIPIndex(base_index.d, device=base_index.device)
            refine_index.shadow_f16 = False
        if refine_index.d != base_index.d:
            raise ValueError(f"RefineFlatIndex: the refine index's d={refine_index.d} is not the base's d={base_index.d}")
        if refine_index.ntotal != base_index.ntotal:
            raise ValueError(f"RefineFlatIndex: the base index holds {base_index.ntotal} rows, the refine index {refine_index.ntotal}")
        self.base_index, self.refine_index = base_index, refine_index
        self.id_base = 0
        self._slot = None
        self._ws = None

    d = property(lambda self: self.base_index.d)
    ntotal = property(lambda self: self.refine_index.ntotal)
    device = property(lambda self: self.refine_index.device)
    is_trained = property(lambda self: bool(getattr(self.base_index, "is_trained", True)))

    # -- rows ------------------------------------------------------------------------------------------------------
    def _rows(self, x, where: str) -> torch.Tensor:
        x = _as_rows(x, self.d, where).to(device=self.device, dtype=torch.float32)
        return x if x.shape[0] == 0 or x.stride(1) == 1 else x.contiguous()

    def train(self, x):
        """Trains the base index (the store needs no training)."""
        self.base_index.train(self._rows(x, "train: "))

    def add(self, x):
        """faiss add(x f32[n, d]) to both indexes; raises before train(), as faiss does."""
        if not self.is_trained:
            raise RuntimeError("RefineFlatIndex.add: the index is not trained (call train() first)")
        x = self._rows(x, "add: ")
        self.base_index.add(x)
        self.refine_index.add(x)

    def append_slot(self, n_rows: int) -> torch.Tensor:
        """The store's own slot for the next n rows (FlatIPIndex: its final fp32 rows; SQFp16Index: its staging): write them, then commit(n)."""
        self._slot = self.refine_index.append_slot(n_rows)
        return self._slot

    def commit(self, n_rows: int):
        if n_rows > 0:
            if self._slot is None or n_rows > self._slot.shape[0]:
                raise ValueError(f"commit({n_rows}): only {0 if self._slot is None else self._slot.shape[0]} slot rows")
            rows = self._slot[:n_rows]
            if not self.is_trained:
                self.base_index.train(rows)
            self.base_index.add(rows)                  # (before the store's commit: SQFp16Index.commit releases its staging)
        self._slot = None
        self.refine_index.commit(n_rows)

    def reset(self):
        """faiss reset(): drops the rows of both indexes, keeps the base's training."""
        self.base_index.reset()
        self.refine_index.reset()
        self._slot = None

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """Rows [i0, i0 + n) from the refine store (faiss IndexRefine::reconstruct): fp32 device tensor [n, d]."""
        _check_range(i0, n, self.ntotal)
        if isinstance(self.refine_index, SQFp16Index):
            return self.refine_index.reconstruct_n(i0, n)
        return self.refine_index.vectors[i0:i0 + n].clone()

    # -- search --------------------------------------------------------------------------------------------------
    def search(self, q, k: int, k_factor: Optional[float] = None, row_map: Optional[torch.Tensor] = None):
        """-> (D f32[Q,k], I i64[Q,k]) device tensors: base.search(q, k_base = int(k * k_factor))'s rows rescored from the store, best k by
        (score desc, row asc), (-FLT_MAX, -1) padding; I = id_base + row, or row_map[row] (int64 CUDA tensor of >= ntotal entries).
        k_factor: this call's (default: the index's).  k_base > 2048: ValueError."""
        k_base = check_k_base(k, self.k_factor if k_factor is None else check_k_factor(k_factor))
        if self.base_index.id_base != 0:
            raise ValueError(f"RefineFlatIndex.search: the base index's id_base={self.base_index.id_base} must be 0")
        if self.base_index.ntotal != self.refine_index.ntotal:
            raise ValueError(f"RefineFlatIndex.search: the base index holds {self.base_index.ntotal} rows, the refine index {self.refine_index.ntotal}")
        if row_map is not None and not (row_map.is_cuda and row_map.dtype == torch.int64 and row_map.is_contiguous() and row_map.numel() >= self.ntotal):
            raise ValueError("row_map must be a contiguous int64 CUDA tensor of >= ntotal entries")
        q = _as_rows(q, self.d, "search: ", "Q").to(device=self.device, dtype=torch.float32).contiguous()
        if q.shape[0] == 0:
            return (torch.empty(0, k, dtype=torch.float32, device=self.device), torch.empty(0, k, dtype=torch.int64, device=self.device))
        _, cand = self.base_index.search(q, k_base)
        return rerank(q, self.refine_index, cand, k, self.id_base, row_map, vars(self))

    def range_search(self, q, radius: float):
        raise NotImplementedError("RefineFlatIndex.range_search is not served (faiss's IndexRefine has none)")

    # -- persistence (faiss.write_index / read_index of an IndexRefine, see index_io.py) -------------------------------
    def save(self, fname: str):
        from .index_io import write_refine
        write_refine(fname, self.d, self.ntotal, self.is_trained, self.k_factor, lambda f, prefix: self.base_index.save(f, prefix=prefix),
                     lambda f: self.refine_index.save(f, append=True))

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0) -> "RefineFlatIndex":
        from .index_io import FOURCC_FLAT_IP, FOURCC_IVF_PQ, FOURCC_IVF_SQ, FOURCC_PQ, FOURCC_PRE_TRANSFORM, QT_FP16, ivf_sq_qtype, read_refine
        st = read_refine(fname)
        b, r = st["base"], st["store"]
        if b["fourcc"] == FOURCC_PQ:
            base_cls = PQIndex
        elif b["fourcc"] == FOURCC_PRE_TRANSFORM:
            base_cls = PreTransformIndex
        elif b["fourcc"] == FOURCC_IVF_PQ:
            base_cls = IVFPQIndex
        elif b["fourcc"] == FOURCC_IVF_SQ:
            base_cls = IVFSQIndex if ivf_sq_qtype(fname, b["offset"], b["end"]) == QT_FP16 else IVFSQ8Index   # (each reader refuses the other's record by name)
        else:
            base_cls = SQFp16Index if b["qtype"] == QT_FP16 else SQ8Index
        base = base_cls.load(fname, device=device, offset=b["offset"], end=b["end"])
        if r["fourcc"] == FOURCC_FLAT_IP:
            store = FlatIPIndex.load(fname, device=base.device, offset=r["offset"], end=r["end"], shadow_f16=False)
        else:
            store = SQFp16Index.load(fname, device=base.device, offset=r["offset"], end=r["end"])
        idx = cls(base, store, k_factor=st["k_factor"])
        idx.id_base = id_base
        return idx
