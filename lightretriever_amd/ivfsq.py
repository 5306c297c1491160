"""Inverted-file fp16 scalar-quantised index: the faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_fp16, METRIC_INNER_PRODUCT) surface
over lrx_ivf_sq_fp16_ip_search (csrc/lrx_search_ivfsq.h).

    idx = IVFSQIndex(2048, nlist=1024, nprobe=32); idx.train(x); idx.add(x)
    D, I = idx.search(q, 100)            # the exact top 100, under the fp16 store's score, over the rows of each query's 32 best cells

IVFFlatIndex's cells over SQFp16Index's codes: 2 bytes per element instead of 4, every scanned (query, row) pair scored exactly over the codes.
(8-bit codes over the same cells: IVFSQ8Index, ivfsq8.py.)  With by_residual (faiss's default) a row is coded as its residual to its cell's centroid and a scanned row's score starts at the coarse score
of its cell; without, the codes and -- probing every cell -- the result are SQFp16Index's, bit for bit."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .index import _check_range, _grown
from .ivf import MAX_NPROBE, _IVFCells, check_ivf_args

_CAPTURE_WS_ERROR = ("IVFSQIndex.search under graph capture: the search workspaces must exist before the capture starts -- run one eager "
                     "search with the same number of queries, k and nprobe first")


def check_ivfsq_args(d: int, nlist: int, qtype: str = "QT_fp16", nprobe: int = 1):
    """The constructor's refusals (no GPU is needed): any quantiser type but QT_fp16, and what IVFFlatIndex refuses."""
    if qtype != "QT_fp16":
        raise NotImplementedError(f"IVFSQIndex: qtype {qtype!r} is not served (only 'QT_fp16'; QT_8bit over cells is a follow-up)")
    check_ivf_args(d, nlist, nprobe, "IVFSQIndex")


class IVFSQIndex(_IVFCells):
    """faiss.IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_fp16, METRIC_INNER_PRODUCT): d, nlist, nprobe, qtype, by_residual, ntotal,
    is_trained, id_base; train / add / search / reset / reconstruct_n / save / load / set_contents / append_slot / commit / max_scan_rows.
    d % 32 == 0, 32 <= d <= 8192; qtype = "QT_fp16"; 1 <= nlist; 1 <= nprobe <= min(nlist, 2048); 1 <= k <= 2048.
    Range search: range_search_probed(q, radius, nprobe) and faiss's range_search_preassigned(q, radius, probes, probe_scores) -- every row of
    the probed cells with a score > radius, in segment order (_IVFCells in ivf.py).  The plain name range_search stays refused:
    a test pins it.

    Coarse quantiser: IVFFlatIndex's, from the code both share (`quantizer`, a FlatIPIndex over centroids trained by the same k-means: the same
    bits for the same input and seed).  train() is that k-means and nothing else: the fp16 quantiser has nothing to train.  A row's cell at add()
    and a query's probe list at search() are its exact top-1 / top-nprobe by INNER PRODUCT, ties to the lower cell.
    Codes: fp16, row-major [ntotal, d] by stored position, in cell order; inside a cell in ascending original row.  code = fp16(v), SQFp16Index's
    rounding (round-to-nearest-even, saturating at +-65504 where faiss gives inf); v = x, or with by_residual x - centroid[cell] (one fp32
    subtraction).  add() codes the rows at their arrival positions: one coarse top-1, lrx_ivf_sq_fp16_encode_rows.  `list_off`, `row_ids` and
    the host `list_sizes` as in IVFFlatIndex.  The cell order is rebuilt lazily, at the first search after an add: a stable sort of the cell
    numbers and a gather of the code rows in chunks of `rebuild_chunk_rows` into a second buffer -- two copies while it runs, never a third.
    Score of a scanned row: (float)(B + the fp64 sum of q_i * float(code_i)), B = the coarse search's own exact score of the row's cell with
    by_residual, 0 without (include/lrx.h, lrx_ivf_sq_fp16_ip_search); top k by score descending, ties to the lower original row.
    Memory: 2 B/element + 16 B per row (row_ids, the row's cell) + the centroids + the search workspace (8 bytes per scanned row and query of
    a chunk, under 1 GiB).  NOT thread-safe."""

    def __init__(self, d: int, nlist: int, qtype: str = "QT_fp16", nprobe: int = 1, by_residual: bool = True, capacity: int = 0,
                 device: Optional[torch.device] = None, id_base: int = 0):
        check_ivfsq_args(d, nlist, qtype, nprobe)
        self._init_cells(d, nlist, nprobe, capacity, device, id_base)
        self.qtype, self.by_residual = qtype, bool(by_residual)
        self.rebuild_chunk_rows = 262144
        self._codes = torch.empty(max(capacity, 0), d, dtype=torch.float16, device=self.device)

    def train(self, x, niter: Optional[int] = None, seed: Optional[int] = None):
        """The coarse k-means (IVFFlatIndex.train's; see the class note).  niter=0 leaves the initial centroids (distinct sampled rows)."""
        self._train_cells(self._rows(x, "train: "), niter, seed)

    # -- rows ------------------------------------------------------------------------------------------------------
    def _reserve(self, n_rows: int):
        if n_rows > self._codes.shape[0]:
            new = torch.empty(n_rows, self.d, dtype=torch.float16, device=self.device)
            new[:self.ntotal].copy_(self._codes[:self.ntotal])
            self._codes = new
        self._reserve_assign(n_rows)

    def _encode_into(self, x: torch.Tensor, cells: torch.Tensor, codes: torch.Tensor, row0: int):
        """Code rows [row0, row0 + len(x)) of `codes` from the fp32 rows x and their cells (one kernel)."""
        n = x.shape[0]
        if x.data_ptr() % 16:
            x = x.clone()
        cent = self.centroids.contiguous() if self.by_residual else None
        _lib.check(self.lib.lrx_ivf_sq_fp16_encode_rows(_lib.ptr(x), x.stride(0) if n > 1 else self.d, n, self.d, _lib.ptr(cent), _lib.ptr(cells), self.nlist,
                                                        _lib.ptr(codes), row0, _lib.current_stream()))

    def add(self, x):
        """faiss add(x f32[n, d]): each row goes to the cell of its best centroid by inner product and is coded (its residual to that centroid
        with by_residual) at its arrival position (raises before train(), as faiss does)."""
        if not self.is_trained:
            raise RuntimeError("IVFSQIndex.add: the index is not trained (call train() first)")
        x = self._rows(x, "add: ")
        n = x.shape[0]
        if n == 0:
            return
        if self.ntotal + n > self._codes.shape[0]:
            self._reserve(_grown(self._codes.shape[0], self.ntotal + n))
        a, b = self.ntotal, self.ntotal + n
        self._cells_of(x, self._assign[a:b])
        self._encode_into(x, self._assign[a:b], self._codes, a)
        self.list_sizes = self.list_sizes + torch.bincount(self._assign[a:b], minlength=self.nlist).cpu().numpy()
        self.ntotal = b

    def _finalize(self):
        """The codes back into cell order (see the class note): a no-op unless rows were added since the last search."""
        if self._nsorted == self.ntotal:
            return
        n = self.ntotal
        orig, perm = self._cell_order()
        new = torch.empty(max(self._codes.shape[0], n), self.d, dtype=torch.float16, device=self.device)
        for s in range(0, n, self.rebuild_chunk_rows):
            e = min(s + self.rebuild_chunk_rows, n)
            torch.index_select(self._codes, 0, perm[s:e], out=new[s:e])
        self._codes = new
        self._set_cell_order(orig, perm)

    def stored_codes(self) -> torch.Tensor:
        """The codes as stored, cell by cell: fp16 [ntotal, d] (a view)."""
        self._finalize()
        return self._codes[:self.ntotal]

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """ORIGINAL rows [i0, i0 + n) decoded to fp32 [n, d]: float(code), plus centroid[cell] (one fp32 add) with by_residual."""
        _check_range(i0, n, self.ntotal)
        self._finalize()
        if n == 0:
            return torch.empty(0, self.d, dtype=torch.float32, device=self.device)
        pos = torch.empty(self.ntotal, dtype=torch.int64, device=self.device)
        pos[self.row_ids] = torch.arange(self.ntotal, dtype=torch.int64, device=self.device)
        out = self._codes[pos[i0:i0 + n]].float()
        return out + self.centroids[self._assign[i0:i0 + n]] if self.by_residual else out

    @property
    def vectors(self) -> torch.Tensor:
        return self.reconstruct_n(0, self.ntotal)

    def set_contents(self, centroids, codes, list_off, row_ids):
        """Replace the centroids ([nlist, d]) and the rows: `codes` fp16 [n, d] already in cell order, list_off int64 [nlist + 1] (ascending from
        0 to n), row_ids int64 [n] a permutation of 0 .. n - 1 (position -> original row): load() and tests."""
        codes = torch.as_tensor(codes)
        if codes.ndim != 2 or codes.shape[1] != self.d or codes.dtype != torch.float16:
            raise ValueError(f"set_contents: codes must be fp16 [n, {self.d}], got {codes.dtype} {tuple(codes.shape)}")
        lo, ri = self._check_cells(codes.shape[0], list_off, row_ids)
        self._set_centroids(torch.as_tensor(centroids))
        self._clear_rows()
        self._codes = codes.to(self.device).contiguous().clone()
        self._set_cells(lo, ri)

    # -- search --------------------------------------------------------------------------------------------------
    def search(self, q, k: int, nprobe: Optional[int] = None, row_map: Optional[torch.Tensor] = None):
        """-> (D f32[Q,k], I i64[Q,k]) device tensors: the exact top k under the score of the class note over the rows of each query's nprobe
        best cells, score descending, ties to the lower original row, (-FLT_MAX, -1) padding where those cells hold fewer than k rows.
        I = id_base + row, or row_map[row] (int64 CUDA tensor of >= ntotal entries).  nprobe: this call's (default: the index's)."""
        q, nprobe = self._begin_search(q, k, nprobe, row_map)
        if q.shape[0] == 0:
            return (torch.empty(0, k, dtype=torch.float32, device=self.device), torch.empty(0, k, dtype=torch.int64, device=self.device))
        probe_scores, probes = self.quantizer.search(q, nprobe)
        return ops.ivf_sq_fp16_ip_topk(q, self._codes[:self.ntotal], self.list_off, self.row_ids, probes, probe_scores, self.by_residual, k,
                                       self.max_scan_rows(nprobe), self.id_base, row_map, ws_slots=vars(self), capture_error=_CAPTURE_WS_ERROR)

    def _range_cells(self, q, radius, probes, probe_scores, max_scan_rows, row_map):
        return ops.ivf_sq_fp16_ip_range_search(q, self._codes[:self.ntotal], self.list_off, self.row_ids, probes, probe_scores, self.by_residual, radius,
                                               max_scan_rows, self.id_base, row_map, ws_slots=vars(self))

    def range_search(self, q, radius: float):
        raise NotImplementedError("IVFSQIndex.range_search is not served (range search over the probed cells is a follow-up)")

    # -- persistence (faiss.write_index / read_index of an IndexIVFScalarQuantizer, see index_io.py) ----------------------
    def save(self, fname: str, prefix: bytes = b"", append: bool = False):
        from .index_io import write_ivf_sq
        codes = self.stored_codes().cpu().numpy()
        write_ivf_sq(fname, self.centroids.cpu().numpy(), self.list_sizes, codes, self.row_ids.cpu().numpy(), self.nprobe, self.by_residual,
                     self.is_trained, prefix=prefix, append=append)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, offset: int = 0, end: Optional[int] = None) -> "IVFSQIndex":
        from .index_io import read_ivf_sq
        st = read_ivf_sq(fname, offset, end)
        idx = cls(st["d"], st["nlist"], nprobe=min(max(st["nprobe"], 1), st["nlist"], MAX_NPROBE), by_residual=st["by_residual"], device=device,
                  id_base=id_base)
        if st["is_trained"]:
            idx.set_contents(np.array(st["centroids"], copy=True), torch.from_numpy(np.array(st["codes"], copy=True)), st["list_off"], st["row_ids"])
        return idx
