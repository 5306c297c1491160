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

from . import _lib
from .index import _check_range
from .ivf import _IVFCells, check_ivf_args

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
        self._init_store(capacity, torch.float16)

    def train(self, x, niter: Optional[int] = None, seed: Optional[int] = None):
        """The coarse k-means (IVFFlatIndex.train's; see the class note).  niter=0 leaves the initial centroids (distinct sampled rows)."""
        self._train_cells(self._rows(x, "train: "), niter, seed)

    # -- rows ------------------------------------------------------------------------------------------------------
    def _encode_into(self, x: torch.Tensor, cells: torch.Tensor, codes: torch.Tensor, row0: int):
        """Code rows [row0, row0 + len(x)) of `codes` from the fp32 rows x and their cells (one kernel)."""
        n = x.shape[0]
        if x.data_ptr() % 16:
            x = x.clone()
        cent = self.centroids.contiguous() if self.by_residual else None
        _lib.check(self.lib.lrx_ivf_sq_fp16_encode_rows(_lib.ptr(x), x.stride(0) if n > 1 else self.d, n, self.d, _lib.ptr(cent), _lib.ptr(cells), self.nlist,
                                                        _lib.ptr(codes), row0, _lib.current_stream()))

    def _put(self, x: torch.Tensor, a: int, b: int):
        self._encode_into(x, self._assign[a:b], self._store, a)

    def stored_codes(self) -> torch.Tensor:
        """The codes as stored, cell by cell: fp16 [ntotal, d] (a view)."""
        return self._stored()

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """ORIGINAL rows [i0, i0 + n) decoded to fp32 [n, d]: float(code), plus centroid[cell] (one fp32 add) with by_residual."""
        _check_range(i0, n, self.ntotal)
        self._finalize()
        if n == 0:
            return torch.empty(0, self.d, dtype=torch.float32, device=self.device)
        out = self._store[self._positions(i0, n)].float()
        return out + self.centroids[self._assign[i0:i0 + n]] if self.by_residual else out

    def set_contents(self, centroids, codes, list_off, row_ids):
        """Replace the centroids ([nlist, d]) and the rows: `codes` fp16 [n, d] already in cell order, list_off int64 [nlist + 1] (ascending from
        0 to n), row_ids int64 [n] a permutation of 0 .. n - 1 (position -> original row): load() and tests."""
        codes = torch.as_tensor(codes)
        if codes.ndim != 2 or codes.shape[1] != self.d or codes.dtype != torch.float16:
            raise ValueError(f"set_contents: codes must be fp16 [n, {self.d}], got {codes.dtype} {tuple(codes.shape)}")
        lo, ri = self._check_cells(codes.shape[0], list_off, row_ids)
        self._set_centroids(torch.as_tensor(centroids))
        self._clear_rows()
        self._store = codes.to(self.device).contiguous().clone()
        self._set_cells(lo, ri)

    # -- search: the exact top k under the score of the class note -----------------------------------------------------------
    IVF_FAMILY, CODED = "sq_fp16", True

    def _store_operands(self):
        return (self._store[:self.ntotal],)

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
        idx = cls(st["d"], st["nlist"], nprobe=cls._load_nprobe(st), by_residual=st["by_residual"], device=device,
                  id_base=id_base)
        if st["is_trained"]:
            idx.set_contents(np.array(st["centroids"], copy=True), torch.from_numpy(np.array(st["codes"], copy=True)), st["list_off"], st["row_ids"])
        return idx
