"""Inverted-file 8-bit scalar-quantised index: the faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit | QT_8bit_uniform,
METRIC_INNER_PRODUCT) surface ("IVF...,SQ8") over lrx_ivf_sq8_ip_search (csrc/lrx_search_ivfsq8.h).

    idx = IVFSQ8Index(2048, nlist=1024, nprobe=32); idx.train(x); idx.add(x)
    D, I = idx.search(q, 100)            # the exact top 100, under the 8-bit store's score, over the rows of each query's 32 best cells

IVFFlatIndex's cells over SQ8Index's quantiser: 1 byte per element instead of 4, every scanned (query, row) pair scored exactly over the
decoded row.  With by_residual (faiss's default) a row is coded as its residual to its cell's centroid -- the range is trained on the
residuals -- and a scanned row's score starts at the coarse score of its cell; without, the codes are SQ8Index's for the same `trained`."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .index import _check_range
from .ivf import _IVFCells, check_ivf_args

QTYPES = {"QT_8bit": 0, "QT_8bit_uniform": 2}     # faiss ScalarQuantizer::QuantizerType


def check_ivfsq8_args(d: int, nlist: int, qtype: str = "QT_8bit", nprobe: int = 1):
    """The constructor's refusals (no GPU is needed): any quantiser type but the two 8-bit ones, and what IVFFlatIndex refuses."""
    if qtype not in QTYPES:
        raise NotImplementedError(f"IVFSQ8Index: qtype {qtype!r} is not served (only {sorted(QTYPES)}; 'QT_fp16' is IVFSQIndex's)")
    check_ivf_args(d, nlist, nprobe, "IVFSQ8Index")


class IVFSQ8Index(_IVFCells):
    """faiss.IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit | QT_8bit_uniform, METRIC_INNER_PRODUCT): d, nlist, nprobe, qtype,
    by_residual, trained, ntotal, is_trained, id_base; train / add / search / reset / reconstruct_n / save / load / set_contents / append_slot /
    commit / max_scan_rows.  d % 32 == 0, 32 <= d <= 8192; 1 <= nlist; 1 <= nprobe <= min(nlist, 2048); 1 <= k <= 2048.
    Range search: range_search_probed(q, radius, nprobe) and faiss's range_search_preassigned(q, radius, probes, probe_scores) -- every row of
    the probed cells with a score > radius, in segment order (_IVFCells in ivf.py).  The plain name range_search stays refused:
    a test pins it.

    Coarse quantiser: IVFFlatIndex's, from the code both share (the same centroid bits for the same input and seed).  train() runs that k-means
    and then trains the range as faiss's train_encoder does: every training row goes to its coarse top-1 cell, the residual is
    fl32(x - centroid[cell]) with by_residual (the row itself without), and `trained` = vmin ++ (vmax - vmin) of the residuals by SQ8Index.train's
    arithmetic (per dimension, or over all elements for QT_8bit_uniform; NaN ignored, an empty range is 0).  No RNG beyond the k-means.
    Codes: uint8, row-major [ntotal, d] by stored position, in cell order; inside a cell in ascending original row.  The code of v and the
    decoded element are SQ8Index's (include/lrx.h, lrx_ivf_sq8_ip_search).  add() codes the rows at their arrival positions: one coarse top-1,
    lrx_ivf_sq8_encode_rows.  The cell order is rebuilt lazily, at the first search after an add: a stable sort of the cell numbers and a gather
    of the code rows in chunks of `rebuild_chunk_rows` into a second buffer -- two copies while it runs, never a third.
    Score of a scanned row: (float)(B + the fp64 sum of q_i * y_i) over the decoded row y, B = the coarse search's own exact score of the row's
    cell with by_residual, 0 without; top k by score descending, ties to the lower original row.
    Memory: 1 B/element + 16 B per row (row_ids, the row's cell) + the centroids + `trained` + the search workspace.  NOT thread-safe."""

    TRAIN_CHUNK_ROWS = 262144

    def __init__(self, d: int, nlist: int, qtype: str = "QT_8bit", nprobe: int = 1, by_residual: bool = True, capacity: int = 0,
                 device: Optional[torch.device] = None, id_base: int = 0):
        check_ivfsq8_args(d, nlist, qtype, nprobe)
        self._init_cells(d, nlist, nprobe, capacity, device, id_base)
        self.qtype, self._qt, self.by_residual = qtype, QTYPES[qtype], bool(by_residual)
        self.uniform = self._qt == 2
        self.trained = torch.zeros(2 if self.uniform else 2 * d, dtype=torch.float32, device=self.device)
        self._init_store(capacity, torch.uint8)

    def train(self, x, niter: Optional[int] = None, seed: Optional[int] = None):
        """The coarse k-means (IVFFlatIndex.train's), then the range of the training rows' residuals (see the class note)."""
        x = self._rows(x, "train: ")
        self._train_cells(x, niter, seed)
        mm = torch.empty(2, self.d, dtype=torch.float32, device=self.device)
        mm[0].fill_(float("inf"))
        mm[1].fill_(float("-inf"))
        cent = self.centroids
        for s in range(0, x.shape[0], self.TRAIN_CHUNK_ROWS):
            xs = x[s:s + self.TRAIN_CHUNK_ROWS]
            if self.by_residual:
                xs = xs - cent[self.quantizer.search(xs, 1)[1][:, 0]]
            _lib.check(self.lib.lrx_sq8_train_minmax(_lib.ptr(xs), xs.shape[0], xs.stride(0) if xs.shape[0] > 1 else self.d, self.d, _lib.ptr(mm),
                                                     _lib.current_stream()))
        mn, mx = mm[0], mm[1]
        if self.uniform:
            mn, mx = mn.min().reshape(1), mx.max().reshape(1)
        empty = mn > mx                                # no value that is not NaN: vmin = vdiff = 0
        mn, mx = mn.masked_fill(empty, 0.0), mx.masked_fill(empty, 0.0)
        self.trained = torch.cat([mn, mx - mn]).contiguous()

    # -- rows ------------------------------------------------------------------------------------------------------
    def _encode_into(self, x: torch.Tensor, cells: torch.Tensor, codes: torch.Tensor, row0: int):
        """Code rows [row0, row0 + len(x)) of `codes` from the fp32 rows x and their cells (one kernel)."""
        n = x.shape[0]
        if x.data_ptr() % 16:
            x = x.clone()
        cent = self.centroids.contiguous() if self.by_residual else None
        _lib.check(self.lib.lrx_ivf_sq8_encode_rows(_lib.ptr(x), x.stride(0) if n > 1 else self.d, n, self.d, _lib.ptr(cent), _lib.ptr(cells), self.nlist,
                                                    _lib.ptr(self.trained), self._qt, _lib.ptr(codes), row0, _lib.current_stream()))

    def _put(self, x: torch.Tensor, a: int, b: int):
        self._encode_into(x, self._assign[a:b], self._store, a)

    def stored_codes(self) -> torch.Tensor:
        """The codes as stored, cell by cell: uint8 [ntotal, d] (a view)."""
        return self._stored()

    def decode_stored(self, p0: int = 0, n: Optional[int] = None, residual: bool = False) -> torch.Tensor:
        """Stored POSITIONS [p0, p0 + n) decoded to fp32 [n, d] (lrx_ivf_sq8_decode_rows): the rows themselves, or with residual=True what the
        codes hold (no centroid added)."""
        self._finalize()
        n = self.ntotal - p0 if n is None else n
        _check_range(p0, n, self.ntotal)
        out = torch.empty(n, self.d, dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        add = self.by_residual and not residual
        cells = self._assign[self.row_ids[p0:p0 + n]].contiguous() if add else None
        cent = self.centroids.contiguous() if add else None
        _lib.check(self.lib.lrx_ivf_sq8_decode_rows(_lib.ptr(self._store), p0, n, self.d, _lib.ptr(self.trained), self._qt, _lib.ptr(cent), _lib.ptr(cells),
                                                    self.nlist, _lib.ptr(out), self.d, _lib.current_stream()))
        return out

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """ORIGINAL rows [i0, i0 + n) decoded to fp32 [n, d]: the decoded code, plus centroid[cell] (one fp32 add) with by_residual."""
        _check_range(i0, n, self.ntotal)
        self._finalize()
        if n == 0:
            return torch.empty(0, self.d, dtype=torch.float32, device=self.device)
        out = torch.empty(self.ntotal, self.d, dtype=torch.float32, device=self.device) if (i0, n) == (0, self.ntotal) else None
        if out is not None:                            # every row: decode in stored order, scatter to the original rows
            out[self.row_ids] = self.decode_stored()
            return out
        codes = self._store[self._positions(i0, n)].contiguous()
        cells = self._assign[i0:i0 + n].contiguous() if self.by_residual else None
        cent = self.centroids.contiguous() if self.by_residual else None
        out = torch.empty(n, self.d, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.lrx_ivf_sq8_decode_rows(_lib.ptr(codes), 0, n, self.d, _lib.ptr(self.trained), self._qt, _lib.ptr(cent), _lib.ptr(cells), self.nlist,
                                                    _lib.ptr(out), self.d, _lib.current_stream()))
        return out

    def set_contents(self, centroids, trained, codes, list_off, row_ids):
        """Replace the centroids ([nlist, d]), the range (`trained`: vmin ++ vdiff) and the rows: `codes` uint8 [n, d] already in cell order,
        list_off int64 [nlist + 1] (ascending from 0 to n), row_ids int64 [n] a permutation of 0 .. n - 1 (position -> original row): load() and
        tests."""
        codes = torch.as_tensor(codes)
        t = torch.as_tensor(trained).to(torch.float32).reshape(-1)
        if t.numel() != self.trained.numel():
            raise ValueError(f"set_contents: trained must hold {self.trained.numel()} floats for {self.qtype}, got {t.numel()}")
        if codes.ndim != 2 or codes.shape[1] != self.d or codes.dtype != torch.uint8:
            raise ValueError(f"set_contents: codes must be uint8 [n, {self.d}], got {codes.dtype} {tuple(codes.shape)}")
        lo, ri = self._check_cells(codes.shape[0], list_off, row_ids)
        self._set_centroids(torch.as_tensor(centroids))
        self.trained = t.to(self.device).contiguous().clone()
        self._clear_rows()
        self._store = codes.to(self.device).contiguous().clone()
        self._set_cells(lo, ri)

    # -- search: the exact top k under the score of the class note -----------------------------------------------------------
    IVF_FAMILY, CODED = "sq8", True

    def _store_operands(self):
        return (self._store[:self.ntotal], self.trained, self._qt)

    # -- persistence (faiss.write_index / read_index of an IndexIVFScalarQuantizer, see index_io.py) ----------------------
    def save(self, fname: str, prefix: bytes = b"", append: bool = False):
        from .index_io import write_ivf_sq8
        codes = self.stored_codes().cpu().numpy()
        write_ivf_sq8(fname, self.centroids.cpu().numpy(), self.trained.cpu().numpy(), self._qt, self.list_sizes, codes, self.row_ids.cpu().numpy(), self.nprobe,
                      self.by_residual, self.is_trained, prefix=prefix, append=append)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, offset: int = 0, end: Optional[int] = None) -> "IVFSQ8Index":
        from .index_io import read_ivf_sq8
        st = read_ivf_sq8(fname, offset, end)
        qtype = {v: k for k, v in QTYPES.items()}[st["qtype"]]
        idx = cls(st["d"], st["nlist"], qtype, nprobe=cls._load_nprobe(st), by_residual=st["by_residual"], device=device,
                  id_base=id_base)
        if st["is_trained"]:
            idx.set_contents(np.array(st["centroids"], copy=True), np.array(st["trained"], copy=True), torch.from_numpy(np.array(st["codes"], copy=True)),
                             st["list_off"], st["row_ids"])
        return idx
