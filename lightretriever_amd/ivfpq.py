"""Inverted-file product-quantised index: the faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8, METRIC_INNER_PRODUCT) surface over
lrx_ivf_pq_ip_search (csrc/lrx_search_ivfpq.h).

    idx = IVFPQIndex(2048, nlist=1024, M=128, nprobe=32); idx.train(x); idx.add(x)
    D, I = idx.search(q, 100)            # the top 100 under the ADC score over the rows of each query's 32 best cells

IVFFlatIndex's cells over PQIndex's codes: M bytes per row, and only the `nprobe` best cells of a query are scanned -- at nprobe / nlist = 1/32
a query does about 1/32 of PQIndex's table lookups.  With by_residual (faiss's default) a row is coded as its residual to its cell's centroid
and a scanned row's score starts at the coarse score of its cell; without, the codes and -- probing every cell -- the result are PQIndex's."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .index import PQIndex, _check_range
from .ivf import _IVFCells, check_ivf_args

def check_ivfpq_args(d: int, nlist: int, M: int, nbits: int = 8, nprobe: int = 1):
    """The constructor's refusals (no GPU is needed): nbits != 8, d / M > 64, d outside what IVFFlatIndex and PQIndex both accept, nprobe."""
    if nbits != 8:
        raise NotImplementedError(f"IVFPQIndex: nbits={nbits} is not served (only 8)")
    if M <= 0 or d % M != 0:
        raise ValueError(f"IVFPQIndex: d={d} is not a multiple of M={M}")
    if d // M > 64:
        raise NotImplementedError(f"IVFPQIndex: sub-space dimension d / M = {d // M} > 64 is not served")
    check_ivf_args(d, nlist, nprobe, "IVFPQIndex")


class IVFPQIndex(_IVFCells):
    """faiss.IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8, METRIC_INNER_PRODUCT): d, nlist, nprobe, M, by_residual, ntotal, is_trained, id_base;
    train / add / search / reset / reconstruct_n / save / load / set_contents / append_slot / commit / max_scan_rows.
    d % 32 == 0, 32 <= d <= 8192, d % M == 0, d / M <= 64; nbits = 8; 1 <= nlist; 1 <= nprobe <= min(nlist, 2048); 1 <= k <= 2048.
    Range search: range_search_probed(q, radius, nprobe) and faiss's range_search_preassigned(q, radius, probes, probe_scores) -- every row of
    the probed cells with a score > radius, in segment order (_IVFCells in ivf.py).  The plain name range_search stays refused:
    a test pins it.

    Coarse quantiser: IVFFlatIndex's, from the code both share (`quantizer`, a FlatIPIndex over centroids trained by the same k-means: the same
    bits for the same input and seed).  A row's cell at add() and a query's probe list at search() are its exact top-1 / top-nprobe by INNER
    PRODUCT, ties to the lower cell.
    Codebooks: an internal PQIndex(d, M) (`pq`) holds them and the codes.  by_residual: trained on the residuals x - centroid[cell(x)] (one
    fp32 subtraction, the cell by add()'s rule) of the rows PQIndex's own sampler draws -- the draw is made first, so the residuals of a whole
    corpus are never materialised -- and equal to PQIndex(d, M).train(all residuals) bit for bit; otherwise trained on the rows themselves.
    train() needs max(nlist, 256) rows; `niter` (when given) is the iteration count of both k-means.
    Codes: M bytes per row in PQIndex's blocked layout, by stored position, in cell order; inside a cell in ascending original row.  `list_off`,
    `row_ids` and the host `list_sizes` as in IVFFlatIndex.  add() codes the rows (their residuals) at their arrival positions: one coarse
    search, one subtraction, lrx_pq_encode.  The cell order is rebuilt lazily, at the first search after an add: a stable sort of the cell
    numbers and the codes permuted as row-major rows (PQIndex.blocked_to_rows / rows_to_blocked).
    Score of a scanned row: fp32, (by_residual ? the coarse search's own exact score of its cell : 0) + the query's table entries of the row's
    codes in ascending m (include/lrx.h, lrx_ivf_pq_ip_search); top k by score descending, ties to the lower original row.
    Memory: M + 16 B per row + the centroids + the codebooks + the search workspace (M KiB of tables and 8 bytes per scanned row for every
    query of a chunk, under 1 GiB).  NOT thread-safe."""

    def __init__(self, d: int, nlist: int, M: int, nbits: int = 8, nprobe: int = 1, by_residual: bool = True, capacity: int = 0,
                 device: Optional[torch.device] = None, id_base: int = 0):
        check_ivfpq_args(d, nlist, M, nbits, nprobe)
        self._init_cells(d, nlist, nprobe, capacity, device, id_base)
        self.M, self.nbits, self.by_residual = int(M), int(nbits), bool(by_residual)
        self.pq = PQIndex(d, M, nbits, capacity=capacity, device=self.device)

    # -- training ------------------------------------------------------------------------------------------------
    def _residuals(self, x: torch.Tensor, cells: Optional[torch.Tensor] = None) -> torch.Tensor:
        """What the codebooks see of the rows x: x - centroid[cell] (one fp32 subtraction), or x itself without by_residual."""
        if not self.by_residual or x.shape[0] == 0:
            return x
        if cells is None:
            cells = torch.empty(x.shape[0], dtype=torch.int64, device=self.device)
            self._cells_of(x, cells)
        return x - self.centroids[cells]

    def train(self, x, niter: Optional[int] = None, seed: Optional[int] = None):
        """The coarse k-means (IVFFlatIndex.train's), then the codebooks (see the class note).  niter: of both (default: 10 and 25)."""
        x = self._rows(x, "train: ")
        need = max(self.nlist, PQIndex.KSUB)
        if x.shape[0] < need:
            raise ValueError(f"IVFPQIndex.train: {x.shape[0]} training rows < max(nlist={self.nlist}, {PQIndex.KSUB} centroids) = {need}")
        self._train_cells(x, niter, seed)
        rng, rows = self.pq.sample_rows(x.shape[0], seed)
        sample = x if rows is None else x[torch.from_numpy(rows).to(self.device)]
        self.pq.train(self._residuals(sample), niter=niter, rng=rng)

    # -- rows ------------------------------------------------------------------------------------------------------
    def _reserve(self, n_rows: int):
        self._reserve_assign(n_rows)                   # (the codes grow inside `pq`)

    def _put(self, x: torch.Tensor, a: int, b: int):
        for s in range(0, b - a, 262144):
            self.pq.add(self._residuals(x[s:s + 262144], self._assign[a + s:min(a + s + 262144, b)]))

    def _permute(self, perm: torch.Tensor):
        self.pq._codes = self.pq.rows_to_blocked(self.pq.blocked_to_rows(self.pq._codes, self.ntotal)[perm])

    def reset(self):
        """faiss reset(): drops the rows, keeps the training."""
        super().reset()
        self.pq.reset()

    def stored_codes(self) -> torch.Tensor:
        """The codes as stored, cell by cell: row-major uint8 [ntotal, M] (a copy: the stored layout is blocked)."""
        self._finalize()
        return self.pq.codes()

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """ORIGINAL rows [i0, i0 + n) decoded to fp32 [n, d]: centroid[cell] + the decoded codes (one fp32 add); the decode alone without
        by_residual."""
        _check_range(i0, n, self.ntotal)
        self._finalize()
        out = torch.empty(n, self.d, dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        picked = self.pq.rows_to_blocked(self.pq.blocked_to_rows(self.pq._codes, self.ntotal)[self._positions(i0, n)])
        _lib.check(self.lib.lrx_pq_decode_rows(_lib.ptr(picked), 0, n, _lib.ptr(self.pq.centroids), self.d, self.M, _lib.ptr(out), self.d,
                                               _lib.current_stream()))
        return self.centroids[self._assign[i0:i0 + n]] + out if self.by_residual else out

    def set_contents(self, centroids, pq_centroids, codes, list_off, row_ids):
        """Replace the centroids ([nlist, d]), the codebooks ([M, 256, d / M]) and the rows: `codes` uint8 [n, M] already in cell order, list_off
        int64 [nlist + 1] (ascending from 0 to n), row_ids int64 [n] a permutation of 0 .. n - 1 (position -> original row): load() and tests."""
        codes = torch.as_tensor(codes)
        if codes.ndim != 2 or codes.shape[1] != self.M or codes.dtype != torch.uint8:
            raise ValueError(f"set_contents: codes must be uint8 [n, {self.M}], got {codes.dtype} {tuple(codes.shape)}")
        lo, ri = self._check_cells(codes.shape[0], list_off, row_ids)
        self._set_centroids(torch.as_tensor(centroids))
        self._clear_rows()
        self.pq.set_contents(pq_centroids, codes)
        self._set_cells(lo, ri)

    # -- search: the top k under the ADC score of the class note ------------------------------------------------------------
    IVF_FAMILY, CODED = "pq", True

    def _store_operands(self):
        return (self.pq._codes, self.pq.centroids)

    # -- persistence (faiss.write_index / read_index of an IndexIVFPQ, see index_io.py) ---------------------------------
    def save(self, fname: str, prefix: bytes = b"", append: bool = False):
        from .index_io import write_ivf_pq
        codes = self.stored_codes().cpu().numpy()
        write_ivf_pq(fname, self.centroids.cpu().numpy(), self.pq.centroids.cpu().numpy(), self.list_sizes, codes, self.row_ids.cpu().numpy(), self.nprobe,
                     self.by_residual, self.is_trained, prefix=prefix, append=append)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, offset: int = 0, end: Optional[int] = None) -> "IVFPQIndex":
        from .index_io import read_ivf_pq
        st = read_ivf_pq(fname, offset, end)
        idx = cls(st["d"], st["nlist"], st["M"], nprobe=cls._load_nprobe(st), by_residual=st["by_residual"], device=device,
                  id_base=id_base)
        if st["is_trained"]:
            idx.set_contents(np.array(st["centroids"], copy=True), np.array(st["pq_centroids"], copy=True), torch.from_numpy(np.array(st["codes"], copy=True)),
                             st["list_off"], st["row_ids"])
        return idx
