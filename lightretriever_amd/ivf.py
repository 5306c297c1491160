"""Inverted-file flat index: the faiss IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT) surface over lrx_ivf_flat_ip_search
(csrc/lrx_search_ivf.h).

    idx = IVFFlatIndex(2048, nlist=1024, nprobe=32); idx.train(x); idx.add(x)
    D, I = idx.search(q, 100)            # the exact top 100 over the rows of each query's 32 best cells

k-means cells, the fp32 rows stored once, cell by cell, and only the `nprobe` best cells of a query scanned: at nprobe / nlist = 1/32 a single
query reads about 1/32 of the rows.  No fp16 shadow is kept.  Every scanned (query, row) pair is scored exactly -- the flat index's own bits --
so with nprobe == nlist the result IS FlatIPIndex.search's.

    lims, D, I = idx.range_search_probed(q, 0.8)     # every row of those cells scoring above 0.8, never cut at a k

range_search_probed / range_search_preassigned (lrx_ivf_flat_ip_range_search) live in _IVFCells, for the four inverted-file
indexes."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .index import FlatIPIndex, _as_rows, _check_range, _grown, _pq_update, _range_args, _range_empty
from .selector import RowSelector, check_selector
from .transform import linear_transform

MAX_NPROBE = 2048
MAX_K = 2048

def check_ivf_args(d: int, nlist: int, nprobe: int, who: str = "IVFFlatIndex"):
    if d % 32 != 0 or not 32 <= d <= 8192:
        raise ValueError(f"{who}: d={d} must be a multiple of 32 (32 .. 8192)")
    if nlist < 1:
        raise ValueError(f"{who}: nlist={nlist} must be >= 1")
    check_nprobe(nprobe, nlist, who)


def check_nprobe(nprobe: int, nlist: int, who: str = "IVFFlatIndex") -> int:
    if not 1 <= nprobe <= min(nlist, MAX_NPROBE):
        raise ValueError(f"{who}: nprobe={nprobe} out of range (1..min(nlist={nlist}, {MAX_NPROBE}))")
    return int(nprobe)


class _IVFCells:
    """What the inverted-file indexes (IVFFlatIndex here, IVFPQIndex, IVFSQIndex, IVFSQ8Index) share: the coarse quantiser -- a FlatIPIndex over
    k-means centroids -- and its training, the cell bookkeeping (`list_off`, `row_ids`, the host `list_sizes`, the cell `_assign` of every
    original row, `_nsorted`), the staging of append_slot / commit, add() and the rebuild of the cell order (_finalize) around two hooks, search()
    around one, and the range search over the probed cells (range_search_probed / range_search_preassigned).
    The three cell-major indexes keep their rows or codes in `_store`, row-major [capacity, d] by stored position (_init_store), which is
    reserved, permuted and mapped here; IVFPQIndex overrides _reserve / _permute over the blocked codes of its PQIndex.  A subclass brings
    _put (rows [a, b) into the store: a copy, or an encode), IVF_FAMILY / CODED / _store_operands (what _cells_op, the one place that picks the
    wrapper and lists its operands, needs to know of it), set_contents, reconstruct_n and persistence.
    After _finalize the cell order, the stored rows or codes and every result are a function of the centroids (and the subclass's training) and
    of the added rows in arrival order, and of nothing else that happened to the index -- how the adds were split, when a search rebuilt the
    order, reset, reload."""

    NITER = 10
    MAX_POINTS_PER_CENTROID = 256
    SEED = 1234
    ASSIGN_CHUNK_BYTES = 256 << 20      # score matrix [rows, nlist] of one assignment chunk

    def _init_cells(self, d: int, nlist: int, nprobe: int, capacity: int, device: Optional[torch.device], id_base: int):
        _lib.require_gpu()
        self.lib = _lib.lib()
        self.d, self.nlist, self.nprobe = int(d), int(nlist), int(nprobe)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.id_base = id_base
        self.ntotal = 0
        self.is_trained = False
        self.quantizer = FlatIPIndex(d, capacity=nlist, device=self.device)
        self._assign = torch.empty(max(capacity, 0), dtype=torch.int64, device=self.device)   # cell of ORIGINAL row r
        self._clear_rows()
        self._stage = None
        self._ws = None

    def _clear_rows(self):
        self.ntotal = 0
        self._nsorted = 0                 # positions [0, _nsorted) are in cell order; [_nsorted, ntotal) hold original rows _nsorted .. as added
        self.list_off = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
        self.row_ids = torch.empty(0, dtype=torch.int64, device=self.device)
        self.list_sizes = np.zeros(self.nlist, dtype=np.int64)

    @property
    def centroids(self) -> torch.Tensor:
        return self.quantizer.vectors

    # -- training ------------------------------------------------------------------------------------------------
    def _rows(self, x, where: str = "") -> torch.Tensor:
        x = _as_rows(x, self.d, where).to(device=self.device, dtype=torch.float32)
        return x if x.shape[0] == 0 or (x.stride(1) == 1 and (x.shape[0] == 1 or x.stride(0) % 4 == 0)) else x.contiguous()

    def _assign_l2(self, x: torch.Tensor, cent: torch.Tensor) -> torch.Tensor:
        """argmax_j (x . c_j - |c_j|^2 / 2) per row (the nearest centroid in L2), ties to the lower j -> int64 [n]."""
        b = (-(cent.double() ** 2).sum(dim=1) / 2).float().contiguous()
        chunk = max(1, self.ASSIGN_CHUNK_BYTES // (4 * self.nlist))
        out = torch.empty(x.shape[0], dtype=torch.int64, device=self.device)
        for s in range(0, x.shape[0], chunk):
            torch.argmax(linear_transform(x[s:s + chunk], cent, b), dim=1, out=out[s:s + chunk])
        return out

    def _train_cells(self, x: torch.Tensor, niter: Optional[int] = None, seed: Optional[int] = None):
        """Lloyd k-means of the coarse quantiser over the rows x (IVFFlatIndex's class note has the rules)."""
        n = x.shape[0]
        if n < self.nlist:
            raise ValueError(f"{type(self).__name__}.train: {n} training rows < nlist={self.nlist}")
        niter = self.NITER if niter is None else niter
        rng = np.random.default_rng(self.SEED if seed is None else seed)
        max_pts = self.nlist * self.MAX_POINTS_PER_CENTROID
        if n > max_pts:
            x = x[torch.from_numpy(np.sort(rng.permutation(n)[:max_pts])).to(self.device)]
            n = max_pts
        cent = x[torch.from_numpy(rng.permutation(n)[:self.nlist]).to(self.device)].contiguous()       # [nlist, d] distinct rows
        if niter > 0:
            x_t = x.double()[None]                                                         # [1, n, d]
            for _ in range(niter):
                codes = self._assign_l2(x, cent)
                cent = _pq_update(x_t, codes[None], self.nlist, cent[None], rng)[0].contiguous()
        self._set_centroids(cent)

    def _set_centroids(self, cent: torch.Tensor):
        self.quantizer.reset()
        self.quantizer.add(cent.to(self.device, torch.float32).reshape(self.nlist, self.d))
        self.is_trained = True

    def _cells_of(self, x: torch.Tensor, out: torch.Tensor):
        """out[i] = the cell of row i: its best centroid by inner product, ties to the lower cell (one coarse search per 262144 rows)."""
        for s in range(0, x.shape[0], 262144):
            out[s:s + 262144].copy_(self.quantizer.search(x[s:s + 262144], 1)[1][:, 0])

    def _reserve_assign(self, n_rows: int):
        if n_rows > self._assign.shape[0]:
            new = torch.empty(n_rows, dtype=torch.int64, device=self.device)
            new[:self.ntotal].copy_(self._assign[:self.ntotal])
            self._assign = new

    # -- rows ------------------------------------------------------------------------------------------------------
    def _init_store(self, capacity: int, dtype: torch.dtype):
        self.rebuild_chunk_rows = 262144
        self._store = torch.empty(max(capacity, 0), self.d, dtype=dtype, device=self.device)

    def _reserve(self, n_rows: int):
        """Room for n_rows rows: the store and `_assign` grow together."""
        if n_rows > self._store.shape[0]:
            new = torch.empty(n_rows, self.d, dtype=self._store.dtype, device=self.device)
            new[:self.ntotal].copy_(self._store[:self.ntotal])
            self._store = new
        self._reserve_assign(n_rows)

    def add(self, x):
        """faiss add(x f32[n, d]): each row goes to the cell of its best centroid by inner product and is stored (coded) at its arrival
        position -- _put -- (raises before train(), as faiss does)."""
        if not self.is_trained:
            raise RuntimeError(f"{type(self).__name__}.add: the index is not trained (call train() first)")
        x = self._rows(x, "add: ")
        n = x.shape[0]
        if n == 0:
            return
        a, b = self.ntotal, self.ntotal + n
        if b > self._assign.shape[0]:
            self._reserve(_grown(self._assign.shape[0], b))
        self._cells_of(x, self._assign[a:b])
        self._put(x, a, b)
        self.list_sizes = self.list_sizes + torch.bincount(self._assign[a:b], minlength=self.nlist).cpu().numpy()
        self.ntotal = b

    def _finalize(self):
        """The rows back into cell order (see IVFFlatIndex's class note): a no-op unless rows were added since the last search."""
        if self._nsorted == self.ntotal:
            return
        orig, perm = self._cell_order()
        self._permute(perm)
        self._set_cell_order(orig, perm)

    def _permute(self, perm: torch.Tensor):
        """Store row i becomes row perm[i] of the old store: a gather in chunks of `rebuild_chunk_rows` into a second buffer."""
        n = self.ntotal
        new = torch.empty(max(self._store.shape[0], n), self.d, dtype=self._store.dtype, device=self.device)
        for s in range(0, n, self.rebuild_chunk_rows):
            e = min(s + self.rebuild_chunk_rows, n)
            torch.index_select(self._store, 0, perm[s:e], out=new[s:e])
        self._store = new

    def _stored(self) -> torch.Tensor:
        """The store as it stands, cell by cell: [ntotal, d] (a view)."""
        self._finalize()
        return self._store[:self.ntotal]

    def _positions(self, i0: int, n: int) -> torch.Tensor:
        """The stored positions of ORIGINAL rows [i0, i0 + n)."""
        pos = torch.empty(self.ntotal, dtype=torch.int64, device=self.device)
        pos[self.row_ids] = torch.arange(self.ntotal, dtype=torch.int64, device=self.device)
        return pos[i0:i0 + n]

    @property
    def vectors(self) -> torch.Tensor:
        return self.reconstruct_n(0, self.ntotal)

    def _cell_order(self):
        """(orig, perm) of the rebuild: orig[pos] = the original row of every stored position as it stands (the ordered part, then the new
        rows as added), perm = the stable sort of their cells -- within a cell old rows (ascending) before new rows (ascending)."""
        n, ns = self.ntotal, self._nsorted
        orig = torch.cat([self.row_ids[:ns], torch.arange(ns, n, dtype=torch.int64, device=self.device)])
        return orig, torch.argsort(self._assign[orig], stable=True)

    def _set_cell_order(self, orig: torch.Tensor, perm: torch.Tensor):
        self.row_ids = orig[perm]
        self.list_off = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
        self.list_off[1:] = torch.from_numpy(np.cumsum(self.list_sizes)).to(self.device)
        self._nsorted = self.ntotal

    def _check_cells(self, n: int, list_off, row_ids):
        """set_contents' validation of (list_off, row_ids) for n stored rows -> the two as int64 numpy arrays."""
        lo = np.asarray(torch.as_tensor(list_off).cpu().numpy(), dtype=np.int64).reshape(-1)
        ri = np.asarray(torch.as_tensor(row_ids).cpu().numpy(), dtype=np.int64).reshape(-1)
        if lo.shape[0] != self.nlist + 1 or lo[0] != 0 or lo[-1] != n or (np.diff(lo) < 0).any():
            raise ValueError(f"set_contents: list_off must ascend from 0 to n={n} over nlist + 1 = {self.nlist + 1} entries")
        if ri.shape[0] != n or not np.array_equal(np.sort(ri), np.arange(n)):
            raise ValueError(f"set_contents: row_ids must be a permutation of 0 .. {n - 1}")
        return lo, ri

    def _set_cells(self, lo: np.ndarray, ri: np.ndarray):
        n = ri.shape[0]
        self.row_ids = torch.from_numpy(ri).to(self.device)
        self.list_off = torch.from_numpy(lo).to(self.device)
        self.list_sizes = np.diff(lo)
        self._assign = torch.empty(max(n, 0), dtype=torch.int64, device=self.device)
        self._assign[self.row_ids] = torch.repeat_interleave(torch.arange(self.nlist, device=self.device), torch.from_numpy(self.list_sizes).to(self.device))
        self.ntotal = self._nsorted = n

    def append_slot(self, n_rows: int) -> torch.Tensor:
        """A transient fp32 staging view for the next n rows: write them, then commit(n)."""
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
            self.add(rows)
        self._stage = None                             # staging released (stream-ordered by the allocator)

    def reset(self):
        """faiss reset(): drops the rows, keeps the training."""
        self._clear_rows()
        self._stage = None

    def max_scan_rows(self, nprobe: Optional[int] = None) -> int:
        """The most rows one query can scan: the sum of the nprobe largest cells (from the host copy of the sizes)."""
        nprobe = self.nprobe if nprobe is None else nprobe
        return int(np.sort(self.list_sizes)[::-1][:nprobe].sum())

    def _begin_search(self, q, k: Optional[int], nprobe: Optional[int], row_map: Optional[torch.Tensor]):
        """The checks every search starts with -> (q fp32 [Q, d] on the device, nprobe); the cell order is rebuilt when rows were added.
        k = None: a range search, which has none."""
        who = type(self).__name__
        if not self.is_trained:
            raise RuntimeError(f"{who}.search: the index is not trained")
        if k is not None and not 1 <= k <= MAX_K:
            raise ValueError(f"search: k={k} out of range (1..{MAX_K})")
        nprobe = check_nprobe(self.nprobe if nprobe is None else nprobe, self.nlist, who)
        if row_map is not None and not (row_map.is_cuda and row_map.dtype == torch.int64 and row_map.is_contiguous() and row_map.numel() >= self.ntotal):
            raise ValueError("row_map must be a contiguous int64 CUDA tensor of >= ntotal entries")
        q = _as_rows(q, self.d, "search: ", "Q").to(device=self.device, dtype=torch.float32).contiguous()
        if q.shape[0] and self._nsorted != self.ntotal:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.LrxError(f"{who}.search under graph capture: rows were added since the last search (run one eager search first)")
            self._finalize()
        return q, nprobe

    def search(self, q, k: int, nprobe: Optional[int] = None, row_map: Optional[torch.Tensor] = None, sel: Optional[RowSelector] = None):
        """-> (D f32[Q,k], I i64[Q,k]) device tensors: the top k, under the index's score of a scanned row (its class note), over the rows of each
        query's nprobe best cells (by inner product with the centroids), score descending, ties to the lower original row, (-FLT_MAX, -1)
        padding where those cells hold fewer than k rows.  I = id_base + row, or row_map[row] (int64 CUDA tensor of >= ntotal entries).
        nprobe: this call's (default: the index's).
        sel: a RowSelector over the ntotal ORIGINAL rows (faiss SearchParameters(sel=...)) -- the top k over the SELECTED rows
        of those cells, padding where fewer than k of them were scanned; the unfiltered result restricted to the selected rows, bit for bit.
        One selector for all queries; id_base / row_map apply after it.  Allowed under graph capture as a search without one: set_mask_ /
        set_rows_ between replays change the filter."""
        q, nprobe = self._begin_search(q, k, nprobe, row_map)
        sel = check_selector(sel, self.ntotal, self.device, f"{type(self).__name__}.search")
        if q.shape[0] == 0:
            return (torch.empty(0, k, dtype=torch.float32, device=self.device), torch.empty(0, k, dtype=torch.int64, device=self.device))
        probe_scores, probes = self.quantizer.search(q, nprobe)
        capture_error = (f"{type(self).__name__}.search under graph capture: the search workspaces must exist before the capture starts -- run one "
                         "eager search with the same number of queries, k and nprobe first")
        return self._topk_cells(q, k, probes, probe_scores, self.max_scan_rows(nprobe), row_map, capture_error, sel)

    # -- the library calls: ops.ivf_<IVF_FAMILY>_ip_topk / _range_search, or their *_sel siblings under a selector -----------------------
    # A subclass states IVF_FAMILY, _store_operands() (what its ops take between q and list_off) and CODED: whether its ops take probe_scores
    # and by_residual (the three over codes) or not (the flat one).  sel: the selector's words, as check_selector returns them, or None.
    def _cells_op(self, name: str, q, probes, probe_scores, sel):
        """-> (the wrapper ops.<name> or, under a selector, ops.<name>_sel; its operands up to the k or radius)."""
        a = [q, *self._store_operands(), self.list_off, self.row_ids, probes]
        if self.CODED:
            a.append(probe_scores)
        if sel is not None:
            name += "_sel"
            a.append(sel)
        if self.CODED:
            a.append(self.by_residual)
        return getattr(ops, name), a

    def _topk_cells(self, q, k, probes, probe_scores, max_scan_rows, row_map, capture_error, sel=None):
        fn, a = self._cells_op(f"ivf_{self.IVF_FAMILY}_ip_topk", q, probes, probe_scores, sel)
        return fn(*a, k, max_scan_rows, self.id_base, row_map, ws_slots=vars(self), capture_error=capture_error)

    def _range_cells(self, q, radius, probes, probe_scores, max_scan_rows, row_map, sel=None):
        fn, a = self._cells_op(f"ivf_{self.IVF_FAMILY}_ip_range_search", q, probes, probe_scores, sel)
        return fn(*a, radius, max_scan_rows, self.id_base, row_map, ws_slots=vars(self))

    def range_search(self, q, radius: float):
        raise NotImplementedError(f"{type(self).__name__}.range_search is not served (range search over the probed cells is a follow-up)")

    @staticmethod
    def _load_nprobe(st: dict) -> int:
        """A file's nprobe, clamped to what the constructor accepts."""
        return min(max(st["nprobe"], 1), st["nlist"], MAX_NPROBE)

    # -- range search over the probed cells -----------------------------------------------------------------
    def range_search_probed(self, q, radius: float, nprobe: Optional[int] = None, row_map: Optional[torch.Tensor] = None,
                            sel: Optional[RowSelector] = None):
        """-> (lims i64[Q + 1], D f32[lims[Q]], I i64[lims[Q]]) device tensors: every row of each query's nprobe best cells -- the cells search()
        scans -- whose score, the value search() reports for it, is strictly greater than `radius`; never cut at a k.  Query i's hits are
        D / I[lims[i]:lims[i + 1]] in SEGMENT order, faiss's for an IVF range search: its cells in probe order (best centroid first), inside
        a cell by stored position (ascending original row) -- not sorted by score, and not FlatIPIndex.range_search's ascending-row order.
        I = id_base + row, or row_map[row].  The coarse search of search(), then range_search_preassigned.  Reads the result length back
        to the host once: refused under graph capture.  NaN radius: ValueError.  sel: a RowSelector over the ntotal original rows (see
        search): only selected rows are hits, the order is unchanged."""
        radius = _range_args(type(self).__name__, radius)
        q, nprobe = self._begin_search(q, None, nprobe, row_map)
        sel = check_selector(sel, self.ntotal, self.device, f"{type(self).__name__}.range_search_probed")
        if q.shape[0] == 0 or self.ntotal == 0:
            return _range_empty(self.device, q.shape[0])
        probe_scores, probes = self.quantizer.search(q, nprobe)
        return self._range_cells(q, radius, probes, probe_scores, self.max_scan_rows(nprobe), row_map, sel)

    def range_search_preassigned(self, q, radius: float, probes: torch.Tensor, probe_scores: Optional[torch.Tensor] = None,
                                 row_map: Optional[torch.Tensor] = None, sel: Optional[RowSelector] = None):
        """faiss IndexIVF::range_search_preassigned(x, radius, keys, coarse_dis): range_search_probed over the caller's cells.  probes: int64
        [Q, nprobe] on the device, the cells of each query in the order their hits are wanted (an entry < 0 is skipped; one >= nlist is
        skipped and counted in lrx_device_error_count; a cell named twice is scanned once).  probe_scores: fp32 [Q, nprobe], the score of each
        cell's centroid for the query -- required by an index that codes residuals (by_residual), ignored by one that does not.  sel: as
        range_search_probed's."""
        who = type(self).__name__
        radius = _range_args(who, radius)
        if not (isinstance(probes, torch.Tensor) and probes.is_cuda and probes.dtype == torch.int64 and probes.dim() == 2):
            raise ValueError("range_search_preassigned: probes must be an int64 CUDA tensor [Q, nprobe]")
        q, _ = self._begin_search(q, None, probes.shape[1], row_map)
        sel = check_selector(sel, self.ntotal, self.device, f"{who}.range_search_preassigned")
        if probes.shape[0] != q.shape[0]:
            raise ValueError(f"range_search_preassigned: probes has {probes.shape[0]} rows for {q.shape[0]} queries")
        if getattr(self, "by_residual", False):
            if probe_scores is None:
                raise ValueError(f"range_search_preassigned: {who} codes residuals (by_residual): probe_scores (fp32 [Q, nprobe]) is required")
            if not (probe_scores.is_cuda and probe_scores.dtype == torch.float32 and probe_scores.shape == probes.shape):
                raise ValueError("range_search_preassigned: probe_scores must be an fp32 CUDA tensor of the shape of probes")
            probe_scores = probe_scores.contiguous()
        else:
            probe_scores = None
        if q.shape[0] == 0 or self.ntotal == 0:
            return _range_empty(self.device, q.shape[0])
        return self._range_cells(q, radius, probes.contiguous(), probe_scores, self.max_scan_rows(probes.shape[1]), row_map, sel)


class IVFFlatIndex(_IVFCells):
    """faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT): d, nlist, nprobe, ntotal, is_trained, id_base; train / add / search /
    reset / reconstruct_n / save / load / set_contents, and append_slot / commit as the other trainable shards have.
    d % 32 == 0, 32 <= d <= 8192; 1 <= nlist; 1 <= nprobe <= min(nlist, 2048); 1 <= k <= 2048.
    Range search: range_search_probed(q, radius, nprobe) and faiss's range_search_preassigned(q, radius, probes) -- every row of the probed
    cells with a score > radius, in segment order (_IVFCells).  The plain name range_search stays refused: a test pins it.

    Training: Lloyd k-means on the L2 objective (what faiss's Clustering minimises for a non-spherical IP index) with PQIndex's rules --
    np.random.default_rng(1234), at most 256 x nlist rows (sampled without replacement, row numbers sorted), initial centroids = nlist distinct
    sampled rows, NITER = 10, deterministic fp64 segmented sums, faiss's split of empty cells; niter=0 leaves the initial centroids.  The
    assignment is argmax_j (x . c_j - |c_j|^2 / 2), ties to the lower j: lrx_linear_transform (A = centroids, b = -|c|^2 / 2) over row chunks and
    an arg-max.  The same input and seed give the same centroid bits; they are not faiss's (its RNG differs).
    Coarse quantiser: a FlatIPIndex over the centroids (`quantizer`).  A row's cell at add() and a query's probe list at search() are its exact
    top-1 / top-nprobe by INNER PRODUCT, ties to the lower cell.
    Rows: fp32, held once, in cell order; inside a cell in ascending original row (faiss's insertion order).  `list_off` int64 [nlist + 1] and
    `row_ids` int64 [ntotal] (position -> original row) sit beside them, `list_sizes` (numpy) is the host copy of the cell sizes, so a search
    sizes its workspace without a device sync.  add() appends the rows as they come (one coarse search, one host read of the new cell sizes);
    the cell order is rebuilt lazily, at the first search after an add: a stable sort of the cell numbers and a gather of the rows in chunks
    of `rebuild_chunk_rows` into a second buffer -- two copies of the rows while it runs, never a third.
    Memory: 4 B/element + 16 B per row (row_ids, the row's cell) + the centroids (6 B/element: the quantiser keeps its shadow) + the search
    workspace (8 bytes per scanned row and query of a chunk, under 1 GiB).  NOT thread-safe."""

    def __init__(self, d: int, nlist: int, nprobe: int = 1, capacity: int = 0, device: Optional[torch.device] = None, id_base: int = 0):
        check_ivf_args(d, nlist, nprobe)
        self._init_cells(d, nlist, nprobe, capacity, device, id_base)
        self._init_store(capacity, torch.float32)

    def train(self, x, niter: Optional[int] = None, seed: Optional[int] = None):
        """Lloyd k-means (see the class note).  niter=0 leaves the initial centroids (distinct sampled rows)."""
        self._train_cells(self._rows(x, "train: "), niter, seed)

    # -- rows ------------------------------------------------------------------------------------------------------
    def _put(self, x: torch.Tensor, a: int, b: int):
        self._store[a:b].copy_(x)

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """ORIGINAL rows [i0, i0 + n) as an fp32 device tensor [n, d]."""
        _check_range(i0, n, self.ntotal)
        self._finalize()
        if n == 0:
            return torch.empty(0, self.d, dtype=torch.float32, device=self.device)
        return self._store[self._positions(i0, n)]

    def stored_rows(self) -> torch.Tensor:
        """The rows as stored, cell by cell: fp32 [ntotal, d] (a view)."""
        return self._stored()

    def set_contents(self, centroids, rows, list_off, row_ids):
        """Replace the centroids ([nlist, d]) and the rows: `rows` fp32 [n, d] already in cell order, list_off int64 [nlist + 1] (ascending from
        0 to n), row_ids int64 [n] a permutation of 0 .. n - 1 (position -> original row): load() and tests."""
        rows = torch.as_tensor(rows)
        if rows.ndim != 2 or rows.shape[1] != self.d:
            raise ValueError(f"set_contents: rows must be [n, {self.d}], got {tuple(rows.shape)}")
        lo, ri = self._check_cells(rows.shape[0], list_off, row_ids)
        self._set_centroids(torch.as_tensor(centroids))
        self._clear_rows()
        self._store = rows.to(self.device, torch.float32).contiguous().clone()
        self._set_cells(lo, ri)

    # -- search: the exact top k, every scanned (query, row) pair scored with the flat index's own bits --------------------------
    IVF_FAMILY, CODED = "flat", False

    def _store_operands(self):
        return (self._store[:self.ntotal],)

    # -- persistence (faiss.write_index / read_index of an IndexIVFFlat, see index_io.py) -------------------------------
    def save(self, fname: str):
        from .index_io import write_ivf_flat
        write_ivf_flat(fname, self.centroids.cpu().numpy(), self.list_sizes, self.stored_rows().cpu().numpy(), self.row_ids.cpu().numpy(), self.nprobe,
                       self.is_trained)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0) -> "IVFFlatIndex":
        from .index_io import read_ivf_flat
        st = read_ivf_flat(fname)
        idx = cls(st["d"], st["nlist"], nprobe=cls._load_nprobe(st), device=device, id_base=id_base)
        if st["is_trained"]:
            idx.set_contents(np.array(st["centroids"], copy=True), st["rows"], st["list_off"], st["row_ids"])
        return idx
