"""Graph index: a fixed-degree neighbour graph over the fp32 rows and a beam search on it -- the role faiss gives GpuIndexCagra / IndexHNSWCagra,
and what this package serves where the reference builds an IndexHNSWFlat (lrx_graph_ip_search / lrx_graph_detour_counts,
csrc/lrx_search_graph.h).

    idx = GraphFlatIndex(2048, degree=32, intermediate_degree=64); idx.add(x)
    D, I = idx.search(q, 100, ef_search=128)      # a few thousand rows scored per query, whatever the row count

The only index here whose search cost does not grow with the corpus: a query scores the rows its beam meets, each with the flat index's own
exact score, so a hit's score IS FlatIPIndex.search's for that row; which rows are met is approximate (recall < 1).  The build is exact and
deterministic: exact kNN lists from the flat search, detour counts (one integer kernel), a prune by rank and a merge with the reverse edges
under a fixed order rule -- no sequential insertion, no random levels.  faiss's own HNSW record is neither written nor read."""
from __future__ import annotations

import time
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .index import FlatIPIndex, _as_rows, _check_range

MAX_DEGREE = 128
MAX_INTERMEDIATE_DEGREE = 256
MAX_BEAM = 2048
MAX_ENTRY = 2048                 # entry rows one query hands the kernel
DEFAULT_N_ENTRY = 4096
KNN_BATCH = 1024                 # queries per flat search of the kNN step
FLT_MAX = float(np.finfo(np.float32).max)


def check_graph_args(d: int, degree: int, intermediate_degree: int, ef_search: int, search_width: int, who: str = "GraphFlatIndex"):
    if d % 32 != 0 or not 32 <= d <= 8192:
        raise ValueError(f"{who}: d={d} must be a multiple of 32 (32 .. 8192)")
    if degree % 8 != 0 or not 8 <= degree <= MAX_DEGREE:
        raise ValueError(f"{who}: degree={degree} must be a multiple of 8 (8 .. {MAX_DEGREE})")
    if not degree <= intermediate_degree <= MAX_INTERMEDIATE_DEGREE:
        raise ValueError(f"{who}: intermediate_degree={intermediate_degree} out of range (degree={degree} .. {MAX_INTERMEDIATE_DEGREE})")
    if not 1 <= search_width <= 8 or search_width * degree > 1024:
        raise ValueError(f"{who}: search_width={search_width} out of range (1 .. 8, search_width * degree <= 1024)")
    check_ef_search(ef_search, who)


def check_ef_search(ef_search: int, who: str = "GraphFlatIndex") -> int:
    if not 1 <= ef_search <= MAX_BEAM:
        raise ValueError(f"{who}: ef_search={ef_search} out of range (1 .. {MAX_BEAM})")
    return int(ef_search)


# -- the build, step by step (tests/graph_yardstick.py is the model of each) -----------------------------------------------------------
def knn_lists(store: FlatIPIndex, K: int) -> torch.Tensor:
    """Step 1 -> int32 [n, K]: knn[u] = the K best rows v != u by the store's exact score, score descending, ties to the lower row; -1 where
    n - 1 < K.  store.search(x[u0:u1], K + 1) in batches of at most KNN_BATCH queries with u dropped from its own list -- or the last entry,
    when more than K duplicates of u rank before it."""
    n = store.ntotal
    knn = torch.empty(n, K, dtype=torch.int32, device=store.device)
    x = store.vectors
    cols = torch.arange(K + 1, device=store.device)
    for u0 in range(0, n, KNN_BATCH):
        u1 = min(u0 + KNN_BATCH, n)
        I = store.search(x[u0:u1], K + 1)[1] - store.id_base
        own = I == torch.arange(u0, u1, device=store.device)[:, None]
        drop = torch.where(own.any(dim=1), own.int().argmax(dim=1), K)
        knn[u0:u1] = I[cols[None, :] != drop[:, None]].view(u1 - u0, K).to(torch.int32)
    return knn


def prune(knn: torch.Tensor, counts: torch.Tensor, R: int) -> torch.Tensor:
    """Step 3 -> int32 [n, R]: the rows at the R list positions with the fewest detours, ties to the lower position (a stable sort on
    counts * K + position); empty slots (-1) rank after every row."""
    n, K = knn.shape
    pos = torch.arange(K, device=knn.device, dtype=torch.int64)
    key = torch.where(knn >= 0, counts.to(torch.int64) * K + pos, torch.iinfo(torch.int64).max)
    order = torch.argsort(key, dim=1, stable=True)[:, :R]
    return torch.gather(knn, 1, order)


def merge_reverse(pruned: torch.Tensor) -> torch.Tensor:
    """Step 4 -> int32 [n, R]: rev[v] = the rows u with v in pruned[u], ordered by (position of v in pruned[u], u), cut to R / 2 entries;
    graph[u] = the first R distinct entries of pruned[u][:R/2] ++ rev[u] ++ pruned[u][R/2:], padded with -1.  Sorts only: the order rule
    makes the table a function of `pruned`."""
    n, R = pruned.shape
    dev = pruned.device
    h = R // 2
    # the (u, j) pairs in (j, u) order, then a stable sort by v = pruned[u][j]: inside a v the pairs stay in (j, u) order
    v = pruned.t().reshape(-1).to(torch.int64)
    u = torch.arange(n, device=dev, dtype=torch.int64).repeat(R)
    ok = v >= 0
    v, u = v[ok], u[ok]
    by_v = torch.argsort(v, stable=True)
    v, u = v[by_v], u[by_v]
    start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(v, minlength=n), 0, out=start[1:])
    rank = torch.arange(v.numel(), device=dev, dtype=torch.int64) - start[v]
    rev = torch.full((n, h), -1, dtype=torch.int32, device=dev)
    keep = rank < h
    rev[v[keep], rank[keep]] = u[keep].to(torch.int32)
    cat = torch.cat([pruned[:, :h], rev, pruned[:, h:]], dim=1)                      # [n, 3 R / 2]
    # first occurrences: after a stable sort of a row's values, an entry equal to its predecessor is a repeat of an earlier position
    vals, idx = torch.sort(cat, dim=1, stable=True)
    rep_sorted = torch.zeros_like(vals, dtype=torch.bool)
    rep_sorted[:, 1:] = vals[:, 1:] == vals[:, :-1]
    rep = torch.zeros_like(rep_sorted).scatter_(1, idx, rep_sorted)
    take = (cat >= 0) & ~rep
    slot = torch.cumsum(take, dim=1) - 1
    take &= slot < R
    graph = torch.full((n, R), -1, dtype=torch.int32, device=dev)
    rows = torch.arange(n, device=dev)[:, None].expand_as(cat)
    graph[rows[take], slot[take]] = cat[take]
    return graph


def entry_row_numbers(n: int, n_entry: int) -> np.ndarray:
    """The n_entry strided rows floor(i * n / n_entry), i < n_entry (distinct: n_entry <= n)."""
    return (np.arange(n_entry, dtype=np.int64) * n) // max(n_entry, 1)


class GraphFlatIndex:
    """d, degree, intermediate_degree, ef_search, search_width, n_entry, ntotal, id_base; add / append_slot / commit / reset / reconstruct_n /
    vectors / search / save / load.  d % 32 == 0, 32 <= d <= 8192; degree % 8 == 0, 8 <= degree <= 128; degree <= intermediate_degree <= 256;
    1 <= ef_search <= 2048; 1 <= search_width <= 8; 1 <= k <= 2048.

    Rows: a FlatIPIndex `store` WITH its fp16 shadow -- the build's kNN lists are flat searches over it.  The table `graph` int32 [ntotal, degree]
    (-1 = no edge) is built lazily, at the first search after rows changed (_finalize); incremental insertion is not served: ANY change of
    rows rebuilds the whole graph (ntotal / 1024 flat searches of 1024 queries, k = intermediate_degree + 1).
    Entry rows: `n_entry` strided rows floor(i * ntotal / n_entry) -- default min(ntotal, 4096) -- held as a small FlatIPIndex of their own.  A
    search asks it for each query's best min(beam, n_entry, 2048) through the flat search and hands those rows to the kernel: the caller owns
    the coarse step, as with the inverted-file indexes.  A connected component of the graph that holds no entry row cannot be reached: raise
    n_entry (n_entry = ntotal makes every row a start) for corpora of many small, mutually distant clusters.
    search(q, k, ef_search): beam = max(ef_search, k), as faiss's HNSW search does; results under the contract of lrx_graph_ip_search
    (include/lrx.h): exact scores, score descending, ties to the lower row, (-FLT_MAX, -1) where the beam holds fewer than k rows.
    Memory: the store's 6 B/element (4 fp32 + 2 shadow; dropping the shadow after the build is a follow-up) + 4 * degree B per row + the
    entry index (6 B/element of n_entry rows); while building, 12 * intermediate_degree B per row on top (lists, counts, sort keys).
    NOT thread-safe."""

    def __init__(self, d: int, degree: int = 32, intermediate_degree: int = 64, ef_search: int = 128, search_width: int = 4,
                 n_entry: Optional[int] = None, capacity: int = 0, device: Optional[torch.device] = None, id_base: int = 0):
        check_graph_args(d, degree, intermediate_degree, ef_search, search_width)
        if n_entry is not None and n_entry < 1:
            raise ValueError(f"GraphFlatIndex: n_entry={n_entry} must be >= 1")
        _lib.require_gpu()
        self.d, self.degree, self.intermediate_degree = int(d), int(degree), int(intermediate_degree)
        self.ef_search, self.search_width, self.n_entry = int(ef_search), int(search_width), n_entry
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.id_base = id_base
        self.store = FlatIPIndex(d, capacity=capacity, device=self.device)
        self.is_trained = True
        self.max_iterations = 0              # lrx_graph_ip_search's bound on the steps of a query (0: ceil(beam / width) + 32)
        self.build_times: dict = {}          # seconds of the last build's steps (knn / detours / prune_merge), device-synchronised
        self._ws = None
        self._drop_graph()

    def _drop_graph(self):
        self.graph: Optional[torch.Tensor] = None
        self.entry_rows: Optional[torch.Tensor] = None
        self._entries: Optional[FlatIPIndex] = None
        self._graph_rows = -1

    @property
    def ntotal(self) -> int:
        return self.store.ntotal

    # -- rows: the store's; any change drops the graph ----------------------------------------------------------------------------
    def add(self, x):
        x = _as_rows(x, self.d, "add: ")
        if x.shape[0]:
            self.store.add(x)
            self._graph_rows = -1

    def append_slot(self, n_rows: int) -> torch.Tensor:
        """Rows [ntotal, ntotal + n) of the store as a writable view (an encoder writes them in place); call commit(n) afterwards."""
        return self.store.append_slot(n_rows)

    def commit(self, n_rows: int):
        self.store.commit(n_rows)
        if n_rows > 0:
            self._graph_rows = -1

    def reset(self):
        self.store.reset()
        self._drop_graph()

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        _check_range(i0, n, self.ntotal)
        return self.store.vectors[i0:i0 + n].clone()

    @property
    def vectors(self) -> torch.Tensor:
        return self.store.vectors

    # -- the build ------------------------------------------------------------------------------------------------------------------
    def _n_entry_for(self, n: int) -> int:
        return min(n, DEFAULT_N_ENTRY if self.n_entry is None else self.n_entry)

    def _set_entries(self, rows: np.ndarray):
        self.entry_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(self.device)
        self._entries = FlatIPIndex(self.d, capacity=rows.shape[0], device=self.device)
        if rows.shape[0]:
            self._entries.add(self.store.vectors[self.entry_rows])

    def _finalize(self):
        """The graph and the entry index for the rows as they stand: a no-op unless rows changed since the last build."""
        n = self.ntotal
        if self._graph_rows == n and self.graph is not None:
            return
        t = [self._now()]
        knn = knn_lists(self.store, self.intermediate_degree)
        t.append(self._now())
        counts = ops.graph_detour_counts(knn)
        t.append(self._now())
        self.graph = merge_reverse(prune(knn, counts, self.degree))
        t.append(self._now())
        self.build_times = {"knn": t[1] - t[0], "detours": t[2] - t[1], "prune_merge": t[3] - t[2]}
        self._set_entries(entry_row_numbers(n, self._n_entry_for(n)))
        self._graph_rows = n

    def _now(self) -> float:
        torch.cuda.synchronize(self.device)
        return time.perf_counter()

    # -- search -------------------------------------------------------------------------------------------------------------------------
    def search(self, q, k: int, ef_search: Optional[int] = None, row_map: Optional[torch.Tensor] = None, sel=None):
        """-> (D f32[Q,k], I i64[Q,k]) device tensors (see the class note).  ef_search: this call's (default: the index's).  I = id_base + row,
        or row_map[row] (int64 CUDA tensor of >= ntotal entries).  sel: not served."""
        if sel is not None:
            raise NotImplementedError("GraphFlatIndex.search(sel=...) is not served (filtered search over the graph is out of scope)")
        return self._search(q, k, ef_search, row_map, False)

    def _search(self, q, k: int, ef_search: Optional[int], row_map: Optional[torch.Tensor], stats: bool):
        """search(), or with stats=True -> (D, I, S i32[Q,2] = steps taken, rows scored): tools."""
        if not 1 <= k <= MAX_BEAM:
            raise ValueError(f"search: k={k} out of range (1..{MAX_BEAM})")
        beam = max(check_ef_search(self.ef_search if ef_search is None else ef_search), k)
        if row_map is not None and not (row_map.is_cuda and row_map.dtype == torch.int64 and row_map.is_contiguous() and row_map.numel() >= self.ntotal):
            raise ValueError("row_map must be a contiguous int64 CUDA tensor of >= ntotal entries")
        q = _as_rows(q, self.d, "search: ", "Q").to(device=self.device, dtype=torch.float32).contiguous()
        Q = q.shape[0]
        if Q == 0 or self.ntotal == 0:
            out = (torch.full((Q, k), -FLT_MAX, dtype=torch.float32, device=self.device), torch.full((Q, k), -1, dtype=torch.int64, device=self.device))
            return out + (torch.zeros(Q, 2, dtype=torch.int32, device=self.device),) if stats else out
        if self._graph_rows != self.ntotal or self.graph is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.LrxError("GraphFlatIndex.search under graph capture: rows changed since the last search (run one eager search first)")
            self._finalize()
        n_start = min(beam, self.entry_rows.numel(), MAX_ENTRY)
        local = self._entries.search(q, n_start)[1]
        entries = torch.where(local >= 0, self.entry_rows[local.clamp(min=0)], local)
        return ops.graph_ip_topk(q, self.store.vectors, self.graph, entries, k, beam, self.search_width, self.max_iterations, self.id_base, row_map,
                                 stats=stats, ws_slots=vars(self))

    def range_search(self, q, radius: float):
        raise NotImplementedError("GraphFlatIndex.range_search is not served (a beam search has no radius; use FlatIPIndex.range_search)")

    # -- persistence: the store as faiss's IndexFlatIP record + a side file with the table ------------------------------------------------
    def save(self, fname: str):
        """`fname`: the store's flat record -- faiss.read_index gives an IndexFlatIP over the rows.  `fname + ".graph.npz"`: the table, the
        entry rows and the parameters.  faiss's own HNSW record (levels, offsets, neighbour lists) is NOT written: this graph has no levels."""
        self._finalize()
        self.store.save(fname)
        write_graph_file(fname, self.graph.cpu().numpy(), self.entry_rows.cpu().numpy(),
                         dict(d=self.d, ntotal=self.ntotal, degree=self.degree, intermediate_degree=self.intermediate_degree, ef_search=self.ef_search,
                              search_width=self.search_width, n_entry=-1 if self.n_entry is None else self.n_entry))

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0) -> "GraphFlatIndex":
        """The index save() wrote; ValueError when the side file's table, entry rows or parameters disagree with the store's rows."""
        st = read_graph_file(fname)
        idx = cls(st["d"], st["degree"], st["intermediate_degree"], st["ef_search"], st["search_width"], None if st["n_entry"] < 0 else st["n_entry"],
                  device=device, id_base=id_base)
        idx.store = FlatIPIndex.load(fname, device=idx.device)
        idx.set_graph(st["graph"], st["entry_rows"], st["ntotal"])
        return idx

    def set_graph(self, graph, entry_rows, ntotal: Optional[int] = None):
        """Install a table and entry rows for the rows as they stand (check_table's rules): load() and tests.  ntotal: what the table was built
        for, when the caller knows it."""
        graph, entry_rows = check_table(graph, entry_rows, self.ntotal, self.degree, self.store.d if self.store.d != self.d else None, ntotal)
        self.graph = torch.from_numpy(graph).to(self.device)
        self._set_entries(entry_rows)
        self._graph_rows = self.ntotal


PARAMS = ("d", "ntotal", "degree", "intermediate_degree", "ef_search", "search_width", "n_entry")      # the side file's `params`, in order (n_entry -1: default)


def write_graph_file(fname: str, graph: np.ndarray, entry_rows: np.ndarray, params: dict):
    np.savez(fname + ".graph.npz", graph=graph, entry_rows=entry_rows, params=np.array([params[p] for p in PARAMS], dtype=np.int64))


def read_graph_file(fname: str) -> dict:
    """`fname + ".graph.npz"` -> {graph, entry_rows, **params}, the table checked against the file's own parameters (check_table)."""
    path = fname + ".graph.npz"
    with np.load(path) as z:
        missing = [a for a in ("graph", "entry_rows", "params") if a not in z.files]
        if missing:
            raise ValueError(f"{path}: no {', '.join(missing)}")
        graph, entry_rows, params = z["graph"], z["entry_rows"], z["params"].reshape(-1)
    if params.shape[0] != len(PARAMS):
        raise ValueError(f"{path}: params holds {params.shape[0]} entries, expected {len(PARAMS)}")
    st = {p: int(v) for p, v in zip(PARAMS, params)}
    try:
        check_graph_args(st["d"], st["degree"], st["intermediate_degree"], st["ef_search"], st["search_width"], path)
        st["graph"], st["entry_rows"] = check_table(graph, entry_rows, st["ntotal"], st["degree"])
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    return st


def check_table(graph, entry_rows, n: int, degree: int, store_d: Optional[int] = None, built_for: Optional[int] = None):
    """-> (graph int32 [n, degree] C-contiguous, entry_rows int64 [1 .. n]) or ValueError: the table's shape and dtype, its entries in [-1, n),
    the entry rows in [0, n) (at least one unless n == 0), and -- when given -- the row count the table was built for and a store of another d."""
    graph, entry_rows = np.asarray(graph), np.asarray(entry_rows).reshape(-1)
    if store_d is not None:
        raise ValueError(f"the store holds rows of d={store_d}, not the index's")
    if built_for is not None and built_for != n:
        raise ValueError(f"graph table built for {built_for} rows, but the store holds {n}")
    if graph.ndim != 2 or graph.shape != (n, degree) or graph.dtype != np.int32:
        raise ValueError(f"graph must be int32 [{n}, {degree}], got {graph.dtype} {tuple(graph.shape)}")
    if graph.size and (graph.min() < -1 or graph.max() >= n):
        raise ValueError(f"graph entries must lie in [-1, {n})")
    if entry_rows.dtype.kind not in "iu" or entry_rows.shape[0] > max(n, 0) or (n and not entry_rows.size) or \
            (entry_rows.size and (entry_rows.min() < 0 or entry_rows.max() >= n)):
        raise ValueError(f"entry_rows must be 1 .. {n} integer rows in [0, {n})")
    return np.ascontiguousarray(graph), np.ascontiguousarray(entry_rows, dtype=np.int64)
