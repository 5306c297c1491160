"""HBM-resident inner-product index shards: the faiss.IndexFlatIP surface the reference uses (retriever/faiss_index.py:20-73: add / search /
reset / ntotal), backed by lrx_flat_ip_search, its fp16 scalar-quantised and product-quantised siblings, and the binary flat index (IndexBinaryFlat)."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional

import numpy as np
import torch

from . import _lib


_SHARDS = weakref.WeakValueDictionary()   # fp32 storage pointer -> FlatIPIndex / SQFp16Index (lets the encoder recognise a shard slot it writes into)


def shard_of(out: torch.Tensor):
    """(index, first_row) when `out` is a view of whole rows of a live shard's fp32 storage (FlatIPIndex rows, SQFp16Index staging), else
    None.  LrxEncoder.encode_packed uses it to hand the shard's fp16 shadow rows (or codes) and bounds to the encoder's last kernel
    (lrx_encode_packed_shard)."""
    if not _SHARDS or out.dtype != torch.float32 or out.ndim != 2:
        return None
    idx = _SHARDS.get(out.untyped_storage().data_ptr())
    if idx is None or out.shape[1] != idx.d or out.stride(0) != idx._x.stride(0) or out.stride(1) != 1:
        return None
    off = out.data_ptr() - idx._x.data_ptr()
    row_bytes = idx._x.stride(0) * 4
    if off < 0 or off % row_bytes:
        return None
    return idx, off // row_bytes


def _as_rows(x, d: int, where: str = "", rows: str = "n") -> torch.Tensor:
    """x (torch tensor on any device, or numpy) as a tensor, checked to be [rows, d] (ValueError "{where}expected [{rows},{d}], got ...")."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(x)
    if x.ndim != 2 or x.shape[1] != d:
        raise ValueError(f"{where}expected [{rows},{d}], got {tuple(x.shape)}")
    return x


def _grow_blocks(buf: torch.Tensor, n_rows: int, width: int, keep_rows: int, zero: bool = False) -> torch.Tensor:
    """`buf` (flat, whole 128-row blocks of `width` elements per row), or a larger copy of it (zero- or empty-filled) when it holds fewer than
    `n_rows` rows; the copy keeps the blocks that hold rows [0, keep_rows)."""
    need = -(-max(n_rows, 0) // 128) * 128 * width
    if need <= buf.numel():
        return buf
    new = (torch.zeros if zero else torch.empty)(need, dtype=buf.dtype, device=buf.device)
    n_old = min(buf.numel(), -(-keep_rows // 128) * 128 * width)
    if n_old:
        new[:n_old].copy_(buf[:n_old])
    return new


def _grown(have: int, need: int) -> int:
    """Rows to reserve when `need` rows no longer fit `have`: at least half as many again, so that repeated appends copy O(n) rows in all."""
    return max(need, int(have * 1.5) + 1)


def _workspace(slots: dict, key, need: int, device, capture_error: Optional[str] = None) -> torch.Tensor:
    """slots[key] (a uint8 workspace), regrown to `need` bytes when smaller.  The old block is dropped before the new one is allocated, so
    the caching allocator can reuse its memory.  capture_error: raise it instead of allocating under HIP-graph capture."""
    ws = slots.get(key)
    if ws is None or ws.numel() < need:
        if capture_error is not None and torch.cuda.is_current_stream_capturing():
            raise _lib.LrxError(capture_error)
        ws = slots[key] = None
        ws = slots[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _check_range(i0: int, n: int, ntotal: int):
    if i0 < 0 or n < 0 or i0 + n > ntotal:
        raise ValueError(f"reconstruct_n({i0}, {n}) outside [0, {ntotal})")


def _uncovered(intervals: list, a: int, b: int):
    """The maximal sub-ranges of [a, b) that no (start, end) interval covers, in ascending order."""
    pos = a
    for s, e in sorted(intervals):
        s, e = max(s, a), min(e, b)
        if e <= pos:
            continue
        if s > pos:
            yield pos, min(s, b)
        pos = max(pos, e)
    if pos < b:
        yield pos, b


def _range_call(device, Q: int, chunk: int, call):
    """What every range_search shares: the queries in host chunks of `chunk`, each one library call `call(s, n, lims, D, I, capacity)` over
    queries [s, s + n) whose outputs are sized by a first guess of 1024 hits per query and resized once if that is short (the library writes
    nothing then and the retry's result is the same: every path is deterministic); the chunks' results are stitched into one (lims, D, I).
    Synchronises with the host once per library call (the length of its result)."""
    lims = torch.zeros(Q + 1, dtype=torch.int64, device=device)
    parts = []
    for s in range(0, Q, chunk):
        nq = min(chunk, Q - s)
        lc = lims[s:s + nq + 1] if s == 0 else torch.empty(nq + 1, dtype=torch.int64, device=device)
        cap = nq * 1024
        for attempt in range(2):
            Dc = torch.empty(cap, dtype=torch.float32, device=device)
            Ic = torch.empty(cap, dtype=torch.int64, device=device)
            call(s, nq, lc, Dc, Ic, cap)
            n = int(lc[-1].item())
            if n <= cap:
                break
            cap = n
        parts.append((lc, Dc[:n], Ic[:n], n))
    if len(parts) == 1:
        return lims, parts[0][1], parts[0][2]
    off = 0
    for j, (lc, _, _, n) in enumerate(parts):
        s = j * chunk
        lims[s + 1:s + lc.shape[0]] = lc[1:] + off
        off += n
    return lims, torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts])


def _range_args(name: str, radius) -> float:
    """The checks every range_search starts with: refused under graph capture before anything is launched, NaN radius refused."""
    if torch.cuda.is_current_stream_capturing():
        raise _lib.LrxError(f"{name}.range_search under graph capture: the result length is read back to the host")
    radius = float(radius)
    if radius != radius:
        raise ValueError("range_search: radius is NaN")
    return radius


def _range_empty(device, Q: int):
    return (torch.zeros(Q + 1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.float32, device=device),
            torch.empty(0, dtype=torch.int64, device=device))


_CAPTURE_WS_ERROR = ("FlatIPIndex.search under graph capture: the search workspace must exist before the capture starts -- "
                     "run one eager search with the same number of queries and k first")


class _TiledIPIndex:
    """What FlatIPIndex and SQFp16Index share: rows streamed by the bounded inner-product search from a tiled fp16 layout (include/lrx.h:
    [128-row block][64-wide k-slice] tiles of 16 KiB, fragment-major inside), the {max |row|, max |row - fp16(row)|} bounds pair, the
    fp32 storage or staging view the encoder recognises (shard_of), and the search driver: query chunking under max_workspace_bytes, the
    fork of a call's library chunks over `chunk_lanes` internal streams, per-lane workspaces, wire_out / row_map, last_list_counts.
    A subclass keeps its own storage (reserve / append_slot / shard_sink / commit / add / save / load) and points the driver at its rows
    with four hooks:
      _search_ws_bytes(flags)                     -> f(ntotal, d, nq, k): workspace bytes of one library call of nq queries
      _search_rows()                              -> (row stride of the fp32 rows, the tiled fp16 rows the search streams or None)
      _lib_chunk_queries(n, k, flags, has_xb)     -> queries per library chunk of a call of n queries
      _search_chunk(qc, Dc, Ic, k, ws, stream, xb, ldx, flags, row_map, wire)   one library call over queries qc on `stream`
    The rows, the tiled fp16 rows and the bounds an index holds, and what it returns, are a function of the committed rows in arrival order and
    of nothing else that happened to it -- reserve, slots that were never committed, reset, reload, shadow_f16 / two_pass toggles."""
    # lrx_flat_ip_search_bounded flags (_lib.SEARCH_FILTER_*): which filter the bounded search runs.  A class-level default that tests and A/B
    # tools override (per index or for all); the hits do not depend on it.  (Round 2 had a process-global switch inside the library.)
    search_flags = _lib.SEARCH_FILTER_AUTO
    # the bounded search (filter pass + exact rescoring); FlatIPIndex.two_pass = False forces the six-product path for every search
    two_pass = True
    _D_ALIGN = 32

    def __init__(self, d: int, device: Optional[torch.device], id_base: int):
        _lib.require_gpu()
        if d % self._D_ALIGN != 0:
            raise ValueError(f"{type(self).__name__}: d={d} must be a multiple of {self._D_ALIGN}")
        self.lib = _lib.lib()
        self.d = d
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.ntotal = 0
        self.id_base = id_base  # added to local row numbers (global row of this shard's row 0)
        self._ws = None                      # search workspace of lane 0 (the only one unless searches are pipelined over lanes)
        self._lane_ws: dict = {}             # lane != 0 -> its own workspace: searches in flight on different HIP streams must not share one
        self.chunk_lanes = 2                 # a search of more queries than one library chunk (256) alternates its chunks over this many internal streams
        self._chunk_streams = None
        self._last_search = None             # what last_list_counts() needs to find the statistics of the last two-pass search
        # {max |row|, max |row - fp16(row)|} over the committed rows, kept on the device (no host sync): the error bound of the fp16
        # filter pass is built from them
        self._bounds = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.max_workspace_bytes = 12 << 30  # search(): cap of the search workspace; larger query batches are chunked
        self._xb: Optional[torch.Tensor] = None   # the tiled fp16 rows (FlatIPIndex: shadow, SQFp16Index: codes), whole 128-row blocks
        self._shadow_rows = 0                # committed rows [0, _shadow_rows) have valid tiled rows
        self._fused: list = []               # row intervals whose tiled rows + bounds the encoder has already written
        self._x = torch.empty(0, d, dtype=torch.float32, device=self.device)

    def _set_storage(self, x: torch.Tensor):
        if self._x.numel():
            _SHARDS.pop(self._x.untyped_storage().data_ptr(), None)
        self._x = x
        if x.numel():
            _SHARDS[x.untyped_storage().data_ptr()] = self

    def reset(self):
        self.ntotal = 0
        self._shadow_rows = 0
        self._bounds.zero_()
        self._fused = []

    def shadow_rows(self, n: Optional[int] = None) -> torch.Tensor:
        """The tiled fp16 rows as a row-major [n, d] fp16 tensor (a copy: the stored layout is tiled): tests and tools."""
        n = self.ntotal if n is None else n
        if self._xb is None:
            raise ValueError("this index keeps no fp16 shadow")
        nb = -(-n // 128)
        # tile = [16-row group w][k-step ks][fq][fi][8]  ->  row 128 b + 16 w + fi, column 64 s + 32 ks + 8 fq + j
        t = self._xb[:nb * 128 * self.d].view(nb, self.d // 64, 8, 2, 4, 16, 8)          # b, s, w, ks, fq, fi, j
        return t.permute(0, 2, 5, 1, 3, 4, 6).reshape(nb * 128, self.d)[:n]

    # -- search --------------------------------------------------------------------------------------------------
    def _lane_workspace(self, lane: int, need: int, user_stream: Optional["torch.cuda.Stream"] = None) -> torch.Tensor:
        """The workspace of `lane`, grown to `need` bytes.  user_stream: the stream its kernels will run on when that is not the stream
        current now (the internal chunk streams): the caching allocator is told, so that a later regrow / free cannot hand the block to the
        caller's stream while kernels of that stream still use it."""
        # (an allocation made under HIP-graph capture lives in the graph's private pool: the index would keep pointing at memory that goes
        # back to the allocator with the graph -- the memory-access fault of round 2's capture probe)
        ws = _workspace(vars(self) if lane == 0 else self._lane_ws, "_ws" if lane == 0 else lane, need, self.device, _CAPTURE_WS_ERROR)
        if user_stream is not None and user_stream != torch.cuda.current_stream():
            ws.record_stream(user_stream)
        return ws

    def _fit_chunk(self, Q: int, ws_bytes) -> int:
        """Queries per host chunk: Q, or the largest of 256, 128, 64, ... whose workspace ws_bytes(chunk) stays under max_workspace_bytes."""
        chunk = Q
        while chunk > 1 and int(ws_bytes(chunk)) > int(self.max_workspace_bytes):
            chunk = 256 if chunk > 256 else (128 if chunk > 128 else chunk // 2)
        return chunk

    def search(self, q, k: int, wire_out: Optional[torch.Tensor] = None, row_map: Optional[torch.Tensor] = None, lane: int = 0):
        """-> (D f32[Q,k], I i64[Q,k]) device tensors, descending scores, ids = id_base + row, ties -> lower id,
        (-FLT_MAX, -1) padding when k > ntotal.  wire_out (int64 [Q,k], optional): also filled with the exchange words of a row-sharded
        search (lrx_pack_topk's format, `row_map` applied) by the last kernel of the search itself.  lane: which of the index's search
        workspaces to use -- searches that may be in flight at the same time (different HIP streams: pipeline.SearchLanes) take different lanes."""
        q = _as_rows(q, self.d, "search: ", "Q").to(device=self.device, dtype=torch.float32).contiguous()
        Q = q.shape[0]
        D = torch.empty(Q, k, dtype=torch.float32, device=self.device)
        I = torch.empty(Q, k, dtype=torch.int64, device=self.device)
        if Q == 0:
            return D, I
        if wire_out is not None and not (wire_out.is_cuda and wire_out.dtype == torch.int64 and wire_out.is_contiguous() and tuple(wire_out.shape) == (Q, k)):
            raise ValueError("wire_out must be a contiguous int64 CUDA tensor [Q, k]")
        # the bounded search needs a workspace that stops growing at 256 queries; the six-product path (two_pass = False) a
        # [queries, rows] fp32 score matrix.  Either way the queries go through in chunks that keep it under max_workspace_bytes
        # (results do not depend on the chunking).
        flags = int(self.search_flags)
        ws_bytes = self._search_ws_bytes(flags)
        chunk = self._fit_chunk(Q, lambda n: ws_bytes(self.ntotal, self.d, n, k))
        ldx, xb = self._search_rows()
        # the library walks a call's queries in chunks of this size: 256 over the shadow (128 without) or, where its main pass runs on the GEMM
        # kernel (D >= 1024), ONE pass over the shadow per up to 1024 queries (lrx_flat_ip_bounded_chunk_queries, round 6)
        has_xb = xb is not None and self.d % 64 == 0
        lib_chunk_of = lambda n: self._lib_chunk_queries(n, k, flags, has_xb)
        lib_chunk = lib_chunk_of(min(Q, chunk))
        # More queries than one library chunk: the chunks are independent searches over the same rows, so they alternate between two
        # internal HIP streams (own workspaces), forked from and joined back into the caller's stream inside this call -- the short
        # latency-bound kernels that frame one chunk's passes overlap the other chunk's passes (Q = 1000, top-1000 over a 100 k-row
        # chunk, the reference's operating point: 2.45 -> ~2.2 ms; the stream semantics of the call do not change).  Not under graph capture.
        fork = (self.two_pass and self.chunk_lanes > 1 and Q > lib_chunk and lane == 0 and not torch.cuda.is_current_stream_capturing())
        if fork and int(ws_bytes(self.ntotal, self.d, min(chunk, lib_chunk), k)) * self.chunk_lanes > int(self.max_workspace_bytes):
            fork = False                               # one workspace per internal stream would exceed the cap: chunks one after the other
        if fork:
            chunk = min(chunk, lib_chunk)
        need = int(ws_bytes(self.ntotal, self.d, chunk, k))
        cur = torch.cuda.current_stream()
        if fork:
            if self._chunk_streams is None:
                self._chunk_streams = [torch.cuda.Stream(device=self.device) for _ in range(self.chunk_lanes)]
            # (lane 0's own workspace serves the first internal stream, lanes -1, -2, ... the others)
            lane_ws = [self._lane_workspace(-j, need, user_stream=self._chunk_streams[j]) for j in range(self.chunk_lanes)]
            ws = lane_ws[0]
            start = torch.cuda.Event()
            start.record(cur)
        else:
            ws = self._lane_workspace(lane, need)
        try:
            self._run_chunks(q, D, I, k, chunk, fork, lane_ws if fork else None, ws, start if fork else None, xb, ldx, flags, row_map, wire_out)
        finally:
            if fork:                                   # the side streams are joined back whatever happened in the loop
                for st in self._chunk_streams:
                    cur.wait_stream(st)
        if wire_out is not None and not self.two_pass:
            _lib.check(self.lib.lrx_pack_topk(_lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map), int(self.id_base), Q * k, _lib.ptr(wire_out), _lib.current_stream()))
        # (nq of the last library chunk of the last host chunk, the ntotal / mode the workspace was planned for, and the workspace itself)
        last_ws = lane_ws[((Q - 1) // chunk) % self.chunk_lanes] if fork else ws
        n_last_call = (Q - 1) % chunk + 1                                    # queries of the last library call ...
        self._last_search = ((n_last_call - 1) % lib_chunk_of(n_last_call) + 1, k, flags, xb is not None, last_ws, self.ntotal, bool(self.two_pass), ldx)   # ... and of its last chunk
        return D, I

    def _run_chunks(self, q, D, I, k, chunk, fork, lane_ws, ws, start, xb, ldx, flags, row_map, wire_out):
        Q = q.shape[0]
        for j, s in enumerate(range(0, Q, chunk)):
            qc, Dc, Ic = q[s:s + chunk], D[s:s + chunk], I[s:s + chunk]
            if fork:
                st = self._chunk_streams[j % self.chunk_lanes]
                if j < self.chunk_lanes:
                    st.wait_event(start)
                ws = lane_ws[j % self.chunk_lanes]
                stream = C.c_void_p(st.cuda_stream)
            else:
                stream = _lib.current_stream()
            self._search_chunk(qc, Dc, Ic, k, ws, stream, xb, ldx, flags, row_map, wire_out[s:s + chunk] if wire_out is not None else None)

    def last_list_counts(self) -> torch.Tensor:
        """uint32-valued int64 tensor [q]: candidate-list entries per query of the last chunk of the last two-pass search (the rows that
        passed the filter threshold and reached the refine step) -- statistics for tools and bench legs.  Zeros when the last search was
        not a two-pass search (no candidate lists exist); raises before the first search."""
        if self._last_search is None:
            raise _lib.LrxError("last_list_counts(): no search has run on this index yet")
        nq, k, flags, has_shadow, ws, ntotal, two_pass, _ = self._last_search
        out = torch.zeros(nq, dtype=torch.int32, device=self.device)
        if two_pass:                    # the workspace layout is the one planned for the ntotal of THAT search (add() / reset() since do not matter)
            _lib.check(self.lib.lrx_flat_ip_bounded_list_counts(_lib.ptr(ws), ntotal, self.d, nq, k, flags, int(has_shadow), _lib.ptr(out),
                                                                _lib.current_stream()))
        return out.to(torch.int64)

    def last_chunk_state(self, max_entries: Optional[int] = None) -> dict:
        """What the stages of the last chunk of the last two-pass search left in its workspace (lrx_flat_ip_bounded_chunk_state; read-only,
        for tests of the single stages): plan facts `emit`, `fused`, `gemm`, `ss`, `rb`, `cap`, `nsplit`, `row_grouped`, `group_rows`
        (rows per entry of the sample's maxima), `nsamp` (sample units) and `nq`, `k`, `ntotal`; per query (host tensors) `thr` (= T' - 2 eps
        as stored), `eps`, `count` (raw: an overflowing list shows more than `cap`), `flags`, `band` (sum of the parts' counts, -1 when a part
        overflowed); `any_flag` [8]; and the lists: `scores` f32 / `rows` i64 [nq, max_entries] holding the first min(count, cap,
        max_entries) entries of each list (rows = -1 beyond; max_entries defaults to cap).  Raises before the first search, after a search
        with two_pass = False or down the plain path, and -- naming the reason -- when the last search kept no lists (score-matrix filter)."""
        if self._last_search is None:
            raise _lib.LrxError("last_chunk_state(): no search has run on this index yet")
        nq, k, flags, has_shadow, ws, ntotal, two_pass, ldx = self._last_search
        if not two_pass:
            raise _lib.LrxError("last_chunk_state(): the last search was not a two-pass search (two_pass = False): no stage state")
        plan = (C.c_int32 * 12)()
        probe = torch.zeros(3 * nq + 8, dtype=torch.int32, device=self.device)
        fprobe = torch.zeros(2 * nq, dtype=torch.float32, device=self.device)
        call = lambda m, es, er: _lib.check(self.lib.lrx_flat_ip_bounded_chunk_state(
            _lib.ptr(ws), ntotal, self.d, nq, k, flags, int(has_shadow), ldx, plan, _lib.ptr(fprobe), _lib.ptr(probe), m, _lib.ptr(es), _lib.ptr(er),
            _lib.current_stream()))
        call(0, None, None)                      # the plan facts (host side) and the scalars; the lists below once their capacity is known
        emit, fused, gemm, ss, rb, cap, nsplit, row_grouped, group_rows, nsamp, plain = list(plan)[:11]
        if plain:
            raise _lib.LrxError(f"last_chunk_state(): the last search took the plain path ({ntotal} rows, d={self.d}): no stage state")
        if not emit:
            raise _lib.LrxError("last_chunk_state(): the last search kept no candidate lists (score-matrix filter: "
                                f"{ntotal} rows, search_flags={flags})")
        m = cap if max_entries is None else max(0, min(int(max_entries), cap))
        scores = torch.zeros(nq, max(m, 1), dtype=torch.float32, device=self.device)
        rows = torch.full((nq, max(m, 1)), -1, dtype=torch.int64, device=self.device)
        if m:
            call(m, scores, rows)
        ints = probe.cpu()
        thr_eps = fprobe.cpu()
        return dict(emit=bool(emit), fused=bool(fused), gemm=bool(gemm), ss=ss, rb=rb, cap=cap, nsplit=nsplit, row_grouped=bool(row_grouped),
                    group_rows=group_rows, nsamp=nsamp, nq=nq, k=k, ntotal=ntotal,
                    thr=thr_eps[:nq].clone(), eps=thr_eps[nq:].clone(), count=ints[:nq].to(torch.int64) & 0xFFFFFFFF, flags=ints[nq:2 * nq].clone(),
                    band=ints[2 * nq:3 * nq].clone(), any_flag=ints[3 * nq:3 * nq + 8].clone(), scores=scores[:, :m].cpu(), rows=rows[:, :m].cpu())


class FlatIPIndex(_TiledIPIndex):
    """One HBM-resident shard.  Memory: 4 B/element fp32 rows + 2 B/element tiled fp16 shadow + the search workspace -- per lane in use,
    for a chunk of up to 256 queries (up to 1024 where the main pass runs on the GEMM kernel: shadow, d >= 1024, more than 256 queries in the
    call): candidate lists of max(64 Ki, 64 k rounded up to a power of two) 8-byte entries per query (512 KiB per
    query up to k = 1024: 134 MB per 256-query chunk, 0.5 GB per 1024), the compact sample scores and the [128, ntotal] fp32 region of the gated fallback;
    `lrx_flat_ip_bounded_workspace_bytes` is the exact figure.  A search of MORE queries than one library chunk forks its chunks over
    `chunk_lanes` (2) internal HIP streams with one workspace each (so up to 2 x the figure above) unless that would exceed
    `max_workspace_bytes`, in which case it runs the chunks one after the other on the caller's stream.  Lanes != 0 (pipeline.SearchLanes)
    add one workspace each.  NOT thread-safe: an index keeps search state (workspaces, internal streams, the statistics of the last search);
    two host threads must not call search() on the same index at the same time (concurrent searches from ONE thread go through
    SearchLanes, one lane per search in flight)."""

    def __init__(self, d: int, capacity: int = 0, device: Optional[torch.device] = None, id_base: int = 0):
        super().__init__(d, device, id_base)
        # fp16 shadow of the rows (round-to-nearest-even, saturating): the filter pass of the two-pass search streams it instead of the fp32
        # rows (half the bytes; the exact rescoring still reads fp32).  +50 % index memory; False = no shadow.  Shadow rows and bounds are
        # written by the kernel that produces the fp32 rows (the encoder's last kernel for slots, lrx_shard_commit_rows for add()).
        # Layout: [128-row block][64-wide k-slice] tiles of 16 KiB, fragment-major inside (include/lrx.h): a wave of the filter pass loads
        # its MFMA operand with one coalesced 1-KiB request, straight into registers.  (_shadow_rows == ntotal while shadow_f16 stays on.)
        self.shadow_f16 = True
        self._set_storage(torch.empty(max(capacity, 0), d, dtype=torch.float32, device=self.device))

    @property
    def _norm_bound(self) -> torch.Tensor:
        return self._bounds[:1]

    def _wants_shadow(self) -> bool:
        return self.shadow_f16 and self.d % 64 == 0

    # -- storage -------------------------------------------------------------------------------------------------
    def reserve(self, n_rows: int):
        if n_rows > self._x.shape[0]:
            new = torch.empty(n_rows, self.d, dtype=torch.float32, device=self.device)
            if self.ntotal:
                new[:self.ntotal].copy_(self._x[:self.ntotal])
            self._set_storage(new)
        self._ensure_shadow()

    def _ensure_shadow(self):
        if not self._wants_shadow():
            return
        if self._xb is None:
            self._xb = torch.empty(0, dtype=torch.float16, device=self.device)
        # (padding rows of the last block are masked by the kernels; the copy keeps the blocks that hold shadowed rows)
        self._xb = _grow_blocks(self._xb, self._x.shape[0], self.d, self._shadow_rows)
        if self._shadow_rows < self.ntotal:
            # committed rows without a shadow (shadow_f16 switched on after rows were added, or switched off for a while and on again:
            # commits made meanwhile maintained the bounds only): build their shadow from the fp32 rows before anything streams it
            a, self._shadow_rows = self._shadow_rows, self.ntotal
            self._maintain(a, self.ntotal)

    def append_slot(self, n_rows: int) -> torch.Tensor:
        """Rows [ntotal, ntotal+n) of the shard as a writable view (the encoder writes embeddings straight into it, together with
        their shadow rows and the bounds); call commit(n) afterwards."""
        if self.ntotal + n_rows > self._x.shape[0]:
            self.reserve(_grown(self._x.shape[0], self.ntotal + n_rows))
        self._ensure_shadow()
        # whoever receives these rows may write them with anything: an earlier encoder write into them no longer vouches for
        # their shadow / bounds (commit() maintains whatever is not re-recorded by shard_sink() after this point)
        a, b = self.ntotal, self.ntotal + n_rows
        self._fused = [iv for s, e in self._fused for iv in ((s, min(e, a)), (max(s, b), e)) if iv[1] > iv[0]]
        return self._x[a:b]

    def shard_sink(self, row0: int, n_rows: int):
        """(tiled shadow tensor or None, first shadow row, bounds) for rows [row0, row0 + n) and a note that their producer maintains them."""
        self._ensure_shadow()
        if row0 + n_rows > self.ntotal:               # (rows already committed need no bookkeeping: their producer keeps them valid)
            self._fused.append((row0, row0 + n_rows))
        if not (self._wants_shadow() and self._xb is not None):
            return None, 0, self._bounds
        return self._xb, row0, self._bounds

    def _maintain(self, a: int, b: int):
        """Shadow + bounds of rows [a, b) by lrx_shard_commit_rows (one read of the fp32 rows)."""
        if b <= a:
            return
        self._ensure_shadow()
        xb = self._xb if self._wants_shadow() else None
        _lib.check(self.lib.lrx_shard_commit_rows(_lib.ptr(self._x[a:]), self._x.stride(0), b - a, self.d, _lib.ptr(xb), a, _lib.ptr(self._bounds),
                                                  _lib.current_stream()))

    def commit(self, n_rows: int):
        if n_rows > 0:
            # rows the encoder wrote through shard_sink() are done; anything else in [a, b) gets its shadow + bounds now
            for a, b in _uncovered(self._fused, self.ntotal, self.ntotal + n_rows):
                self._maintain(a, b)
        # an interval vouches for ONE commit: rows beyond b that are handed out again (append_slot) or written by something else are
        # maintained by the commit that covers them
        self._fused = []
        self.ntotal += n_rows
        if self._wants_shadow() and self._xb is not None and self._shadow_rows >= self.ntotal - n_rows:
            self._shadow_rows = self.ntotal

    def add(self, x):
        """faiss add(x f32[n,d]); accepts torch (any device) or numpy."""
        x = _as_rows(x, self.d, "add: ")
        slot = self.append_slot(x.shape[0])
        slot.copy_(x.to(dtype=torch.float32))
        self.commit(x.shape[0])

    def refresh_norm_bound(self):
        """Recompute the bounds and the fp16 shadow over all committed rows: needed only after writing into committed rows in place
        with something other than the encoder (which maintains both itself)."""
        self._bounds.zero_()
        self._maintain(0, self.ntotal)

    # -- persistence (faiss.write_index / read_index of an IndexFlatIP, see index_io.py) --------------------------
    def save(self, fname: str, chunk_rows: int = 262144, prefix: bytes = b"", append: bool = False):
        """prefix / load's offset: the record inside an enclosing one (PreTransformIndex.save); append / load's end: the record continues a
        file and is followed by more (RefineFlatIndex.save).  The same holds for every index class's save / load."""
        from .index_io import write_flat_ip
        write_flat_ip(fname, (self._x[s:min(s + chunk_rows, self.ntotal)].cpu().numpy() for s in range(0, self.ntotal, chunk_rows)),
                      self.d, self.ntotal, prefix=prefix, append=append)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, chunk_rows: int = 262144, offset: int = 0,
             end: Optional[int] = None, shadow_f16: bool = True) -> "FlatIPIndex":
        """shadow_f16=False: the shard is built without its fp16 shadow (a row store that is never streamed: RefineFlatIndex.load)."""
        from .index_io import read_flat_ip
        mm = read_flat_ip(fname, offset, end)
        idx = cls(mm.shape[1], capacity=mm.shape[0], device=device, id_base=id_base)
        idx.shadow_f16 = shadow_f16
        for s in range(0, mm.shape[0], chunk_rows):
            e = min(s + chunk_rows, mm.shape[0])
            idx._x[s:e].copy_(torch.from_numpy(np.array(mm[s:e], copy=True)), non_blocking=False)
        idx.commit(mm.shape[0])
        return idx

    @property
    def vectors(self) -> torch.Tensor:
        return self._x[:self.ntotal]

    # -- search hooks (see _TiledIPIndex) ---------------------------------------------------------------------------
    def _search_ws_bytes(self, flags: int):
        if self.two_pass:
            return lambda n, d, nq, kk: self.lib.lrx_flat_ip_bounded_workspace_bytes(n, d, nq, kk, flags)
        return self.lib.lrx_flat_ip_workspace_bytes

    def _search_rows(self):
        ldx = self._x.stride(0) if self._x.shape[0] else self.d
        if self.two_pass and self.shadow_f16:
            self._ensure_shadow()                       # (no-op unless rows were committed while the shadow was switched off)
        xb = self._xb if (self.two_pass and self._wants_shadow() and self._xb is not None and self._shadow_rows >= self.ntotal) else None
        return ldx, xb

    def _lib_chunk_queries(self, n: int, k: int, flags: int, has_xb: bool) -> int:
        return int(self.lib.lrx_flat_ip_bounded_chunk_queries(self.ntotal, self.d, n, k, flags, int(has_xb))) if self.two_pass else 128

    def _search_chunk(self, qc, Dc, Ic, k, ws, stream, xb, ldx, flags, row_map, wire):
        if self.two_pass:
            _lib.check(self.lib.lrx_flat_ip_search_bounded_wire(
                _lib.ptr(self._x), self.ntotal, ldx, self.d, _lib.ptr(xb), _lib.ptr(self._bounds), _lib.ptr(qc), qc.shape[0], k, self.id_base,
                _lib.ptr(Dc), _lib.ptr(Ic), _lib.ptr(row_map), _lib.ptr(wire) if wire is not None else None,
                _lib.ptr(ws), ws.numel(), flags, stream))
        else:
            _lib.check(self.lib.lrx_flat_ip_search(_lib.ptr(self._x), self.ntotal, ldx, self.d, _lib.ptr(self._bounds), _lib.ptr(qc), qc.shape[0], k,
                                                   self.id_base, _lib.ptr(Dc), _lib.ptr(Ic), _lib.ptr(ws), ws.numel(), stream))

    def range_search(self, q, radius: float):
        """faiss range_search for inner product -> (lims i64[Q+1], D f32[lims[Q]], I i64[lims[Q]]) device tensors: query i's hits are
        D[lims[i]:lims[i+1]], I[lims[i]:lims[i+1]] -- every row whose exact score (the value search() reports, bit-equal) is strictly greater
        than `radius`, ids = id_base + row, in ascending row order.  Exact, never truncated, deterministic (independent of the query batch,
        the shadow and two_pass).  Memory: the workspace (lrx_flat_ip_range_workspace_bytes, kept under max_workspace_bytes) plus 12 bytes
        per hit and 8 (Q + 1) for lims -- a result of n hits needs 12 n bytes; the outputs are sized by a first guess of 1024 hits per
        query and resized once if that is short.  Synchronises with the host once per call (the length of the result; once per
        library call when the workspace cap splits the queries); not under graph capture."""
        radius = _range_args("FlatIPIndex", radius)
        q = _as_rows(q, self.d, "range_search: ", "Q").to(device=self.device, dtype=torch.float32).contiguous()
        Q = q.shape[0]
        if Q == 0 or self.ntotal == 0:
            return _range_empty(self.device, Q)
        ldx, xb = self._search_rows()
        ws_bytes = lambda n: int(self.lib.lrx_flat_ip_range_workspace_bytes(self.ntotal, self.d, n, int(xb is not None)))
        chunk = self._fit_chunk(Q, ws_bytes)
        ws = self._lane_workspace(0, ws_bytes(chunk))
        stream = _lib.current_stream()

        def call(s, n, lc, Dc, Ic, cap):
            _lib.check(self.lib.lrx_flat_ip_range_search(
                _lib.ptr(self._x), self.ntotal, ldx, self.d, _lib.ptr(xb), _lib.ptr(self._bounds), _lib.ptr(q[s:s + n]), n, radius,
                self.id_base, _lib.ptr(lc), _lib.ptr(Dc), _lib.ptr(Ic), cap, _lib.ptr(ws), ws.numel(), stream))
        return _range_call(self.device, Q, chunk, call)


class SQFp16Index(_TiledIPIndex):
    """fp16 scalar-quantised inner-product shard: the faiss IndexScalarQuantizer(d, QT_fp16, METRIC_INNER_PRODUCT) surface (add / search /
    reset / ntotal / reconstruct_n / save / load), backed by lrx_sq_fp16_ip_search.  The only resident copy of the rows is their codes
    c = fp16(x) (round-to-nearest-even, saturating at +-65504 where faiss gives inf) in the tiled layout of FlatIPIndex's shadow: 2 B/element
    instead of 6.  Scores are (float) of the fp64 sum of q_i * c_i, exact top-k under that score, ties to the lower row, (-FLT_MAX, -1)
    padding -- for rows that are exactly fp16-representable, bit-identical to FlatIPIndex.  d % 64 == 0.
    Search chunking, lanes, workspaces and wire_out / row_map are the shared driver's (_TiledIPIndex; lrx_sq_fp16_ip_workspace_bytes sizes
    the workspace).  Rows enter through add() (lrx_shard_commit_rows straight from the caller's rows) or through append_slot(n) / commit(n):
    the slot is a transient fp32 staging view that LrxEncoder.encode_packed recognises (shard_of), so the encoder's last kernel writes the
    codes and the bounds itself; commit() converts whatever it did not write and releases the staging.  Staging scales with the chunk being
    added."""
    _D_ALIGN = 64

    def __init__(self, d: int, capacity: int = 0, device: Optional[torch.device] = None, id_base: int = 0):
        super().__init__(d, device, id_base)   # (_x: the staging of the open append_slot, rows ntotal ...)
        self._xb = torch.empty(0, dtype=torch.float16, device=self.device)     # the codes; R16 <= R + E from the bounds pair (include/lrx.h)
        self.reserve(capacity)

    # -- storage -------------------------------------------------------------------------------------------------
    @property
    def capacity(self) -> int:
        return self._xb.numel() // self.d

    def reserve(self, n_rows: int):
        self._xb = _grow_blocks(self._xb, n_rows, self.d, self.ntotal)

    def _set_staging(self, n_rows: int):
        self._set_storage(torch.empty(n_rows, self.d, dtype=torch.float32, device=self.device))

    def append_slot(self, n_rows: int) -> torch.Tensor:
        """A transient fp32 staging view for rows [ntotal, ntotal + n): write them (the encoder writes codes and bounds itself through
        shard_of), then commit(n)."""
        if self.ntotal + n_rows > self.capacity:
            self.reserve(_grown(self.capacity, self.ntotal + n_rows))
        if self._x.shape[0] < n_rows:
            self._set_staging(0)
            self._set_staging(n_rows)
        self._fused = []
        return self._x[:n_rows]

    def shard_sink(self, row0: int, n_rows: int):
        """(codes, first code row, bounds) for staging rows [row0, row0 + n) and a note that their producer maintains them."""
        self._fused.append((row0, row0 + n_rows))
        return self._xb, self.ntotal + row0, self._bounds

    def _commit_from(self, x: torch.Tensor, row0: int):
        if x.shape[0]:
            _lib.check(self.lib.lrx_shard_commit_rows(_lib.ptr(x), x.stride(0), x.shape[0], self.d, _lib.ptr(self._xb), row0, _lib.ptr(self._bounds),
                                                      _lib.current_stream()))

    def commit(self, n_rows: int):
        if n_rows > 0:
            if n_rows > self._x.shape[0]:
                raise ValueError(f"commit({n_rows}): only {self._x.shape[0]} staged rows")
            for a, b in _uncovered(self._fused, 0, n_rows):
                self._commit_from(self._x[a:b], self.ntotal + a)
        self._fused = []
        self.ntotal += n_rows
        self._shadow_rows = self.ntotal
        self._set_staging(0)                           # staging released (stream-ordered by the allocator)

    def add(self, x):
        """faiss add(x f32[n,d]): the codes are written straight from the rows (one device copy when x is not already fp32 on this device)."""
        x = _as_rows(x, self.d, "add: ")
        n = x.shape[0]
        if self.ntotal + n > self.capacity:
            self.reserve(_grown(self.capacity, self.ntotal + n))
        x = x.to(device=self.device, dtype=torch.float32)
        if x.stride(1) != 1 or (n > 1 and x.stride(0) % 4):
            x = x.contiguous()
        self._commit_from(x, self.ntotal)
        self.ntotal += n
        self._shadow_rows = self.ntotal

    def reset(self):
        super().reset()
        self._set_staging(0)

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """Rows [i0, i0 + n) decoded exactly to fp32 (device tensor [n, d])."""
        _check_range(i0, n, self.ntotal)
        out = torch.empty(n, self.d, dtype=torch.float32, device=self.device)
        if n:
            _lib.check(self.lib.lrx_sq_fp16_decode_rows(_lib.ptr(self._xb), i0, n, self.d, _lib.ptr(out), self.d, _lib.current_stream()))
        return out

    @property
    def vectors(self) -> torch.Tensor:
        return self.reconstruct_n(0, self.ntotal)

    def codes(self) -> torch.Tensor:
        """The codes as a row-major [ntotal, d] fp16 tensor (a copy: the stored layout is tiled)."""
        return self.shadow_rows()

    # -- persistence (faiss.write_index / read_index of an IndexScalarQuantizer(QT_fp16), see index_io.py) -----------
    def save(self, fname: str, chunk_rows: int = 262144, prefix: bytes = b"", append: bool = False):
        from .index_io import write_sq_fp16
        write_sq_fp16(fname, (self.reconstruct_n(s, min(chunk_rows, self.ntotal - s)).half().cpu().numpy() for s in range(0, self.ntotal, chunk_rows)),
                      self.d, self.ntotal, prefix=prefix, append=append)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, chunk_rows: int = 262144, offset: int = 0,
             end: Optional[int] = None) -> "SQFp16Index":
        from .index_io import read_sq_fp16
        mm = read_sq_fp16(fname, offset, end)
        idx = cls(mm.shape[1], capacity=mm.shape[0], device=device, id_base=id_base)
        for s in range(0, mm.shape[0], chunk_rows):
            e = min(s + chunk_rows, mm.shape[0])
            idx.add(torch.from_numpy(np.array(mm[s:e], copy=True)).to(idx.device).float())   # fp16 -> fp32 -> fp16: exact
        return idx

    # -- search hooks (see _TiledIPIndex): the codes are the rows -----------------------------------------------------
    def _search_ws_bytes(self, flags: int):
        return lambda n, d, nq, kk: self.lib.lrx_sq_fp16_ip_workspace_bytes(n, d, nq, kk, flags)

    def _search_rows(self):
        return self.d, self._xb

    def _lib_chunk_queries(self, n: int, k: int, flags: int, has_xb: bool) -> int:
        return int(self.lib.lrx_sq_fp16_ip_chunk_queries(self.ntotal, self.d, n, k, flags))

    def _search_chunk(self, qc, Dc, Ic, k, ws, stream, xb, ldx, flags, row_map, wire):
        _lib.check(self.lib.lrx_sq_fp16_ip_search(
            _lib.ptr(self._xb), self.ntotal, self.d, _lib.ptr(self._bounds), _lib.ptr(qc), qc.shape[0], k, self.id_base, _lib.ptr(Dc), _lib.ptr(Ic),
            _lib.ptr(row_map), _lib.ptr(wire) if wire is not None else None, _lib.ptr(ws), ws.numel(), flags, stream))

    def range_search(self, q, radius: float):
        """faiss range_search -> (lims i64[Q+1], D f32[lims[Q]], I i64[lims[Q]]) device tensors, the rules of FlatIPIndex.range_search: every
        row whose score -- the value search() reports, bit-equal: (float) of the fp64 sum of q_i * float(code_i) -- is strictly greater than
        `radius`, ids = id_base + row in ascending row order; exact, never truncated, independent of the query batch, the path inside the
        library and max_workspace_bytes.  One filter pass over the codes + exact rescoring from the codes (lrx_sq_fp16_ip_range_search).
        Synchronises with the host once per library call; not under graph capture."""
        radius = _range_args("SQFp16Index", radius)
        q = _as_rows(q, self.d, "range_search: ", "Q").to(device=self.device, dtype=torch.float32).contiguous()
        Q = q.shape[0]
        if Q == 0 or self.ntotal == 0:
            return _range_empty(self.device, Q)
        ws_bytes = lambda n: int(self.lib.lrx_sq_fp16_ip_range_workspace_bytes(self.ntotal, self.d, n))
        chunk = self._fit_chunk(Q, ws_bytes)
        ws = self._lane_workspace(0, ws_bytes(chunk))
        stream = _lib.current_stream()

        def call(s, n, lc, Dc, Ic, cap):
            _lib.check(self.lib.lrx_sq_fp16_ip_range_search(
                _lib.ptr(self._xb), self.ntotal, self.d, _lib.ptr(self._bounds), _lib.ptr(q[s:s + n]), n, radius, self.id_base, _lib.ptr(lc),
                _lib.ptr(Dc), _lib.ptr(Ic), cap, _lib.ptr(ws), ws.numel(), stream))
        return _range_call(self.device, Q, chunk, call)


class _CodeIndex:
    """What PQIndex, SQ8Index and BinaryFlatIndex share: `code_size` bytes of codes per row (faiss's name), stored as whole 128-row blocks of
    `_width` bytes per row in `_codes` (the layouts of include/lrx.h); reserve / capacity and the grow policy; the transient fp32 staging view
    of append_slot(n) / commit(n) -- commit() trains an untrained index on the staged rows, add()s them and releases the staging; reset()
    (drops the rows, keeps the training); the search prologue and the search workspace `_ws`.  A subclass checks its arguments BEFORE it
    calls this constructor (no GPU is needed to refuse them) and keeps what is its own: training, _encode_into (or add), the decode call of
    reconstruct_n, the layout permutation (_layout), persistence and the library calls of search.
    The codes an index holds, and what it returns, are a function of its training and of the committed rows in arrival order, and of nothing
    else that happened to it: reset() leaves old codes in the last block, and every kernel is handed ntotal, never the capacity."""
    MAX_K = 2048
    is_trained = True          # (faiss: an index that needs no training is trained; PQIndex / SQ8Index start untrained)
    _capture_ws_error = None   # SQ8Index: the message that refuses to allocate the search workspace under HIP-graph capture

    def __init__(self, d: int, code_size: int, width: int, capacity: int, device: Optional[torch.device], id_base: int):
        _lib.require_gpu()
        self.lib = _lib.lib()
        self.d, self.code_size, self._width = d, code_size, width
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.id_base = id_base
        self.ntotal = 0
        self._codes = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._stage = None
        self._ws = None
        self.reserve(capacity)

    # -- storage -------------------------------------------------------------------------------------------------
    @property
    def capacity(self) -> int:
        return self._codes.numel() // self._width

    def reserve(self, n_rows: int):
        self._codes = _grow_blocks(self._codes, n_rows, self._width, self.ntotal, zero=True)

    def _make_room(self, n: int):
        if self.ntotal + n > self.capacity:
            self.reserve(_grown(self.capacity, self.ntotal + n))

    def _rows(self, x) -> torch.Tensor:
        x = _as_rows(x, self.d).to(device=self.device, dtype=torch.float32)
        return x.contiguous() if x.stride(1) != 1 else x

    def _scratch_blocks(self, n: int) -> torch.Tensor:
        return torch.zeros(-(-n // 128) * 128 * self._width, dtype=torch.uint8, device=self.device)

    def blocked_to_rows(self, blocked: torch.Tensor, n: int) -> torch.Tensor:
        """Codes in the stored layout (include/lrx.h) -> row-major uint8 [n, code_size]."""
        shape, perm = self._layout()
        nb = -(-n // 128)
        return blocked[:nb * 128 * self._width].view(nb, *shape).permute(0, *perm).reshape(nb * 128, self._width)[:n, :self.code_size]

    def rows_to_blocked(self, codes: torch.Tensor) -> torch.Tensor:
        shape, perm = self._layout()
        n = codes.shape[0]
        nb = -(-n // 128)
        buf = torch.zeros(nb * 128, self._width, dtype=torch.uint8, device=self.device)
        buf[:n, :self.code_size] = codes.to(self.device)
        back = [perm.index(a) + 1 for a in range(1, len(perm) + 1)]                       # the inverse permutation
        return buf.view(nb, *(shape[p - 1] for p in perm)).permute(0, *back).contiguous().view(-1)

    # -- rows ------------------------------------------------------------------------------------------------------
    def add(self, x):
        """faiss add(x f32[n, d]): encode into the codes (raises before train(), as faiss does)."""
        if not self.is_trained:
            raise RuntimeError(f"{type(self).__name__}.add: the index is not trained (call train() first)")
        x = self._rows(x)
        n = x.shape[0]
        self._make_room(n)
        if n:
            self._encode_into(x, self._codes, self.ntotal)
        self.ntotal += n

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
        self.ntotal = 0
        self._stage = None

    def codes(self) -> torch.Tensor:
        """The codes as a row-major uint8 [ntotal, code_size] tensor (a copy: the stored layout is blocked)."""
        return self.blocked_to_rows(self._codes, self.ntotal).contiguous()

    @property
    def vectors(self) -> torch.Tensor:
        return self.reconstruct_n(0, self.ntotal)

    # -- search --------------------------------------------------------------------------------------------------
    def _begin_search(self, q, k: int, row_map: Optional[torch.Tensor], d_dtype=torch.float32, k_error: Optional[str] = None):
        """The checks every search starts with (k_error: the subclass's own complaint about k; otherwise 1 <= k <= MAX_K) -> (q fp32 [Q, d] on
        the device, D [Q, k] of d_dtype, I int64 [Q, k]); with no queries the caller returns (D, I) as they are."""
        q = _as_rows(q, self.d, "search: ", "Q").to(device=self.device, dtype=torch.float32).contiguous()
        if k_error is None and not 1 <= k <= self.MAX_K:
            k_error = f"search: k={k} out of range (1..{self.MAX_K})"
        if k_error is not None:
            raise ValueError(k_error)
        if row_map is not None and not (row_map.is_cuda and row_map.dtype == torch.int64 and row_map.is_contiguous() and row_map.numel() >= self.ntotal):
            raise ValueError("row_map must be a contiguous int64 CUDA tensor of >= ntotal entries")
        D = torch.empty(q.shape[0], k, dtype=d_dtype, device=self.device)
        I = torch.empty(q.shape[0], k, dtype=torch.int64, device=self.device)
        return q, D, I

    def _search_workspace(self, need: int) -> torch.Tensor:
        return _workspace(vars(self), "_ws", int(need), self.device, self._capture_ws_error)


class PQIndex(_CodeIndex):
    """Product-quantised inner-product shard: the faiss IndexPQ(d, M, nbits=8, METRIC_INNER_PRODUCT) surface (train / is_trained / add /
    search / reset / ntotal / reconstruct_n / save / load), backed by lrx_pq_ip_search.  Resident: M bytes per row (the codes, in the
    blocked layout of include/lrx.h) + the centroids [M, 256, d / M] fp32.  Scores are the fp32 sums of the query's lookup table over the
    row's codes in ascending m; exact top-k under that score with the flat index's tie and padding rules.
    Training: Lloyd k-means per sub-space (256 centroids, 25 iterations, at most 256 x 256 sampled rows, fixed seed), assignments by the
    encoding kernel, deterministic fp64 centroid sums (sorted by code, segmented sums), faiss's split of empty clusters.  The same input
    and seed give the same centroids; they are not faiss's (its RNG differs).
    Rows enter through add() or through append_slot(n) / commit(n): the slot is a transient fp32 staging view; commit() trains the index
    if it is untrained, encodes the rows and releases the staging.  Search: one library call (it walks the queries in chunks that keep
    the score matrix under 1 GiB), workspace kept by the index.  NOT thread-safe."""

    KSUB = 256
    NITER = 25
    MAX_POINTS_PER_CENTROID = 256
    SEED = 1234

    def __init__(self, d: int, M: int = 96, nbits: int = 8, capacity: int = 0, device: Optional[torch.device] = None, id_base: int = 0):
        if nbits != 8:
            raise NotImplementedError(f"PQIndex: nbits={nbits} is not served (only 8)")
        if M <= 0 or d % M != 0:
            raise ValueError(f"PQIndex: d={d} is not a multiple of M={M}")
        if d // M > 64:
            raise NotImplementedError(f"PQIndex: sub-space dimension d / M = {d // M} > 64 is not served")
        self.M, self.nbits, self.dsub = M, nbits, d // M
        self.Mp = -(-M // 16) * 16
        super().__init__(d, M, self.Mp, capacity, device, id_base)
        self.is_trained = False
        self.centroids = torch.zeros(M, self.KSUB, self.dsub, dtype=torch.float32, device=self.device)

    def _layout(self):
        return (self.Mp // 16, 128, 16), (2, 1, 3)       # a block: [16-sub-space group][row][byte] -> [row][group][byte]

    def _encode_into(self, x: torch.Tensor, codes: torch.Tensor, row0: int, centroids: Optional[torch.Tensor] = None):
        centroids = self.centroids if centroids is None else centroids
        for s in range(0, x.shape[0], 262144):
            xs = x[s:s + 262144]
            _lib.check(self.lib.lrx_pq_encode(_lib.ptr(xs), xs.shape[0], xs.stride(0), _lib.ptr(centroids), self.d, self.M, _lib.ptr(codes),
                                              row0 + s, _lib.current_stream()))

    def encode(self, x, centroids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """faiss sa_encode: row-major uint8 [n, M] codes of x under `centroids` (default: this index's)."""
        x = self._rows(x)
        c = (self.centroids if centroids is None else centroids).to(self.device, torch.float32).contiguous()
        blocked = self._scratch_blocks(x.shape[0])
        if x.shape[0]:
            self._encode_into(x, blocked, 0, c)
        return self.blocked_to_rows(blocked, x.shape[0])

    # -- training ------------------------------------------------------------------------------------------------
    def sample_rows(self, n: int, seed: Optional[int] = None):
        """(rng, rows): the first draw of train() over n rows -- the sorted numbers of the at most 256 x 256 rows it trains on (None: all of
        them) -- and the generator that made it, for a caller that derives the training rows from that draw (IVFPQIndex: their residuals)
        and hands both to train(sample, rng=rng)."""
        rng = np.random.default_rng(self.SEED if seed is None else seed)
        max_pts = self.KSUB * self.MAX_POINTS_PER_CENTROID
        return rng, (np.sort(rng.permutation(n)[:max_pts]) if n > max_pts else None)

    def train(self, x, niter: Optional[int] = None, seed: Optional[int] = None, rng=None):
        """Lloyd k-means per sub-space (see the class note).  niter=0 leaves the initial centroids (distinct sampled rows).
        rng: x is already the sample of sample_rows(), whose generator this is."""
        x = self._rows(x)
        n = x.shape[0]
        if n < self.KSUB:
            raise ValueError(f"PQIndex.train: {n} training rows < {self.KSUB} centroids")
        niter = self.NITER if niter is None else niter
        if rng is None:
            rng, rows = self.sample_rows(n, seed)
            if rows is not None:
                x = x[torch.from_numpy(rows).to(self.device)]
                n = rows.shape[0]
        M, K, ds = self.M, self.KSUB, self.dsub
        xs = x.view(n, M, ds)
        init = np.stack([rng.permutation(n)[:K] for _ in range(M)])                       # [M, K] distinct rows per sub-space
        cent = xs[torch.from_numpy(init).to(self.device), torch.arange(M, device=self.device)[:, None]].contiguous()   # [M, K, ds]
        x_t = xs.permute(1, 0, 2).double()                                                 # [M, n, ds]
        blocked = self._scratch_blocks(n)
        for _ in range(niter):
            self._encode_into(x, blocked, 0, cent)
            codes = self.blocked_to_rows(blocked, n).t().long()                            # [M, n]
            cent = _pq_update(x_t, codes, K, cent, rng)
        self.centroids = cent.float().contiguous()
        self.is_trained = True

    # -- rows ------------------------------------------------------------------------------------------------------
    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """Rows [i0, i0 + n) decoded (centroid of each code) to fp32, device tensor [n, d]."""
        _check_range(i0, n, self.ntotal)
        out = torch.empty(n, self.d, dtype=torch.float32, device=self.device)
        if n:
            _lib.check(self.lib.lrx_pq_decode_rows(_lib.ptr(self._codes), i0, n, _lib.ptr(self.centroids), self.d, self.M, _lib.ptr(out), self.d,
                                                   _lib.current_stream()))
        return out

    def set_contents(self, centroids, codes):
        """Replace the centroids ([M, 256, d / M]) and the rows (row-major uint8 [n, M] codes): load() and tests."""
        c = torch.as_tensor(centroids).to(self.device, torch.float32).reshape(self.M, self.KSUB, self.dsub).contiguous()
        codes = torch.as_tensor(codes)
        if codes.ndim != 2 or codes.shape[1] != self.M or codes.dtype != torch.uint8:
            raise ValueError(f"set_contents: codes must be uint8 [n, {self.M}]")
        self.centroids = c
        self.is_trained = True
        self._codes = self.rows_to_blocked(codes)
        self.ntotal = codes.shape[0]

    # -- persistence (faiss.write_index / read_index of an IndexPQ, see index_io.py) ----------------------------------------
    def save(self, fname: str, chunk_rows: int = 1 << 20, prefix: bytes = b"", append: bool = False):
        from .index_io import write_pq
        write_pq(fname, self.centroids.cpu().numpy(), (self.blocked_to_rows(self._codes[s // 128 * 128 * self.Mp:], min(chunk_rows, self.ntotal - s)).cpu().numpy()
                                                       for s in range(0, self.ntotal, chunk_rows)), self.d, self.M, self.ntotal, self.is_trained, prefix=prefix,
                 append=append)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, offset: int = 0, end: Optional[int] = None) -> "PQIndex":
        from .index_io import read_pq
        cent, codes, trained = read_pq(fname, offset, end)
        M, _, dsub = cent.shape
        idx = cls(M * dsub, M, device=device, id_base=id_base)
        idx.set_contents(torch.from_numpy(cent), torch.from_numpy(np.array(codes, copy=True)))
        idx.is_trained = trained
        return idx

    # -- search --------------------------------------------------------------------------------------------------
    def search(self, q, k: int, row_map: Optional[torch.Tensor] = None):
        """faiss search -> (D f32[Q,k], I i64[Q,k]) device tensors: score descending, ties to the lower row, (-FLT_MAX, -1) padding when
        k > ntotal.  I = id_base + row, or row_map[row] (int64 CUDA tensor of >= ntotal entries) when given."""
        q, D, I = self._begin_search(q, k, row_map)
        Q = q.shape[0]
        if Q == 0:
            return D, I
        ws = self._search_workspace(self.lib.lrx_pq_ip_workspace_bytes(self.ntotal, self.d, self.M, Q, k))
        _lib.check(self.lib.lrx_pq_ip_search(_lib.ptr(self._codes), self.ntotal, _lib.ptr(self.centroids), self.d, self.M, _lib.ptr(q), Q, k,
                                             int(self.id_base), _lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(), 0,
                                             _lib.current_stream()))
        return D, I

    range_row_chunk = 0   # lrx_pq_ip_range_search's row_chunk: 0 = the library's 4 Mi; tests set a multiple of 128 (the result does not depend on it)

    def range_search(self, q, radius: float):
        """faiss range_search -> (lims i64[Q+1], D f32[lims[Q]], I i64[lims[Q]]) device tensors, the rules of FlatIPIndex.range_search: every
        row whose score -- the fp32 table sum search() reports, bit-equal -- is strictly greater than `radius`, ids = id_base + row in
        ascending row order; exact, never truncated, independent of the query batch and the row chunking.  Two sweeps of the scan
        (lrx_pq_ip_range_search): measured at 2.0x search(q, 100) for 100 queries over 1M x 1536; a result past the
        first guess of 1024 hits per query runs the library a second time.  Synchronises with the host once per call; not under graph capture."""
        radius = _range_args("PQIndex", radius)
        q = _as_rows(q, self.d, "range_search: ", "Q").to(device=self.device, dtype=torch.float32).contiguous()
        Q = q.shape[0]
        if Q == 0 or self.ntotal == 0:
            return _range_empty(self.device, Q)
        if not self.is_trained:
            raise RuntimeError("PQIndex.range_search: the index is not trained")
        rc = int(self.range_row_chunk)
        ws = self._search_workspace(self.lib.lrx_pq_ip_range_workspace_bytes(self.ntotal, self.d, self.M, Q, rc))
        stream = _lib.current_stream()

        def call(s, n, lc, Dc, Ic, cap):
            _lib.check(self.lib.lrx_pq_ip_range_search(_lib.ptr(self._codes), self.ntotal, _lib.ptr(self.centroids), self.d, self.M, _lib.ptr(q), n, radius,
                                                       int(self.id_base), _lib.ptr(lc), _lib.ptr(Dc), _lib.ptr(Ic), cap, _lib.ptr(ws), ws.numel(), stream, rc))
        return _range_call(self.device, Q, Q, call)


class SQ8Index(_CodeIndex):
    """8-bit scalar-quantised inner-product shard: the faiss IndexScalarQuantizer(d, QT_8bit | QT_8bit_uniform, METRIC_INNER_PRODUCT)
    surface (train / is_trained / add / search / reset / ntotal / reconstruct_n / save / load), backed by lrx_sq8_ip_search.  Resident:
    ntotal * d bytes of codes (whole 128-row blocks, the tiled layout of include/lrx.h) + `trained` (vmin ++ vdiff: 8 d bytes for QT_8bit,
    8 for QT_8bit_uniform).  Training is a per-dimension (or global) min / max: no RNG, so codes and files can equal a faiss-written index
    byte for byte.  A score is the (float) of the fp64 sum of q_i * y_i over the decoded row y; top-k is exact under that score with the
    flat index's tie and padding rules: the i8-MFMA scan is a filter with a rigorous per-query bound, the rows inside the
    band are rescored from the codes.  d % 64 == 0.
    train() may be called on several pieces (train(x, more=True) folds a further piece into the range of the earlier ones).  Rows enter
    through add() or through append_slot(n) / commit(n): the slot is a transient fp32 staging view; commit() trains the index on the
    staged rows if it is untrained, encodes them and releases the staging.  Search: one library call (it walks the queries in chunks of
    <= 128), workspace kept by the index; under a HIP-graph capture the workspace must already exist.  NOT thread-safe."""

    QTYPES = {"QT_8bit": 0, "QT_8bit_uniform": 2}     # faiss ScalarQuantizer::QuantizerType
    _capture_ws_error = ("SQ8Index.search under graph capture: the search workspace must exist before the capture starts -- run one eager "
                         "search with the same number of queries and k first")

    def __init__(self, d: int, qtype: str = "QT_8bit", capacity: int = 0, device: Optional[torch.device] = None, id_base: int = 0):
        if qtype not in self.QTYPES:
            raise NotImplementedError(f"SQ8Index: qtype={qtype!r} is not served (only {sorted(self.QTYPES)})")
        if d <= 0 or d % 64 != 0:
            raise ValueError(f"SQ8Index: d={d} must be a multiple of 64")
        super().__init__(d, d, d, capacity, device, id_base)
        self.qtype, self._qt = qtype, self.QTYPES[qtype]
        self.uniform = self._qt == 2
        self.is_trained = False
        self.trained = torch.zeros(2 if self.uniform else 2 * d, dtype=torch.float32, device=self.device)
        self._minmax = None                            # [2, d] running column min / max of the training pieces
        self._last_search = None                       # (Q, k, ntotal, workspace) of the last search: last_chunk_state()

    def _layout(self):
        # a block: [64-column slice][16-row group][16-column piece][row][byte] -> [row group][row][slice][piece][byte]
        return (self.d // 64, 8, 4, 16, 16), (2, 4, 1, 3, 5)

    # -- training ------------------------------------------------------------------------------------------------
    def train(self, x, more: bool = False):
        """Range statistic RS_minmax: vmin / vdiff per dimension (QT_8bit) or over all elements (QT_8bit_uniform); NaN values are ignored
        (a range with no other value gets vmin = vdiff = 0).
        more=True folds x into the range of the earlier train() calls (training on a large input in pieces)."""
        x = self._rows(x)
        if x.shape[0] < 1:
            raise ValueError("SQ8Index.train: 0 training rows")
        if self._minmax is None or not more:
            self._minmax = torch.empty(2, self.d, dtype=torch.float32, device=self.device)
            self._minmax[0].fill_(float("inf"))
            self._minmax[1].fill_(float("-inf"))
        for s in range(0, x.shape[0], 1 << 22):
            xs = x[s:s + (1 << 22)]
            _lib.check(self.lib.lrx_sq8_train_minmax(_lib.ptr(xs), xs.shape[0], xs.stride(0), self.d, _lib.ptr(self._minmax), _lib.current_stream()))
        mn, mx = self._minmax[0], self._minmax[1]
        if self.uniform:
            mn, mx = mn.min().reshape(1), mx.max().reshape(1)
        empty = mn > mx                                # no value that is not NaN: vmin = vdiff = 0 (every code 0, decoded 0)
        mn, mx = mn.masked_fill(empty, 0.0), mx.masked_fill(empty, 0.0)
        self.trained = torch.cat([mn, mx - mn])        # (fp32 subtraction: the contract's vdiff)
        self.is_trained = True

    def _encode_into(self, x: torch.Tensor, codes: torch.Tensor, row0: int):
        for s in range(0, x.shape[0], 262144):
            xs = x[s:s + 262144]
            _lib.check(self.lib.lrx_sq8_encode(_lib.ptr(xs), xs.shape[0], xs.stride(0), _lib.ptr(self.trained), self.d, self._qt, _lib.ptr(codes), row0 + s,
                                               _lib.current_stream()))

    def encode(self, x) -> torch.Tensor:
        """faiss sa_encode: row-major uint8 [n, d] codes of x under this index's training."""
        x = self._rows(x)
        blocked = self._scratch_blocks(x.shape[0])
        if x.shape[0]:
            self._encode_into(x, blocked, 0)
        return self.blocked_to_rows(blocked, x.shape[0]).contiguous()

    # -- rows ------------------------------------------------------------------------------------------------------
    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """Rows [i0, i0 + n) decoded to fp32 (the rows the scores are defined over), device tensor [n, d]."""
        _check_range(i0, n, self.ntotal)
        out = torch.empty(n, self.d, dtype=torch.float32, device=self.device)
        for s in range(0, n, 1 << 20):
            m = min(1 << 20, n - s)
            _lib.check(self.lib.lrx_sq8_decode_rows(_lib.ptr(self._codes), i0 + s, m, _lib.ptr(self.trained), self.d, self._qt, _lib.ptr(out[s:]), self.d,
                                                    _lib.current_stream()))
        return out

    def set_contents(self, trained, codes):
        """Replace the training (vmin ++ vdiff) and the rows (row-major uint8 [n, d] codes): load() and tests."""
        t = torch.as_tensor(trained).to(self.device, torch.float32).reshape(-1).contiguous()
        codes = torch.as_tensor(codes)
        if t.numel() != self.trained.numel():
            raise ValueError(f"set_contents: trained must hold {self.trained.numel()} floats for {self.qtype}")
        if codes.ndim != 2 or codes.shape[1] != self.d or codes.dtype != torch.uint8:
            raise ValueError(f"set_contents: codes must be uint8 [n, {self.d}]")
        self.trained = t
        self.is_trained = True
        self._minmax = None
        self._codes = None
        self._codes = self.rows_to_blocked(codes)
        self.ntotal = codes.shape[0]

    # -- persistence (faiss.write_index / read_index of an IndexScalarQuantizer(QT_8bit[_uniform]), see index_io.py) ----------
    def save(self, fname: str, chunk_rows: int = 1 << 18, prefix: bytes = b"", append: bool = False):
        from .index_io import write_sq8
        write_sq8(fname, self.trained.cpu().numpy(), (self.blocked_to_rows(self._codes[s // 128 * 128 * self.d:], min(chunk_rows, self.ntotal - s)).cpu().numpy()
                                                      for s in range(0, self.ntotal, chunk_rows)), self.d, self.ntotal, self._qt, self.is_trained, prefix=prefix,
                  append=append)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, chunk_rows: int = 1 << 18, offset: int = 0,
             end: Optional[int] = None) -> "SQ8Index":
        from .index_io import read_sq8
        qt, trained, codes, is_trained = read_sq8(fname, offset, end)
        n, d = codes.shape
        idx = cls(d, {v: k for k, v in cls.QTYPES.items()}[qt], capacity=n, device=device, id_base=id_base)
        idx.trained = torch.from_numpy(trained).to(idx.device)
        for s in range(0, n, chunk_rows):              # (chunk_rows is a multiple of 128: whole blocks)
            e = min(s + chunk_rows, n)
            blk = idx.rows_to_blocked(torch.from_numpy(np.array(codes[s:e], copy=True)))
            idx._codes[s * d:s * d + blk.numel()].copy_(blk)
        idx.ntotal = n
        idx.is_trained = is_trained
        return idx

    # -- search --------------------------------------------------------------------------------------------------
    def search(self, q, k: int, row_map: Optional[torch.Tensor] = None):
        """faiss search -> (D f32[Q,k], I i64[Q,k]) device tensors: score descending, ties to the lower row, (-FLT_MAX, -1) padding when
        k > ntotal.  I = id_base + row, or row_map[row] (int64 CUDA tensor of >= ntotal entries) when given."""
        q, D, I = self._begin_search(q, k, row_map)
        Q = q.shape[0]
        if Q == 0:
            return D, I
        ws = self._search_workspace(self.lib.lrx_sq8_ip_workspace_bytes(self.ntotal, self.d, Q, k))
        _lib.check(self.lib.lrx_sq8_ip_search(_lib.ptr(self._codes), self.ntotal, _lib.ptr(self.trained), self.d, self._qt, _lib.ptr(q), Q, k,
                                              int(self.id_base), _lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(), 0,
                                              _lib.current_stream()))
        self._last_search = (Q, k, self.ntotal, ws)
        return D, I

    def _layout_of(self, ntotal: int, Q: int, k: int) -> dict:
        out = (C.c_int64 * 12)()
        _lib.check(self.lib.lrx_sq8_ip_workspace_layout(ntotal, self.d, Q, k, out))
        return dict(zip(("qc", "rc", "ld", "nblk_ld", "qpad", "digits_off", "scale_off", "bias_off", "eps_off", "scores_off", "blkmax_off", "total"),
                        (int(v) for v in out)))

    def last_chunk_state(self) -> dict:
        """What the stages of the last search left in its workspace for its LAST query chunk and LAST row chunk (lrx_sq8_ip_workspace_layout;
        read-only, for tests of the single stages), as host tensors: `q0`, `nq` (the chunk's queries [q0, q0 + nq) of the call), `qpad` (the
        queries k_sq8_prep wrote digits for: nq padded to 16 x (1, 2, 4, 8) tiles), `row0`, `rows` (the row chunk), `k`, `ntotal`, `layout`;
        `hi`, `lo` int8 [qpad, d] (the digit planes un-tiled, padding queries included) and `n` int32 [nq, d] = 128 hi + lo; `scale`, `bias`
        fp64 [nq]; `eps` fp32 [nq]; `scores` fp32 [nq, ld] (filter scores; columns >= rows are whatever the scan made of the codes there) and
        `blkmax` fp32 [nq, ceil(rows / 128)].  Raises before the first search."""
        if self._last_search is None:
            raise _lib.LrxError("last_chunk_state(): no search has run on this index yet")
        Q, k, ntotal, ws = self._last_search
        L = self._layout_of(ntotal, Q, k)
        qc, rc, ld, nblk_ld = L["qc"], L["rc"], L["ld"], L["nblk_ld"]
        q0 = (Q - 1) // qc * qc
        nq = Q - q0
        qpad = self._layout_of(ntotal, nq, k)["qpad"]                     # the tiles k_sq8_prep prepares for a chunk of nq queries
        row0 = (max(ntotal, 1) - 1) // rc * rc
        rows = ntotal - row0
        KC = self.d // 64
        region = lambda off, count, dtype, size: ws[off:off + count * size].view(dtype)
        tiles = region(L["digits_off"], qpad * self.d * 2, torch.int8, 1).view(qpad // 16, KC, 2, 4, 16, 16)
        planes = tiles.permute(2, 0, 4, 1, 3, 5).reshape(2, qpad, self.d).cpu()  # [plane][query tile, query][slice, piece, byte]
        hi, lo = planes[0].contiguous(), planes[1].contiguous()
        nblk = -(-rows // 128)
        return dict(q0=q0, nq=nq, qpad=qpad, row0=row0, rows=rows, k=k, ntotal=ntotal, layout=L, hi=hi, lo=lo,
                    n=(128 * hi[:nq].to(torch.int32) + lo[:nq].to(torch.int32)),
                    scale=region(L["scale_off"], nq, torch.float64, 8).cpu(), bias=region(L["bias_off"], nq, torch.float64, 8).cpu(),
                    eps=region(L["eps_off"], nq, torch.float32, 4).cpu(),
                    scores=region(L["scores_off"], nq * ld, torch.float32, 4).view(nq, ld).cpu(),
                    blkmax=region(L["blkmax_off"], nq * nblk_ld, torch.float32, 4).view(nq, nblk_ld)[:, :nblk].cpu())

    def range_search(self, q, radius: float):
        raise NotImplementedError("SQ8Index.range_search is not served yet (a follow-up: the scan's matrix holds filter scores, so the range "
                                  "search needs the band rescoring from the codes on top of the scan driver's range sweeps)")


class BinaryFlatIndex(_CodeIndex):
    """Binary flat shard: the faiss IndexBinaryFlat(d) surface (add / search / reset / ntotal / reconstruct_n / save / load) plus the reference's
    float rerank (FaissBinaryIndex.search), backed by lrx_binary_ip_search / lrx_binary_hamming_search.  Resident: d / 8 bytes per row (d = the
    number of bits, d % 8 == 0), in the blocked layout of include/lrx.h (rows padded to whole 16-byte groups).  Bit j of a row is
    x[j] > threshold[j] (strict, NaN -> 0), bytes in np.packbits order.  search(): the Hamming top-binary_k (ascending distance, ties to the lower
    row) rescored with the float query against the +-1 rows -- (float) of the fp64 sum -- and the top-k of those by score descending, ties to the
    lower row, (-FLT_MAX, -1) padding; rerank=False returns the int32 Hamming lists, padded with (2^31 - 1, -1).
    Rows enter through add() -- floating rows, binarised with the index's threshold, or uint8 [n, d / 8] rows that are already packed -- or
    through append_slot(n) / commit(n): the slot is a transient fp32 staging view, commit() binarises it and releases it.  Search: one library
    call, workspace kept by the index.  NOT thread-safe."""

    def __init__(self, d: int, capacity: int = 0, device: Optional[torch.device] = None, id_base: int = 0, threshold=0):
        if d <= 0 or d % 8 != 0:
            raise ValueError(f"BinaryFlatIndex: d={d} (bits) must be a positive multiple of 8")
        if d > 16384:
            raise NotImplementedError(f"BinaryFlatIndex: d={d} > 16384 bits is not served")
        self.Mp = -(-d // 128) * 16            # bytes per row in the blocked layout
        super().__init__(d, d // 8, self.Mp, capacity, device, id_base)
        self.threshold = threshold

    def _threshold_args(self, threshold):
        """threshold (a number, or d values) -> (the scalar, the [d] fp32 device vector or None)."""
        if isinstance(threshold, (int, float)):
            return float(threshold), None
        t = torch.as_tensor(threshold)
        if t.numel() == 1:
            return float(t.reshape(()).item()), None
        if t.numel() != self.d:
            raise ValueError(f"threshold must be a scalar or hold d={self.d} values, got {tuple(t.shape)}")
        return 0.0, t.reshape(self.d).to(device=self.device, dtype=torch.float32).contiguous()

    def _pack_into(self, x: torch.Tensor, row0: int):
        thr, tv = self._threshold_args(self.threshold)
        _lib.check(self.lib.lrx_binary_pack_rows(_lib.ptr(x), x.shape[0], x.stride(0), self.d, thr, _lib.ptr(tv), _lib.ptr(self._codes), row0,
                                                 _lib.current_stream()))

    def add(self, x):
        """faiss add: floating rows [n, d] (binarised with the index's threshold) or uint8 [n, d / 8] rows already packed (np.packbits order)."""
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        packed = x.dtype == torch.uint8
        x = _as_rows(x, self.code_size if packed else self.d, "add: ")
        n = x.shape[0]
        self._make_room(n)
        if n:
            if packed:
                x = x.to(self.device).contiguous()
                _lib.check(self.lib.lrx_binary_store_rows(_lib.ptr(x), n, x.stride(0), self.d, _lib.ptr(self._codes), self.ntotal, _lib.current_stream()))
            else:
                x = x.to(device=self.device, dtype=torch.float32)
                self._pack_into(x if x.stride(1) == 1 else x.contiguous(), self.ntotal)
        self.ntotal += n

    def reconstruct_n(self, i0: int, n: int) -> torch.Tensor:
        """Rows [i0, i0 + n) as packed bytes: uint8 device tensor [n, d / 8] (faiss reconstruct of a binary index)."""
        _check_range(i0, n, self.ntotal)
        out = torch.empty(n, self.code_size, dtype=torch.uint8, device=self.device)
        if n:
            _lib.check(self.lib.lrx_binary_decode_rows(_lib.ptr(self._codes), i0, n, self.d, _lib.ptr(out), self.code_size, _lib.current_stream()))
        return out

    def codes(self) -> torch.Tensor:
        """The rows as a row-major uint8 [ntotal, d / 8] tensor (a copy: the stored layout is blocked)."""
        return self.reconstruct_n(0, self.ntotal)

    # -- persistence (faiss.write_index_binary / read_index_binary of an IndexBinaryFlat, see index_io.py) ---------------------
    def save(self, fname: str, chunk_rows: int = 1 << 20):
        from .index_io import write_binary_flat
        write_binary_flat(fname, (self.reconstruct_n(s, min(chunk_rows, self.ntotal - s)).cpu().numpy() for s in range(0, self.ntotal, chunk_rows)),
                          self.d, self.ntotal)

    @classmethod
    def load(cls, fname: str, device: Optional[torch.device] = None, id_base: int = 0, chunk_rows: int = 1 << 20) -> "BinaryFlatIndex":
        from .index_io import read_binary_flat
        mm = read_binary_flat(fname)
        idx = cls(mm.shape[1] * 8, capacity=mm.shape[0], device=device, id_base=id_base)
        for s in range(0, mm.shape[0], chunk_rows):
            idx.add(torch.from_numpy(np.array(mm[s:s + chunk_rows], copy=True)))
        return idx

    # -- search --------------------------------------------------------------------------------------------------
    def search(self, q, k: int, binary_k: int = 1000, rerank: bool = True, score_function: str = "dot", threshold=None,
               row_map: Optional[torch.Tensor] = None, flags: int = 0):
        """-> (D, I) device tensors [Q, k].  rerank=True: D fp32 scores of the float query against the +-1 rows over the Hamming top-binary_k
        candidates, descending, ties to the lower row, (-FLT_MAX, -1) padding.  rerank=False: D int32 Hamming distances, ascending, ties to the
        lower row, (2^31 - 1, -1) padding (binary_k is not used).  threshold: binarises the queries (default: the index's).  I = id_base + row, or
        row_map[row] (int64 CUDA tensor of >= ntotal entries) when given.  1 <= k <= binary_k <= 2048."""
        if score_function != "dot":
            raise NotImplementedError(f"BinaryFlatIndex.search: score_function {score_function!r} is not served (only 'dot')")
        k_error = None
        if rerank and not 1 <= k <= binary_k <= self.MAX_K:
            k_error = f"search: need 1 <= k <= binary_k <= {self.MAX_K}, got k={k}, binary_k={binary_k}"
        q, D, I = self._begin_search(q, k, row_map, torch.float32 if rerank else torch.int32, k_error)
        thr, tv = self._threshold_args(self.threshold if threshold is None else threshold)
        Q = q.shape[0]
        if Q == 0:
            return D, I
        ws = self._search_workspace(self.lib.lrx_binary_workspace_bytes(self.ntotal, self.d, Q, binary_k))
        if rerank:
            _lib.check(self.lib.lrx_binary_ip_search(_lib.ptr(self._codes), self.ntotal, self.d, _lib.ptr(q), Q, thr, _lib.ptr(tv), k, binary_k,
                                                     int(self.id_base), _lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(), flags,
                                                     _lib.current_stream()))
        else:
            _lib.check(self.lib.lrx_binary_hamming_search(_lib.ptr(self._codes), self.ntotal, self.d, _lib.ptr(q), Q, thr, _lib.ptr(tv), k,
                                                          int(self.id_base), _lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(), flags,
                                                          _lib.current_stream()))
        return D, I


_PQ_EPS = np.float32(1.0 / 1024.0)


def _pq_update(x_t: torch.Tensor, codes: torch.Tensor, K: int, cent: torch.Tensor, rng) -> torch.Tensor:
    """One k-means update of every sub-space: x_t fp64 [M, n, ds], codes int64 [M, n] -> centroids fp32 [M, K, ds].  The sums are fp64
    segmented sums over the rows sorted (stably) by code -- a fixed order, no float atomics -- so the update is deterministic.  Empty
    clusters are re-seeded as faiss does: split a cluster drawn with probability ~ (size - 1), the two copies perturbed by +-1/1024."""
    M, n, ds = x_t.shape
    order = torch.argsort(codes, dim=1, stable=True)
    xs = torch.gather(x_t, 1, order[:, :, None].expand(M, n, ds))
    cs = torch.cumsum(xs, dim=1)
    counts = torch.zeros(M, K, dtype=torch.int64, device=codes.device).scatter_add_(1, codes, torch.ones_like(codes))
    ends = torch.cumsum(counts, dim=1)
    cs0 = torch.cat([torch.zeros(M, 1, ds, dtype=cs.dtype, device=cs.device), cs], dim=1)          # cs0[:, e] = sum of the first e rows
    sums = torch.gather(cs0, 1, ends[:, :, None].expand(M, K, ds)) - torch.gather(cs0, 1, (ends - counts)[:, :, None].expand(M, K, ds))
    new = torch.where(counts[:, :, None] > 0, sums / counts.clamp(min=1)[:, :, None].double(), cent.double()).float()
    cnt = counts.cpu().numpy()
    if (cnt == 0).any():
        c = new.cpu().numpy()
        for m in range(M):
            _split_empty(c[m], cnt[m], n, rng)
        new = torch.from_numpy(c).to(new.device)
    return new


def _split_empty(c: np.ndarray, hassign: np.ndarray, n: int, rng):
    """faiss Clustering's handling of empty clusters (in place, fp32): copy a cluster drawn with probability (size - 1) / (n - K) and
    perturb the two copies symmetrically by +-1/1024 per coordinate (even coordinates: up for the new one, odd: down)."""
    K = c.shape[0]
    for ci in range(K):
        if hassign[ci] != 0:
            continue
        cj = 0
        while True:
            p = (float(hassign[cj]) - 1.0) / float(max(n - K, 1))
            if rng.random() < p:
                break
            cj = (cj + 1) % K
        c[ci] = c[cj]
        sign = np.where(np.arange(c.shape[1]) % 2 == 0, np.float32(1), np.float32(-1))
        c[ci] = c[ci] * (np.float32(1) + sign * _PQ_EPS)
        c[cj] = c[cj] * (np.float32(1) - sign * _PQ_EPS)
        hassign[ci] = hassign[cj] // 2
        hassign[cj] -= hassign[ci]


def merge_topk(D_parts: torch.Tensor, I_parts: torch.Tensor):
    """[R,Q,k] per-shard lists -> ([Q,k], [Q,k]) with the same ordering rule (score desc, id asc)."""
    lib = _lib.lib()
    R, Q, k = D_parts.shape
    D_parts, I_parts = D_parts.contiguous(), I_parts.contiguous()
    D = torch.empty(Q, k, dtype=torch.float32, device=D_parts.device)
    I = torch.empty(Q, k, dtype=torch.int64, device=D_parts.device)
    _lib.check(lib.lrx_merge_topk(_lib.ptr(D_parts), _lib.ptr(I_parts), R, Q, k, _lib.ptr(D), _lib.ptr(I), _lib.current_stream()))
    return D, I
