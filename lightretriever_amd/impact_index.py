"""HBM-resident impact index: the sparse half of the hybrid retriever (what the reference gets from Lucene's `-impact -pretokenized` search
over a JsonVectorCollection), backed by lrx_impact_search.  Contract: include/lrx.h; layout, kernel and measurements: DESIGN.md §5.4.6.

Not a code index (index.py): there are no dense rows.  Documents are sets of (term id, integer weight), queries sets of (term id, count);
a score is the exact integer dot product, returned as one fp32 conversion; only rows that share a term with the query are returned.  The
str -> int32 dictionary of the terms belongs to the caller (retriever.ImpactSearch)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .index import _range_args, _range_call, _range_empty, _workspace

SCORE_LIMIT = 1 << 31   # the device accumulates in int32: a query whose bound B_q reaches this is refused


def _as_i64(x, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.ndim != 1 or x.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be a 1-D int32 / int64 array, got {x.dtype} {tuple(x.shape)}")
    return x.to(torch.int64)


def query_csr(queries) -> tuple:
    """[(term ids, counts), ...] -> (q_off, q_term, q_cnt) numpy arrays, the form search() takes."""
    off = np.zeros(len(queries) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t, _ in queries])
    cat = lambda parts: np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts]) if len(parts) else np.zeros(0, np.int64)
    return off, cat([t for t, _ in queries]), cat([c for _, c in queries])


class ImpactIndex:
    """add / finalize / search / reset / ntotal / nnz.  Resident after finalize(): 8 bytes per posting ({int32 row, int32 weight}, grouped by
    term, ascending row inside a term), term_off int64 [n_terms + 1] on the device with a host copy (`term_off_host`), and on the host `maxw`
    int64 [n_terms], the largest weight of every term -- what the overflow refusal of search() reads.  Rows are numbered in insertion order.
    Nothing touches the GPU before finalize() (the first search after an add runs it), so documents can be collected and a query be refused
    without one.  Not persisted: the reference's Lucene index lives in a temporary directory too.  NOT thread-safe."""
    MAX_K = 2048
    range_row_chunk = 0   # lrx_range_impact_search's row_chunk: 0 = the library's 4 Mi; tests set a multiple of 128 (the hits do not depend on it)
    window_rows = 0   # lrx_impact_search's window_rows: 0 = the library's rule; tests and tools set a multiple of 128 (the hits do not depend on it)

    def __init__(self, device: Optional[torch.device] = None, id_base: int = 0):
        self.device = device
        self.id_base = id_base
        self.lib = None
        self._ws = None
        self.reset()

    def reset(self):
        """Drops the documents (and the term statistics: the index has seen no term afterwards)."""
        self.ntotal = 0
        self.n_terms = 0
        self.maxw = np.zeros(0, dtype=np.int64)
        self.term_off_host = np.zeros(1, dtype=np.int64)
        self._pending = []            # (rows, terms, weights) int64 tensors of the adds since the last finalize()
        self._pending_nnz = 0
        self._postings = None         # int32 [nnz, 2] on the device
        self._term_off = None         # int64 [n_terms + 1] on the device
        self._dirty = False

    @property
    def nnz(self) -> int:
        return (0 if self._postings is None else self._postings.shape[0]) + self._pending_nnz

    # -- documents ---------------------------------------------------------------------------------------------------
    def add(self, doc_terms, doc_weights, doc_offsets):
        """A ragged CSR of documents: document i holds terms doc_terms[doc_offsets[i]:doc_offsets[i + 1]] (ids >= 0, each at most once per
        document) with weights doc_weights[...] (1 <= weight < 2^31); numpy or torch, on any device.  The postings stay where the arrays are
        (device arrays are appended on the device) until finalize(); the host-side maxw is updated here."""
        terms, weights, off = _as_i64(doc_terms, "doc_terms"), _as_i64(doc_weights, "doc_weights"), _as_i64(doc_offsets, "doc_offsets")
        n = off.numel() - 1
        if n < 0 or terms.numel() != weights.numel() or not (terms.device == weights.device == off.device):
            raise ValueError("add: doc_offsets needs n + 1 entries, doc_terms / doc_weights one length, all three on one device")
        if n == 0:
            return
        counts = off[1:] - off[:-1]
        if int(off[0]) != 0 or int(off[-1]) != terms.numel() or bool((counts < 0).any()):
            raise ValueError("add: doc_offsets must ascend from 0 to len(doc_terms)")
        if self.ntotal + n >= 1 << 31:
            raise ValueError(f"add: {self.ntotal + n} rows do not fit the postings' int32 row")
        if terms.numel():
            if int(terms.min()) < 0 or int(terms.max()) >= (1 << 31) - 1:
                raise ValueError("add: term ids must be in [0, 2^31 - 1)")
            if int(weights.min()) < 1 or int(weights.max()) >= 1 << 31:
                raise ValueError("add: weights must be in [1, 2^31)")
            n_terms = max(self.n_terms, int(terms.max()) + 1)
            mw = torch.zeros(n_terms, dtype=torch.int64, device=terms.device).scatter_reduce_(0, terms, weights, "amax", include_self=True)
            maxw = np.zeros(n_terms, dtype=np.int64)
            maxw[:self.n_terms] = self.maxw
            self.maxw, self.n_terms = np.maximum(maxw, mw.cpu().numpy()), n_terms
            rows = torch.repeat_interleave(torch.arange(self.ntotal, self.ntotal + n, dtype=torch.int64, device=terms.device), counts)
            self._pending.append((rows, terms, weights))
            self._pending_nnz += terms.numel()
        self.ntotal += n
        self._dirty = True

    def finalize(self):
        """Postings sorted by (term, row) and term_off, on the device (plumbing: one torch.sort of a combined int64 key over all postings)."""
        if not self._dirty:
            return
        _lib.require_gpu()
        if self.lib is None:
            self.lib = _lib.lib()
            self.device = self.device or torch.device("cuda", torch.cuda.current_device())
        parts = [tuple(t.to(self.device) for t in p) for p in self._pending]
        if self._postings is not None and self._postings.shape[0]:
            old_terms = torch.repeat_interleave(torch.arange(self._term_off.numel() - 1, dtype=torch.int64, device=self.device),
                                                self._term_off[1:] - self._term_off[:-1])
            parts.insert(0, (self._postings[:, 0].to(torch.int64), old_terms, self._postings[:, 1].to(torch.int64)))
        if parts:
            key = torch.cat([(t << 32) | r for r, t, _ in parts])
            w = torch.cat([x for _, _, x in parts])
        else:
            key = w = torch.zeros(0, dtype=torch.int64, device=self.device)
        key, order = torch.sort(key)
        if key.numel() > 1 and bool((key[1:] == key[:-1]).any()):
            raise ValueError("finalize: a document holds a term twice (a document is a SET of (term, weight) pairs)")
        terms = key >> 32
        self._postings = torch.stack([(key & 0xFFFFFFFF).to(torch.int32), w[order].to(torch.int32)], dim=1).contiguous()
        self._term_off = torch.zeros(self.n_terms + 1, dtype=torch.int64, device=self.device)
        if terms.numel():
            self._term_off[1:] = torch.cumsum(torch.bincount(terms, minlength=self.n_terms), 0)
        self.term_off_host = self._term_off.cpu().numpy()
        self._pending, self._pending_nnz, self._dirty = [], 0, False

    # -- search --------------------------------------------------------------------------------------------------
    def check_queries(self, q_off, q_term, q_cnt) -> tuple:
        """The host-side half of search(): argument checks, terms without postings dropped, and the overflow refusal -- ValueError for any
        query whose bound B_q = sum_t count[t] * maxw[t] (int64) reaches 2^31.  -> (q_off, q_term, q_cnt) int32 numpy arrays.  No GPU."""
        off, term, cnt = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).astype(np.int64).reshape(-1) for x in (q_off, q_term, q_cnt))
        if off.size < 1 or off[0] != 0 or off[-1] != term.size or term.size != cnt.size or (np.diff(off) < 0).any():
            raise ValueError("search: q_off must ascend from 0 to len(q_term) == len(q_cnt)")
        if term.size and (term.min() < 0 or cnt.min() < 1):
            raise ValueError("search: term ids must be >= 0 and counts >= 1")
        known = term < self.n_terms
        mw = np.zeros(term.size, dtype=np.int64)
        mw[known] = self.maxw[term[known]]
        qid = np.repeat(np.arange(off.size - 1), np.diff(off))
        bound = np.zeros(off.size - 1, dtype=np.int64)
        # (a term's share is capped at 2^31, which already refuses the query: the int64 sum of fewer than 2^31 such shares cannot wrap)
        np.add.at(bound, qid, np.minimum(np.minimum(cnt, SCORE_LIMIT) * mw, SCORE_LIMIT))
        over = np.flatnonzero(bound >= SCORE_LIMIT)
        if over.size:
            raise ValueError(f"search: query {int(over[0])} could score 2^31 or more (B_q = sum of count x the term's largest weight >= "
                             f"{int(bound[over[0]])}); the index accumulates in int32 -- scale the counts or the weights down")
        keep = mw > 0
        new_off = np.zeros(off.size, dtype=np.int64)
        np.add.at(new_off, qid[keep] + 1, 1)
        return np.cumsum(new_off).astype(np.int32), term[keep].astype(np.int32), cnt[keep].astype(np.int32)

    def search(self, q_off, q_term, q_cnt, k: int, row_map: Optional[torch.Tensor] = None):
        """Queries in CSR form (query i: terms q_term[q_off[i]:q_off[i + 1]] with counts q_cnt[...] >= 1; a term may repeat, its counts add up)
        -> (D f32 [Q, k], I i64 [Q, k]) device tensors: the hits by score descending, ties to the lower row, then (-FLT_MAX, -1) padding.
        I = id_base + row, or row_map[row] (int64 CUDA tensor of >= ntotal entries) when given.  Raises ValueError before anything is launched
        for a query that could overflow (check_queries)."""
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"search: k={k} out of range (1..{self.MAX_K})")
        off, term, cnt = self.check_queries(q_off, q_term, q_cnt)
        self._dirty = self._dirty or self._postings is None
        self.finalize()
        if row_map is not None and not (row_map.is_cuda and row_map.dtype == torch.int64 and row_map.is_contiguous() and row_map.numel() >= self.ntotal):
            raise ValueError("row_map must be a contiguous int64 CUDA tensor of >= ntotal entries")
        Q = off.size - 1
        D = torch.empty(Q, k, dtype=torch.float32, device=self.device)
        I = torch.empty(Q, k, dtype=torch.int64, device=self.device)
        if Q == 0:
            return D, I
        csr = torch.from_numpy(np.concatenate([off, term, cnt])).to(self.device)       # one upload
        d_off, d_term, d_cnt = csr[:Q + 1], csr[Q + 1:Q + 1 + term.size], csr[Q + 1 + term.size:]
        ws = _workspace(vars(self), "_ws", int(self.lib.lrx_impact_workspace_bytes(self.ntotal, Q, k)), self.device)
        _lib.check(self.lib.lrx_impact_search(_lib.ptr(self._postings), _lib.ptr(self._term_off), self.n_terms, self.ntotal, _lib.ptr(d_off),
                                              _lib.ptr(d_term), _lib.ptr(d_cnt), Q, k, int(self.id_base), _lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map),
                                              _lib.ptr(ws), ws.numel(), int(self.window_rows), _lib.current_stream()))
        return D, I

    def range_search(self, q_off, q_term, q_cnt, radius: float):
        """Every hit above a score, never cut at k -> (lims i64[Q+1], D f32[lims[Q]], I i64[lims[Q]]) device tensors in the layout of
        FlatIPIndex.range_search: query i owns [lims[i], lims[i+1]); a row is in it iff it is a hit (S >= 1) and (float) S, the score search()
        reports, is strictly greater than `radius` -- a negative radius returns every hit; I = id_base + row in ascending row order.  Exact,
        deterministic, independent of window_rows and the row chunking.  The queries and the overflow refusal are search()'s
        (check_queries).  Synchronises with the host once per call; not under graph capture."""
        radius = _range_args("ImpactIndex", radius)
        off, term, cnt = self.check_queries(q_off, q_term, q_cnt)
        Q = off.size - 1
        if Q == 0 or self.ntotal == 0:
            _lib.require_gpu()
            return _range_empty(self.device or torch.device("cuda", torch.cuda.current_device()), Q)
        self._dirty = self._dirty or self._postings is None
        self.finalize()
        csr = torch.from_numpy(np.concatenate([off, term, cnt])).to(self.device)       # one upload
        d_off, d_term, d_cnt = csr[:Q + 1], csr[Q + 1:Q + 1 + term.size], csr[Q + 1 + term.size:]
        rc = int(self.range_row_chunk)
        ws = _workspace(vars(self), "_ws", int(self.lib.lrx_range_impact_workspace_bytes(self.ntotal, Q, rc)), self.device)
        stream = _lib.current_stream()

        def call(s, n, lc, Dc, Ic, cap):
            _lib.check(self.lib.lrx_range_impact_search(_lib.ptr(self._postings), _lib.ptr(self._term_off), self.n_terms, self.ntotal, _lib.ptr(d_off),
                                                        _lib.ptr(d_term), _lib.ptr(d_cnt), n, radius, int(self.id_base), _lib.ptr(lc), _lib.ptr(Dc),
                                                        _lib.ptr(Ic), cap, _lib.ptr(ws), ws.numel(), int(self.window_rows), stream, rc))
        return _range_call(self.device, Q, Q, call)
