#!/usr/bin/env python3
"""What it costs to hand the encoder's sparse vectors to the impact index: the dict path (convert_sparse_reps_to_json -> ImpactSearch.index,
one Python object per posting) against the device path (convert_sparse_reps_to_csr -> ImpactSearch.index with a SparseRows), same process,
same vectors.  One JSON line per leg.

Vectors: fp32 [B, V] at V = 128 256 with 128 .. 256 non-zeros per row at random columns, values in (0.01, 3) (weights 1 .. 300 at q = 100),
fixed seed; `--batches` batches of `--batch` rows, as encode_corpus hands them over.  Legs:
  ingest       per path: all batches converted and indexed into a fresh engine; `docs_per_s` from the wall clock around a device synchronise,
               `event_ms` from HIP events around the same work; `with_finalize`: the same plus ImpactIndex.finalize() (the one sort both
               paths share).  `d2h_bytes` is computed from the shapes of the copies the path makes, not measured.
  queries      `spr`-like queries (values in (0.5, 1.5): counts around 100): pseudo text + retrieve_with_emb against SparseRows +
               retrieve_with_emb, each on the engine its documents came through; the hits are compared.
  kernels      lrx_sparse_csr_count / lrx_sparse_csr_fill (and lrx_sparse_compact, the capacity kernel of the dict path) alone, HIP events;
               `read_gbps` over the B x V x 4 bytes a launch must read, `csr_share_of_hbm` = 2 x B x V x 4 B over both launches against the
               6.3 TB/s a stream read achieves on the MI355X.  Batches of 256 rows (131 MB) fit the 256 MiB Infinity Cache, 1024 rows do not.
Medians of --reps repetitions after a warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lightretriever_amd import _lib, ops
from lightretriever_amd.modeling import LrxHybridModel
from lightretriever_amd.retriever import ImpactSearch

HBM_STREAM_GBPS = 6300.0


class Converter:
    """convert_sparse_reps_to_json / _to_pseudo_text / _to_csr are methods of LrxHybridModel that only use its device."""
    device = torch.device("cuda", 0)
    convert_sparse_reps_to_json = LrxHybridModel.convert_sparse_reps_to_json
    convert_sparse_reps_to_pseudo_text = LrxHybridModel.convert_sparse_reps_to_pseudo_text
    convert_sparse_reps_to_csr = LrxHybridModel.convert_sparse_reps_to_csr


def vectors(B, V, lo, hi, g, nnz=(128, 256)):
    """fp32 [B, V]: per row a random number in `nnz` of distinct columns with values in (lo, hi)."""
    x = torch.zeros(B, V, device="cuda")
    n = torch.randint(nnz[0], nnz[1] + 1, (B, 1), device="cuda", generator=g)
    cols = torch.rand(B, V, device="cuda", generator=g).topk(nnz[1], dim=1).indices                  # distinct columns per row
    vals = torch.rand(B, nnz[1], device="cuda", generator=g) * (hi - lo) + lo
    vals = torch.where(torch.arange(nnz[1], device="cuda")[None, :] < n, vals, torch.zeros_like(vals))
    return x.scatter_(1, cols, vals)


def timed(fn, reps, warmup=1):
    """-> (median wall seconds, median event ms); fn's work is followed by a device synchronise inside the wall clock."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, ev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        ev.append(e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(ev)


def ingest(conv, batches, ids, path, finalize):
    eng = ImpactSearch()

    def run():
        eng._clear()
        for x, i in zip(batches, ids):
            eng.index(conv.convert_sparse_reps_to_json(x) if path == "dict" else conv.convert_sparse_reps_to_csr(x), i)
        if finalize:
            eng.impact_index.finalize()
    return eng, run


def d2h_bytes(path, batches, V):
    """Bytes the path copies to the host for these batches, from the shapes of its copies."""
    total = 0
    for x in batches:
        B = x.shape[0]
        cnt = ops.sparse_compact_csr(x, 100, empty_marker=False).row_off.diff()
        if path == "dict":      # counts [B] int32, then ids and weights [B, max count] int32
            total += 4 * B + 2 * 4 * B * int(cnt.max())
        else:                   # the length of the CSR; ImpactIndex.add: 7 scalar checks and the per-term maximum weights (int64 [V + 1])
            total += 8 + 7 * 8 + 8 * (V + 1)
    return total


def kernel_leg(B, V, reps, g):
    x = vectors(B, V, 0.01, 3.0, g)
    lib, s = _lib.lib(), _lib.current_stream()
    counts = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(lib.lrx_sparse_csr_count(_lib.ptr(x), B, V, V, 100, 1, _lib.ptr(counts), s))
    off = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(counts, 0)
    terms = torch.empty(int(off[-1]), dtype=torch.int32, device="cuda")
    weights = torch.empty_like(terms)
    _, t_count = timed(lambda: _lib.check(lib.lrx_sparse_csr_count(_lib.ptr(x), B, V, V, 100, 1, _lib.ptr(counts), s)), reps, warmup=2)
    _, t_fill = timed(lambda: _lib.check(lib.lrx_sparse_csr_fill(_lib.ptr(x), B, V, V, 100, 1, _lib.ptr(off), _lib.ptr(terms), _lib.ptr(weights), s)),
                      reps, warmup=2)
    cap = int(counts.max())
    ids, w = torch.empty(B, cap, dtype=torch.int32, device="cuda"), torch.empty(B, cap, dtype=torch.int32, device="cuda")
    _, t_cap = timed(lambda: _lib.check(lib.lrx_sparse_compact(_lib.ptr(x), B, V, V, 100, cap, _lib.ptr(ids), _lib.ptr(w), _lib.ptr(counts), s)), reps,
                     warmup=2)
    nbytes = B * V * 4
    print(json.dumps({"leg": "kernels", "rows": B, "vocab": V, "input_mb": round(nbytes / 1e6, 1), "csr_count_ms": round(t_count, 4),
                      "csr_fill_ms": round(t_fill, 4), "compact_ms": round(t_cap, 4), "csr_count_read_gbps": round(nbytes / t_count / 1e6),
                      "csr_fill_read_gbps": round(nbytes / t_fill / 1e6), "compact_read_gbps": round(nbytes / t_cap / 1e6),
                      "csr_share_of_hbm": round(2 * nbytes / (t_count + t_fill) / 1e6 / HBM_STREAM_GBPS, 3)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--top-k", type=int, default=100)
    ap.add_argument("--kernel-rows", type=int, nargs="*", default=[256, 1024])
    a = ap.parse_args()
    assert a.reps >= 5, "medians of at least 5 repetitions"
    _lib.require_gpu()
    torch.cuda.set_device(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    V, conv = a.vocab, Converter()
    batches = [vectors(a.batch, V, 0.01, 3.0, g) for _ in range(a.batches)]
    ids = [[f"d{j * a.batch + i}" for i in range(a.batch)] for j in range(a.batches)]
    n_docs = a.batch * a.batches
    engines, rates = {}, {}
    for finalize in (False, True):
        for path in ("dict", "csr"):
            eng, run = ingest(conv, batches, ids, path, finalize)
            wall, ev = timed(run, a.reps)
            engines[path] = eng
            rates[path, finalize] = n_docs / wall
            print(json.dumps({"leg": "ingest", "path": path, "with_finalize": finalize, "docs": n_docs, "batch": a.batch, "vocab": V,
                              "postings": eng.impact_index.nnz, "wall_ms": round(wall * 1e3, 2), "event_ms": round(ev, 2),
                              "docs_per_s": round(n_docs / wall), "d2h_bytes": d2h_bytes(path, batches, V)}), flush=True)
        print(json.dumps({"leg": "ingest_ratio", "with_finalize": finalize, "csr_over_dict_docs_per_s": round(rates["csr", finalize] / rates["dict", finalize], 2)}),
              flush=True)
    # queries: both engines hold the finalised corpus
    q = vectors(a.queries, V, 0.5, 1.5, g)
    qids = [f"q{i}" for i in range(a.queries)]
    legs = {"text": lambda: engines["dict"].retrieve_with_emb(conv.convert_sparse_reps_to_pseudo_text(q), qids, top_k=a.top_k),
            "csr": lambda: engines["csr"].retrieve_with_emb(conv.convert_sparse_reps_to_csr(q), qids, top_k=a.top_k)}
    same = legs["text"]() == legs["csr"]()
    qrate = {}
    for form, fn in legs.items():
        wall, ev = timed(fn, a.reps)
        qrate[form] = a.queries / wall
        print(json.dumps({"leg": "queries", "form": form, "queries": a.queries, "top_k": a.top_k, "wall_ms": round(wall * 1e3, 2), "event_ms": round(ev, 2),
                          "queries_per_s": round(a.queries / wall), "hits_equal": same}), flush=True)
    print(json.dumps({"leg": "queries_ratio", "csr_over_text_queries_per_s": round(qrate["csr"] / qrate["text"], 2)}), flush=True)
    del batches, engines
    torch.cuda.empty_cache()
    for B in a.kernel_rows:
        kernel_leg(B, V, max(a.reps, 10), g)
