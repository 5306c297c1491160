#!/usr/bin/env python3
"""range_search timing of the quantised and sparse indexes beside their own unchanged top-k search, same index, same process: one JSON line
per (index, Q, target) -- SQFp16Index 1M x 2048, PQIndex 1M x 1536 (M = 96), ImpactIndex 1M documents x 128 terms over 131 072 (tok-like
queries): the shapes of bench_sq_search.py / bench_pq_search.py / bench_impact_search.py.  Q = 1 and Q = 100; the radius is chosen for the
batch so that about 100 and about 10 000 rows pass per query (Q = 1: for that query).  HIP events, medians of 10 after 3 warm-up calls.
  ms_range     the whole range_search call as a user sees it (its read-back of lims[Q] and, when the result is larger than the first
               guess of 1024 hits per query, the second library call with the exact capacity: library_calls = 2);
  ms_top100 / ms_top1000   search(q, 100) / search(q, 1000) of the same index: the yardstick.
Expectation: fp16-SQ range ~ the fp16-SQ top-k; PQ and impact range ~ twice their top-k scan (two sweeps)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lightretriever_amd import ImpactIndex, PQIndex, SQFp16Index
from lightretriever_amd.impact_index import query_csr


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 4)


def unit_chunks(N, D, seed, chunk=1 << 17):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s in range(0, N, chunk):
        yield torch.nn.functional.normalize(torch.randn(min(chunk, N - s), D, generator=g, device="cuda"), dim=-1)


def unit_queries(Q, D):
    return torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)), dim=-1)


def dense_radius(idx, q, hits):
    """Radius at which ~hits rows per query pass: a quantile of the queries' scores over the first (up to) 64 Ki decoded rows."""
    sc = (q[:16] @ idx.reconstruct_n(0, min(65536, idx.ntotal)).T).flatten().float()
    return float(torch.quantile(sc, 1.0 - hits / idx.ntotal))


def report(name, shape, Q, target, radius, range_fn, top_fn, reps):
    lims, _, _ = range_fn()
    n = int(lims[-1])
    line = {"index": name, "shape": shape, "Q": Q, "target_hits": target, "radius": round(radius, 6), "hits_per_query": round(n / Q, 1),
            "library_calls": 2 if n > Q * 1024 else 1, "ms_range": timed(range_fn, reps), "ms_top100": timed(lambda: top_fn(100), reps),
            "ms_top1000": timed(lambda: top_fn(1000), reps)}
    line["range_over_top100"] = round(line["ms_range"] / line["ms_top100"], 3)
    line["range_over_top1000"] = round(line["ms_range"] / line["ms_top1000"], 3)
    print(json.dumps(line), flush=True)


def dense(name, idx, N, D, qs, targets, reps):
    for Q in qs:
        q = unit_queries(Q, D)
        for t in targets:
            r = dense_radius(idx, q, t)
            report(name, f"{N}x{D}", Q, t, r, lambda: idx.range_search(q, r), lambda k: idx.search(q, k), reps)


def impact(N, V, nnz, qs, targets, reps):
    import bench_impact_search as B
    idx = ImpactIndex()
    for p in B.corpus(N, V, nnz):
        idx.add(*p)
    idx.finalize()
    for Q in qs:
        csr = query_csr(B.make_queries(Q, V, "tok"))
        hits = idx.range_search(*csr, -1.0)                             # every hit: the radius is a quantile of the hits' own scores
        n_hits = int(hits[0][-1])
        for t in targets:
            frac = min(1.0, t * Q / max(n_hits, 1))
            r = float(torch.quantile(hits[1][:: n_hits // (1 << 24) + 1], 1.0 - frac)) if frac < 1.0 else -1.0
            report("impact", f"{N}x{nnz}/{V}", Q, t, r, lambda: idx.range_search(*csr, r), lambda k: idx.search(*csr, k), reps)
        del hits


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=str, default="1,100")
    ap.add_argument("--targets", type=str, default="100,10000")
    ap.add_argument("--only", type=str, default="sq_fp16,pq,impact")
    a = ap.parse_args()
    qs, targets, only = [int(x) for x in a.queries.split(",")], [int(x) for x in a.targets.split(",")], a.only.split(",")
    torch.cuda.set_device(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps}), flush=True)
    if "sq_fp16" in only:
        idx = SQFp16Index(2048, capacity=a.rows)
        for x in unit_chunks(a.rows, 2048, 0):
            idx.add(x)
        dense("sq_fp16", idx, a.rows, 2048, qs, targets, a.reps)
        del idx
        torch.cuda.empty_cache()
    if "pq" in only:
        idx = PQIndex(1536, 96, capacity=a.rows)
        idx.train(next(unit_chunks(min(a.rows, 1 << 20), 1536, 0, chunk=1 << 20)))
        for x in unit_chunks(a.rows, 1536, 0):
            idx.add(x)
        dense("pq", idx, a.rows, 1536, qs, targets, a.reps)
        del idx
        torch.cuda.empty_cache()
    if "impact" in only:
        impact(a.rows, 131072, 128, qs, targets, a.reps)
