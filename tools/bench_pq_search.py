#!/usr/bin/env python3
"""PQIndex (IndexPQ, M = 96, 8-bit codes) beside FlatIPIndex on the same rows, same process: one JSON line per (shape, Q, k) -- 1M x 1536
and 10M x 1536, Q in {1, 100, 1000}, k in {100, 1000}.  CUDA events, medians after warm-up, order pq / flat / pq again.  The PQ index is
trained on the first 1M rows (timed: train, then encode of 1M rows) and the 10M shard reuses those centroids; its codes are encoded
from the same rows the flat index holds."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lightretriever_amd import FlatIPIndex, PQIndex


def chunks(N, D, seed, chunk=1 << 18):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s in range(0, N, chunk):
        yield torch.nn.functional.normalize(torch.randn(min(chunk, N - s), D, generator=g, device="cuda"), dim=-1)


def timed(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(N, D, M, reps, trained, qs, ks):
    pq = PQIndex(D, M, capacity=N)
    flat = FlatIPIndex(D, capacity=N)
    out = {}
    if trained is None:
        first = next(chunks(1 << 20, D, 0, chunk=1 << 20))
        out["train_1M_s"] = round(wall(lambda: pq.train(first)), 3)
        out["encode_1M_s"] = round(wall(lambda: pq.encode(first)), 3)
        del first
    else:
        pq.set_contents(trained, torch.zeros(0, M, dtype=torch.uint8))
    for x in chunks(N, D, 0):
        pq.add(x)
        flat.add(x)
    torch.cuda.synchronize()
    lines = []
    for Q in qs:
        q = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)), dim=-1)
        for k in ks:
            t_pq = timed(lambda: pq.search(q, k), reps)
            t_flat = timed(lambda: flat.search(q, k), reps)
            t_pq2 = timed(lambda: pq.search(q, k), reps)
            lines.append({"shape": f"{N}x{D}", "M": M, "Q": Q, "k": k, "ms_pq": round(t_pq, 4), "ms_flat": round(t_flat, 4), "ms_pq_again": round(t_pq2, 4),
                          "pq_over_flat": round(min(t_pq, t_pq2) / t_flat, 4), "resident_gb_pq": round(pq._codes.numel() / 1e9, 3),
                          "resident_gb_flat": round((flat._x.numel() * 4 + flat._xb.numel() * 2) / 1e9, 3), **out})
            print(json.dumps(lines[-1]), flush=True)
    return pq.centroids


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=str, default="1000000,10000000")
    ap.add_argument("--queries", type=str, default="1,100,1000")
    ap.add_argument("--k", type=str, default="100,1000")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cent = None
    for N in [int(v) for v in a.rows.split(",")]:
        cent = run(N, 1536, 96, a.reps, cent, [int(v) for v in a.queries.split(",")], [int(v) for v in a.k.split(",")])
        torch.cuda.empty_cache()
