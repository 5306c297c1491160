#!/usr/bin/env python3
"""SQFp16Index against FlatIPIndex, same process, same rows (the flat index holds the rows the codes decode to, so both return the same
results): one JSON line per shape -- 1M x 2048 (Q = 100, k = 100) and 100 k x 2048 (Q = 1000, k = 1000).  CUDA events, medians after
warm-up.  --capacity: a shard the flat index cannot hold on one card (default 30M x 2048: 123 GB of codes, 369 GB flat) -- build time,
search time and an fp64 spot check of a few queries."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lightretriever_amd import FlatIPIndex, SQFp16Index


def chunks(N, D, seed, chunk=65536):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s in range(0, N, chunk):
        yield torch.nn.functional.normalize(torch.randn(min(chunk, N - s), D, generator=g, device="cuda"), dim=-1)


def timed(fn, reps):
    for _ in range(3):
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


def ab(N, D, Q, k, reps):
    sq = SQFp16Index(D, capacity=N)
    flat = FlatIPIndex(D, capacity=N)
    for x in chunks(N, D, 0):
        sq.add(x)
        flat.add(x.half().float())
    q = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)), dim=-1)
    Ds, Is = sq.search(q, k)
    Df, If = flat.search(q, k)
    same = bool(torch.equal(Is, If) and torch.equal(Ds.view(torch.int32), Df.view(torch.int32)))
    t_sq = timed(lambda: sq.search(q, k), reps)
    t_flat = timed(lambda: flat.search(q, k), reps)
    t_sq2 = timed(lambda: sq.search(q, k), reps)                   # (A-B-A: drift shows as t_sq != t_sq2)
    return {"shape": f"{N}x{D}", "Q": Q, "k": k, "ms_sq": round(t_sq, 4), "ms_flat": round(t_flat, 4), "ms_sq_again": round(t_sq2, 4),
            "sq_over_flat": round(min(t_sq, t_sq2) / t_flat, 4), "bit_identical": same,
            "resident_gb_sq": round(sq._xb.numel() * 2 / 1e9, 3), "resident_gb_flat": round((flat._x.numel() * 4 + flat._xb.numel() * 2) / 1e9, 3)}


def capacity(N, D, Q, k, reps):
    t0 = time.time()
    sq = SQFp16Index(D, capacity=N)
    for x in chunks(N, D, 2):
        sq.add(x)
    torch.cuda.synchronize()
    t_build = time.time() - t0
    q = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)), dim=-1)
    Ds, Is = sq.search(q, k)
    t = timed(lambda: sq.search(q, k), reps)
    ok = True
    for i in range(4):                                             # fp64 spot check of four queries over all rows
        qd = q[i:i + 1].double()
        S = torch.cat([(qd @ sq.reconstruct_n(s, min(1 << 20, N - s)).double().T).float() for s in range(0, N, 1 << 20)], dim=1)[0]
        v, j = torch.sort(S, descending=True, stable=True)
        ok = ok and bool(torch.equal(j[:k], Is[i]) and torch.equal(v[:k].view(torch.int32), Ds[i].view(torch.int32)))
        del S, v, j
    return {"shape": f"{N}x{D}", "Q": Q, "k": k, "build_s": round(t_build, 2), "ms_sq": round(t, 4), "fp64_spot_check_4_queries": ok,
            "resident_gb_sq": round(sq._xb.numel() * 2 / 1e9, 2), "flat_would_need_gb": round(N * D * 6 / 1e9, 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=0, help="rows of the capacity run (0: skip); 30000000 is the 123-GB shard")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for N, D, Q, k in ((1_000_000, 2048, 100, 100), (100_000, 2048, 1000, 1000)):
        print(json.dumps(ab(N, D, Q, k, a.reps)), flush=True)
        torch.cuda.empty_cache()
    if a.capacity:
        print(json.dumps(capacity(a.capacity, 2048, 100, 100, 5)), flush=True)
