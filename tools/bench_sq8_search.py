#!/usr/bin/env python3
"""SQ8Index against SQFp16Index and FlatIPIndex, same process, same rows: one JSON line per shape -- 1M x 2048 for Q in {1, 100, 1000} x
k in {100, 1000}, 10M x 256 -- plus the training and encoding time of 1M x 2048 rows and the stream-read ceiling of the same run (the
fastest read leg of tools/bench_hbm.py over an 8 GB buffer).  `codes_gbps` is the 8-bit codes' bytes over the whole search time: a lower bound of
what the scan kernel streams (the kernel's own time: rocprofv3 --kernel-trace --stats, profiles/README.md).  CUDA events, medians after
warm-up.  --capacity N: the three indexes over N x 2048 rows next to each other (12M: 221 GB resident)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from lightretriever_amd import FlatIPIndex, SQ8Index, SQFp16Index


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


def stream_ceiling():
    """Every leg of tools/bench_hbm.py in this process; the ceiling is its fastest pure-read leg."""
    import bench_hbm
    legs = bench_hbm.legs()
    best = max((n for n in legs if "copy" not in n), key=lambda n: legs[n][1])
    return {"bench_hbm_gbps": {n: round(v[1]) for n, v in legs.items()}, "stream_read_ceiling_leg": best, "stream_read_ceiling_gbps": round(legs[best][1])}


def build_cost(N, D):
    x = torch.cat(list(chunks(N, D, 4)))
    idx = SQ8Index(D, capacity=N)
    t_train = timed(lambda: idx.train(x), 5)

    def enc():
        idx.reset()
        idx.add(x)
    return {"shape": f"{N}x{D}", "train_ms": round(t_train, 3), "encode_ms": round(timed(enc, 5), 3)}


def shape(N, D, legs, reps, others=True):
    sq8 = SQ8Index(D, capacity=N)
    sq16 = SQFp16Index(D, capacity=N) if others else None
    flat = FlatIPIndex(D, capacity=N) if others else None
    for i, x in enumerate(chunks(N, D, 0)):
        if i == 0:
            sq8.train(x)                                           # (the range of the first chunk; later rows clamp)
        sq8.add(x)
        if others:
            sq16.add(x)
            flat.add(x)
    for Q, k in legs:
        q = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)), dim=-1)
        t8 = timed(lambda: sq8.search(q, k), reps)
        out = {"shape": f"{N}x{D}", "Q": Q, "k": k, "ms_sq8": round(t8, 4), "codes_gbps": round(N * D / t8 / 1e6, 0),
               "resident_gb_sq8": round(sq8._codes.numel() / 1e9, 3)}
        if others:
            t16 = timed(lambda: sq16.search(q, k), reps)
            tf = timed(lambda: flat.search(q, k), reps)
            t8b = timed(lambda: sq8.search(q, k), reps)            # (A-B-A: drift shows as ms_sq8 != ms_sq8_again)
            out.update({"ms_sqfp16": round(t16, 4), "ms_flat": round(tf, 4), "ms_sq8_again": round(t8b, 4),
                        "sq8_over_sqfp16": round(min(t8, t8b) / t16, 3), "sq8_over_flat": round(min(t8, t8b) / tf, 3)})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=0, help="rows of an N x 2048 leg with all three indexes resident (0: skip)")
    ap.add_argument("--one-leg", action="store_true", help="1M x 2048, Q = 100, k = 100 on SQ8Index only (the profiled leg)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    if a.one_leg:
        shape(1_000_000, 2048, [(100, 100)], a.reps, others=False)
        sys.exit(0)
    print(json.dumps(stream_ceiling()), flush=True)
    torch.cuda.empty_cache()
    print(json.dumps(build_cost(1_000_000, 2048)), flush=True)
    torch.cuda.empty_cache()
    shape(1_000_000, 2048, [(Q, k) for Q in (1, 100, 1000) for k in (100, 1000)], a.reps)
    torch.cuda.empty_cache()
    shape(10_000_000, 256, [(100, 100)], a.reps)
    torch.cuda.empty_cache()
    if a.capacity:
        shape(a.capacity, 2048, [(100, 100)], 5)
