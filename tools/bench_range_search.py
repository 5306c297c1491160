#!/usr/bin/env python3
"""FlatIPIndex.range_search timing: one JSON line per shape -- 1M x 2048 with Q = 1 / 100 / 256 at radii giving ~10, ~1 000 and ~20 000 hits
per query, 125 k x 2048 with Q = 100, and search(q, k=1000) on the same index in the same process as the yardstick.  CUDA events, medians
after warm-up.  Two times per range shape:
  ms_one_call  ONE lrx_flat_ip_range_search call with outputs that fit (what the kernels cost; no host synchronisation inside);
  ms           the whole FlatIPIndex.range_search call as a user sees it: its read-back of lims[Q] and, when the result is larger than its
               first guess of 1024 hits per query, a second full library call with the exact capacity (library_calls = 2).
matrix_path_queries: queries ONE library call sent to the score-matrix path because their candidate list overflowed."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lightretriever_amd import FlatIPIndex, _lib


def build(N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = FlatIPIndex(D, capacity=N)
    slot = idx.append_slot(N)
    for s in range(0, N, 65536):
        e = min(s + 65536, N)
        slot[s:e] = torch.nn.functional.normalize(torch.randn(e - s, D, generator=g, device="cuda"), dim=-1)
    idx.commit(N)
    return idx, g


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
    return statistics.median(ts), min(ts)


def radius_for(idx, q, hits):
    """Radius whose mean hit count per query is ~hits: a quantile of the queries' scores over a 64 k-row sample."""
    X = idx.vectors[:65536]
    sc = (q[:16] @ X.T).flatten()
    frac = hits / idx.ntotal
    return float(torch.quantile(sc.float()[:1 << 24], 1.0 - frac))


def main():
    reps = int(os.environ.get("REPS", 10))
    lib = _lib.lib()
    for N, D, qs, targets in ((1_000_000, 2048, (1, 100, 256), (10, 1000, 20000)), (125_000, 2048, (100,), (10, 1000, 20000))):
        idx, g = build(N, D, 7)
        for Q in qs:
            q = torch.nn.functional.normalize(torch.randn(Q, D, generator=g, device="cuda"), dim=-1)
            ms, mn = timed(lambda: idx.search(q, 1000), reps)
            print(json.dumps({"op": "search", "N": N, "D": D, "Q": Q, "k": 1000, "ms": round(ms, 4), "ms_min": round(mn, 4)}), flush=True)
            for t in targets:
                r = radius_for(idx, q, t)
                lims, _, _ = idx.range_search(q, r)
                n = int(lims[-1])
                calls = 2 if n > Q * 1024 else 1
                # one library call with outputs that fit, on the index's own workspace
                Do = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
                Io = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
                lo = torch.empty(Q + 1, dtype=torch.int64, device="cuda")
                ws = idx._ws

                def one_call():
                    _lib.check(lib.lrx_flat_ip_range_search(_lib.ptr(idx._x), idx.ntotal, idx._x.stride(0), D, _lib.ptr(idx._xb), _lib.ptr(idx._bounds),
                                                            _lib.ptr(q), Q, r, 0, _lib.ptr(lo), _lib.ptr(Do), _lib.ptr(Io), n, _lib.ptr(ws), ws.numel(),
                                                            _lib.current_stream()))
                torch.cuda.synchronize()
                lib.lrx_search_fallback_count(1)
                one_call()
                torch.cuda.synchronize()
                fb = int(lib.lrx_search_fallback_count(1))
                assert int(lo[-1]) == n
                ms1, mn1 = timed(one_call, reps)
                ms, mn = timed(lambda: idx.range_search(q, r), reps)
                print(json.dumps({"op": "range_search", "N": N, "D": D, "Q": Q, "radius": round(r, 6), "hits_per_query": round(n / Q, 1),
                                  "matrix_path_queries": fb, "ms_one_call": round(ms1, 4), "ms_one_call_min": round(mn1, 4),
                                  "library_calls": calls, "ms": round(ms, 4), "ms_min": round(mn, 4)}), flush=True)
        del idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
