#!/usr/bin/env python3
"""IVFFlatIndex against FlatIPIndex, same process, same rows: ONE JSON line for the clustered corpus of DESIGN §5.4 (N x 2048 unit rows in
1000 clusters, default 1M; queries drawn near corpus rows), nlist = 1024, k = 100.  Per (Q, nprobe) in {1, 16, 100, 1000} x {1, 8, 32, 128}
  ms            IVFFlatIndex.search(q, k, nprobe): the coarse search and the scan, as the index runs them (and the coarse search alone)
  recall        recall@k against FlatIPIndex.search
  scanned       bytes of rows the call scans: every touched cell once (what the cell-major scan reads from HBM) and once per probing query
                (what a query-major scan would read), and the GB/s either implies over ms
next to FlatIPIndex.search's own ms per Q (taken before and after the rest: A-B-A), the read rate lrx_probe_stream_read reaches in this
run, and the train / add / first-search (cell-order rebuild) times.  HIP events, medians after warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import math

import numpy as np
import torch

from lightretriever_amd import FlatIPIndex, IVFFlatIndex, _lib
from lightretriever_amd.synth import clustered_corpus


def timed(fn, reps=None, budget_ms=300.0):
    """Median event ms of fn after two warm-up calls; reps: given, or 3 .. 20 so that the timed calls take about budget_ms."""
    for _ in range(2):
        fn()
    ts = []
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
        n = reps if reps is not None else max(3, min(20, int(budget_ms / max(ts[0], 1e-3))))
        if len(ts) >= n:
            return statistics.median(ts)


def stream_rate(dev):
    """GB/s of lrx_probe_stream_read over 4 GiB (beyond the Infinity Cache), the best of four grid sizes: bench.py's in-run ceiling."""
    lib = _lib.lib()
    buf = torch.zeros(1 << 30, dtype=torch.int32, device=dev)
    best = 0.0
    for n_wg in (1024, 2048, 4096, 8192):
        sink = torch.zeros(n_wg, dtype=torch.int32, device=dev)
        ms = timed(lambda: _lib.check(lib.lrx_probe_stream_read(_lib.ptr(buf), buf.numel() * 4, _lib.ptr(sink), n_wg, _lib.current_stream())), 6)
        best = max(best, buf.numel() * 4 / (ms * 1e-3) / 1e9)
    return best


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def recall(I: torch.Tensor, ref: torch.Tensor) -> float:
    I, ref = I.cpu().numpy(), ref.cpu().numpy()
    return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(I, ref)) / ref.size


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 100, 1000])
    ap.add_argument("--nprobes", type=int, nargs="+", default=[1, 8, 32, 128])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N, D, k = a.rows, a.d, a.k
    out = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{D}", "nlist": a.nlist, "k": k, "corpus": "1000 clusters, intra_cos 0.9, unit rows"}
    out["stream_read_gbps"] = round(stream_rate(dev), 1)

    flat = FlatIPIndex(D, capacity=N)
    clustered_corpus(flat.append_slot(N), n_clusters=1000, intra_cos=0.9, dup_frac=0.01, seed=5)
    flat.commit(N)
    x = flat.vectors
    Qmax = max(a.queries)
    g = torch.Generator(device=dev).manual_seed(1)
    near = x[torch.randint(0, N, (Qmax,), generator=g, device=dev)]
    u = torch.nn.functional.normalize(torch.randn(Qmax, D, generator=g, device=dev), dim=-1)
    qs = torch.nn.functional.normalize(math.sqrt(0.9) * near + math.sqrt(0.1) * u, dim=-1).contiguous()

    flat_ms = {Q: timed(lambda: flat.search(qs[:Q], k)) for Q in a.queries}
    ref = flat.search(qs, k)[1].clone()

    ivf = IVFFlatIndex(D, a.nlist, nprobe=1, capacity=N)
    out["train_s"] = round(wall(lambda: ivf.train(x)), 3)

    def add_all():
        for s in range(0, N, 262144):
            ivf.add(x[s:s + 262144])
    out["add_s"] = round(wall(add_all), 3)
    out["rebuild_s"] = round(wall(ivf._finalize), 3)
    sizes = ivf.list_sizes
    out["cells"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}

    out["configs"] = []
    for Q in a.queries:
        q = qs[:Q]
        for nprobe in a.nprobes:
            if nprobe > a.nlist:
                continue
            probes = ivf.quantizer.search(q, nprobe)[1].cpu().numpy()
            per_query = int(sizes[probes].sum())
            once = int(sizes[np.unique(probes)].sum())
            ms = timed(lambda: ivf.search(q, k, nprobe=nprobe))
            coarse_ms = timed(lambda: ivf.quantizer.search(q, nprobe))
            I = ivf.search(q, k, nprobe=nprobe)[1]
            out["configs"].append({"Q": Q, "nprobe": nprobe, "ms": round(ms, 4), "coarse_ms": round(coarse_ms, 4), "flat_ms": round(flat_ms[Q], 4),
                                   f"recall_at_{k}": round(recall(I, ref[:Q]), 4), "max_scan_rows": ivf.max_scan_rows(nprobe),
                                   "scanned_gb_cells_once": round(once * D * 4 / 1e9, 4), "scanned_gb_per_query": round(per_query * D * 4 / 1e9, 4),
                                   "gbps_cells_once": round(once * D * 4 / (ms * 1e-3) / 1e9, 1), "gbps_per_query": round(per_query * D * 4 / (ms * 1e-3) / 1e9, 1)})
    out["flat_ms"] = {str(Q): round(v, 4) for Q, v in flat_ms.items()}
    out["flat_ms_again"] = {str(Q): round(timed(lambda: flat.search(qs[:Q], k)), 4) for Q in a.queries}     # (A-B-A: drift shows as a difference)
    out["resident_gb"] = {"flat_with_shadow": round(N * D * 6 / 1e9, 2), "ivf_rows": round(N * D * 4 / 1e9, 2)}
    out["device_errors"] = int(_lib.lib().lrx_device_error_count(0))
    print(json.dumps(out), flush=True)
