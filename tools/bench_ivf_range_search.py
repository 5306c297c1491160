#!/usr/bin/env python3
"""Range search over the probed cells against the top-k search over the same cells and against the flat range search, same process, same
rows: ONE JSON line for the clustered corpus of DESIGN §5.4 (N x 2048 unit rows in 1000 clusters, default 1M; queries drawn near corpus rows),
nlist = 1024, for IVFFlatIndex and IVFSQIndex.  Per index and (Q, nprobe) in {1, 16, 100, 1000} x {1, 8, 32, 128}, at two radii taken from the
data -- r100: the median over the queries of the 100th-best scanned score (about 100 hits per query); r1pct: the score 1 % of the scanned
(query, row) pairs exceed (of up to 16 queries) --
  range_ms        range_search_probed(q, radius, nprobe): the coarse search, the scan, count + lims + fill, the host read of the result length
                  (and the second library call when the first guess of 1024 hits per query was short: `calls`)
  cells_ms        the library call alone over the quantiser's cells (ops.ivf_*_ip_range_search): range_ms without the coarse search
  topk_ms         search(q, 100, nprobe) on the same cells, topk_cells_ms its library call alone (ops.ivf_*_ip_topk over the same probes);
                  cells_ms - topk_cells_ms is what count + lims + fill + the host read cost over the selection (the kernels inside one library
                  call cannot be told apart by events from outside it)
  flat_range_ms   FlatIPIndex.range_search(q, radius) over all rows at the same radius, and its hits per query
  hits_per_query, scanned rows per query, lrx_device_error_count.
HIP events, medians after warm-up."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from lightretriever_amd import FlatIPIndex, IVFFlatIndex, IVFSQIndex, _lib, ops
from lightretriever_amd.synth import clustered_corpus


def timed(fn, reps=None, budget_ms=200.0):
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


def radii(idx, q, nprobe):
    """(r100, r1pct) of the class note, from the index's own scores."""
    D = idx.search(q, 100, nprobe=nprobe)[0]
    r100 = float(D[:, 99].median())
    every = idx.range_search_probed(q[:16], float("-inf"), nprobe)[1]
    r1 = float(torch.kthvalue(every, max(1, int(every.numel() * 0.99))).values) if every.numel() else 0.0
    return r100, r1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 100, 1000])
    ap.add_argument("--nprobes", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--indexes", nargs="+", default=["ivfflat", "ivfsq"], choices=["ivfflat", "ivfsq"])
    ap.add_argument("--no-flat", action="store_true", help="skip FlatIPIndex.range_search (a profile of the IVF kernels alone)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N, D = a.rows, a.d
    out = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{D}", "nlist": a.nlist, "corpus": "1000 clusters, intra_cos 0.9, unit rows"}

    flat = FlatIPIndex(D, capacity=N)
    clustered_corpus(flat.append_slot(N), n_clusters=1000, intra_cos=0.9, dup_frac=0.01, seed=5)
    flat.commit(N)
    x = flat.vectors
    Qmax = max(a.queries)
    g = torch.Generator(device=dev).manual_seed(1)
    near = x[torch.randint(0, N, (Qmax,), generator=g, device=dev)]
    u = torch.nn.functional.normalize(torch.randn(Qmax, D, generator=g, device=dev), dim=-1)
    qs = torch.nn.functional.normalize(math.sqrt(0.9) * near + math.sqrt(0.1) * u, dim=-1).contiguous()

    out["indexes"] = {}
    for name in a.indexes:
        idx = IVFFlatIndex(D, a.nlist, nprobe=1, capacity=N) if name == "ivfflat" else IVFSQIndex(D, a.nlist, nprobe=1, by_residual=True, capacity=N)
        idx.train(x)
        for s in range(0, N, 262144):
            idx.add(x[s:s + 262144])
        idx._finalize()
        sizes = idx.list_sizes
        configs = []
        for Q in a.queries:
            q = qs[:Q]
            for nprobe in a.nprobes:
                if nprobe > a.nlist:
                    continue
                coarse, probes = idx.quantizer.search(q, nprobe)
                scanned = int(sizes[probes.cpu().numpy()].sum())
                scan = idx.max_scan_rows(nprobe)
                topk_ms = timed(lambda: idx.search(q, 100, nprobe=nprobe))
                coarse_ms = timed(lambda: idx.quantizer.search(q, nprobe))
                if name == "ivfflat":
                    topk_cells = lambda: ops.ivf_flat_ip_topk(q, idx.stored_rows(), idx.list_off, idx.row_ids, probes, 100, scan, 0, None, ws_slots=vars(idx))
                else:
                    topk_cells = lambda: ops.ivf_sq_fp16_ip_topk(q, idx.stored_codes(), idx.list_off, idx.row_ids, probes, coarse, True, 100, scan, 0, None,
                                                                 ws_slots=vars(idx))
                topk_cells_ms = timed(topk_cells)
                c = {"Q": Q, "nprobe": nprobe, "max_scan_rows": scan, "scanned_per_query": round(scanned / Q, 1), "topk_ms": round(topk_ms, 4),
                     "topk_cells_ms": round(topk_cells_ms, 4), "coarse_ms": round(coarse_ms, 4)}
                for tag, radius in zip(("r100", "r1pct"), radii(idx, q, nprobe)):
                    lims = idx.range_search_probed(q, radius, nprobe)[0]
                    hits = int(lims[-1])
                    r = {"radius": round(radius, 6), "hits_per_query": round(hits / Q, 1), "calls": 2 if hits > Q * 1024 else 1,
                         "range_ms": round(timed(lambda: idx.range_search_probed(q, radius, nprobe)), 4),
                         "cells_ms": round(timed(lambda: idx.range_search_preassigned(q, radius, probes, coarse)), 4)}
                    if not a.no_flat:
                        fl = flat.range_search(q, radius)[0]
                        r["flat_hits_per_query"] = round(int(fl[-1]) / Q, 1)
                        r["flat_range_ms"] = round(timed(lambda: flat.range_search(q, radius)), 4)
                    c[tag] = r
                configs.append(c)
        out["indexes"][name] = {"cells": {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max())}, "configs": configs}
        del idx
        torch.cuda.empty_cache()
    out["device_errors"] = int(_lib.lib().lrx_device_error_count(0))
    print(json.dumps(out), flush=True)
