#!/usr/bin/env python3
"""IVFPQIndex against PQIndex, IVFFlatIndex and FlatIPIndex, same process, same rows: ONE JSON line for the clustered corpus of DESIGN §5.4
(N x 2048 unit rows in 1000 clusters, default 1M; queries drawn near corpus rows), nlist = 1024, k = 100.  Per M in {64, 128} and
(Q, nprobe) in {1, 16, 100, 1000} x {1, 8, 32, 128}
  ms            IVFPQIndex.search(q, k, nprobe), by_residual: the coarse search, the lookup tables, the plan, the scan and the selection, as the
                index runs them; coarse_ms: the coarse search alone; lut_ms: lrx_pq_lut alone (the tables of the Q queries)
  pq_ms         PQIndex.search (same M), ivf_flat_ms: IVFFlatIndex.search (same cells, same nprobe), flat_ms: FlatIPIndex.search -- unchanged
                code, measured in this run
  recall        recall@k against FlatIPIndex.search: by_residual True and False, PQIndex's own, and RefineFlatIndex(IVFPQIndex, k_factor = 4)
next to the train / add / rebuild times.  HIP events, medians after warm-up.  --repeat N: only N calls of one configuration (the first of
--queries, --nprobes and --Ms), for a kernel trace."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from lightretriever_amd import FlatIPIndex, IVFFlatIndex, IVFPQIndex, PQIndex, RefineFlatIndex, _lib
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def recall(I: torch.Tensor, ref: torch.Tensor) -> float:
    I, ref = I.cpu().numpy(), ref.cpu().numpy()
    return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(I, ref)) / ref.size


def add_all(idx, x):
    for s in range(0, x.shape[0], 262144):
        idx.add(x[s:s + 262144])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 100, 1000])
    ap.add_argument("--nprobes", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--Ms", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--k-factor", type=float, default=4.0)
    ap.add_argument("--repeat", type=int, default=0, help="only call IVFPQIndex.search this many times at --queries[0], --nprobes[0], --Ms[0]")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    N, D, k = a.rows, a.d, a.k
    out = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{D}", "nlist": a.nlist, "k": k, "k_factor": a.k_factor,
           "corpus": "1000 clusters, intra_cos 0.9, unit rows"}

    flat = FlatIPIndex(D, capacity=N)
    clustered_corpus(flat.append_slot(N), n_clusters=1000, intra_cos=0.9, dup_frac=0.01, seed=5)
    flat.commit(N)
    x = flat.vectors
    Qmax = max(a.queries)
    g = torch.Generator(device=dev).manual_seed(1)
    near = x[torch.randint(0, N, (Qmax,), generator=g, device=dev)]
    u = torch.nn.functional.normalize(torch.randn(Qmax, D, generator=g, device=dev), dim=-1)
    qs = torch.nn.functional.normalize(math.sqrt(0.9) * near + math.sqrt(0.1) * u, dim=-1).contiguous()

    if a.repeat:
        Q, nprobe, M = a.queries[0], a.nprobes[0], a.Ms[0]
        idx = IVFPQIndex(D, a.nlist, M, nprobe=nprobe, capacity=N)
        idx.train(x)
        add_all(idx, x)
        for _ in range(a.repeat):
            idx.search(qs[:Q], k)
        torch.cuda.synchronize()
        print(json.dumps({"repeat": a.repeat, "Q": Q, "nprobe": nprobe, "M": M}), flush=True)
        sys.exit(0)

    flat_ms = {Q: timed(lambda: flat.search(qs[:Q], k)) for Q in a.queries}
    ref = flat.search(qs, k)[1].clone()

    ivf = IVFFlatIndex(D, a.nlist, nprobe=1, capacity=N)
    out["ivf_flat_train_s"] = round(wall(lambda: ivf.train(x)), 3)
    add_all(ivf, x)
    ivf._finalize()
    sizes = ivf.list_sizes
    out["cells"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}
    ivf_ms = {(Q, p): timed(lambda: ivf.search(qs[:Q], k, nprobe=p)) for Q in a.queries for p in a.nprobes if p <= a.nlist}

    out["per_M"] = []
    for M in a.Ms:
        rec = {"M": M}
        pq = PQIndex(D, M, capacity=N)
        rec["pq_train_s"] = round(wall(lambda: pq.train(x)), 3)
        rec["pq_add_s"] = round(wall(lambda: add_all(pq, x)), 3)
        pq_ms = {Q: timed(lambda: pq.search(qs[:Q], k)) for Q in a.queries}
        rec[f"pq_recall_at_{k}"] = round(recall(pq.search(qs, k)[1], ref), 4)
        res = IVFPQIndex(D, a.nlist, M, nprobe=1, by_residual=True, capacity=N)
        rec["train_s"] = round(wall(lambda: res.train(x)), 3)
        rec["add_s"] = round(wall(lambda: add_all(res, x)), 3)
        rec["rebuild_s"] = round(wall(res._finalize), 3)
        plain = IVFPQIndex(D, a.nlist, M, nprobe=1, by_residual=False, capacity=N)
        plain.train(x)
        add_all(plain, x)
        refine = RefineFlatIndex(res, flat, k_factor=a.k_factor)
        lut = torch.empty(Qmax * M * 256, dtype=torch.float32, device=dev)
        rec["configs"] = []
        for Q in a.queries:
            q = qs[:Q]
            lut_ms = timed(lambda: _lib.check(lib.lrx_pq_lut(_lib.ptr(q), Q, _lib.ptr(res.pq.centroids), D, M, _lib.ptr(lut), _lib.current_stream())))
            for nprobe in a.nprobes:
                if nprobe > a.nlist:
                    continue
                res.nprobe = nprobe
                ms = timed(lambda: res.search(q, k))
                coarse_ms = timed(lambda: res.quantizer.search(q, nprobe))
                plain_ms = timed(lambda: plain.search(q, k, nprobe=nprobe))
                c = {"Q": Q, "nprobe": nprobe, "ms": round(ms, 4), "coarse_ms": round(coarse_ms, 4), "lut_ms": round(lut_ms, 4),
                     "ms_no_residual": round(plain_ms, 4), "pq_ms": round(pq_ms[Q], 4), "ivf_flat_ms": round(ivf_ms[(Q, nprobe)], 4),
                     "flat_ms": round(flat_ms[Q], 4), "max_scan_rows": res.max_scan_rows(nprobe),
                     f"recall_at_{k}": round(recall(res.search(q, k)[1], ref[:Q]), 4),
                     f"recall_at_{k}_no_residual": round(recall(plain.search(q, k, nprobe=nprobe)[1], ref[:Q]), 4)}
                if int(k * a.k_factor) <= 2048:
                    c[f"refine_recall_at_{k}"] = round(recall(refine.search(q, k)[1], ref[:Q]), 4)
                    c["refine_ms"] = round(timed(lambda: refine.search(q, k)), 4)
                rec["configs"].append(c)
            print(f"M={M} Q={Q} done", file=sys.stderr, flush=True)
        rec["pq_ms"] = {str(Q): round(v, 4) for Q, v in pq_ms.items()}
        out["per_M"].append(rec)
        del pq, res, plain, refine, lut
    out["flat_ms"] = {str(Q): round(v, 4) for Q, v in flat_ms.items()}
    out["flat_ms_again"] = {str(Q): round(timed(lambda: flat.search(qs[:Q], k)), 4) for Q in a.queries}     # (A-B-A: drift shows as a difference)
    out["device_errors"] = int(lib.lrx_device_error_count(0))
    print(json.dumps(out), flush=True)
