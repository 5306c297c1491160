#!/usr/bin/env python3
"""IVFSQ8Index against IVFFlatIndex, IVFSQIndex, SQ8Index and FlatIPIndex, same process, same rows: ONE JSON line for the clustered corpus of
DESIGN §5.4 (N x 2048 unit rows in 1000 clusters, default 1M; queries drawn near corpus rows), nlist = 1024, k = 100, QT_8bit.  Per (Q, nprobe)
in {1, 16, 100, 1000} x {1, 8, 32, 128}
  ms               IVFSQ8Index.search(q, k, nprobe), by_residual: the coarse search and the scan, as the index runs them; coarse_ms: the coarse
                   search alone; ms_no_residual: the same call on an index built with by_residual=False
  ivf_flat_ms      IVFFlatIndex.search and
  ivf_sq_fp16_ms   IVFSQIndex.search (by_residual) on the same cells, queries and nprobe -- unchanged code: the two yardsticks for time
  scan_ms          the library call alone (ops.ivf_sq8_ip_topk over probe lists and scores made beforehand: plan, scan, selection), with and
                   without residuals, beside ivf_flat_scan_ms and ivf_sq_fp16_scan_ms over the same probe lists
  recall           recall@k against FlatIPIndex.search, for both by_residual values, beside IVFFlatIndex's and IVFSQIndex's on the same probes
next to FlatIPIndex.search's own ms per Q (taken before and after the rest: A-B-A; the relative difference of the two flat measurements is the
run's spread), SQ8Index's recall, the resident GB of the indexes, the train / add / rebuild times and the device error count.  The inverted
files share one training (the same centroid bits), so their cells are the same (`same_cells`).  HIP events, medians after warm-up."""
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

from lightretriever_amd import FlatIPIndex, IVFFlatIndex, IVFSQ8Index, IVFSQIndex, SQ8Index, _lib, ops
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
    ap.add_argument("--qtype", default="QT_8bit")
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 100, 1000])
    ap.add_argument("--nprobes", type=int, nargs="+", default=[1, 8, 32, 128])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N, D, k = a.rows, a.d, a.k
    out = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{D}", "nlist": a.nlist, "k": k, "qtype": a.qtype,
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

    flat_ms = {Q: timed(lambda: flat.search(qs[:Q], k)) for Q in a.queries}
    ref = flat.search(qs, k)[1].clone()
    sq8 = SQ8Index(D, a.qtype, capacity=N)
    sq8.train(x)
    add_all(sq8, x)
    out[f"sq8_recall_at_{k}"] = round(recall(sq8.search(qs, k)[1], ref), 4)
    del sq8

    ivf = IVFFlatIndex(D, a.nlist, nprobe=1, capacity=N)
    out["ivf_flat_train_s"] = round(wall(lambda: ivf.train(x)), 3)
    out["ivf_flat_add_s"] = round(wall(lambda: add_all(ivf, x)), 3)
    out["ivf_flat_rebuild_s"] = round(wall(ivf._finalize), 3)
    h16 = IVFSQIndex(D, a.nlist, nprobe=1, by_residual=True, capacity=N)
    h16.set_contents(ivf.centroids, torch.zeros(0, D, dtype=torch.float16), np.zeros(a.nlist + 1, np.int64), np.zeros(0, np.int64))   # the same training
    add_all(h16, x)
    h16._finalize()
    res = IVFSQ8Index(D, a.nlist, a.qtype, nprobe=1, by_residual=True, capacity=N)
    out["train_s"] = round(wall(lambda: res.train(x)), 3)
    out["add_s"] = round(wall(lambda: add_all(res, x)), 3)
    out["rebuild_s"] = round(wall(res._finalize), 3)
    plain = IVFSQ8Index(D, a.nlist, a.qtype, nprobe=1, by_residual=False, capacity=N)
    out["train_s_no_residual"] = round(wall(lambda: plain.train(x)), 3)
    out["add_s_no_residual"] = round(wall(lambda: add_all(plain, x)), 3)
    out["rebuild_s_no_residual"] = round(wall(plain._finalize), 3)
    out["same_cells"] = bool(torch.equal(res.centroids, ivf.centroids) and torch.equal(plain.centroids, ivf.centroids) and torch.equal(res.row_ids, ivf.row_ids) and
                             torch.equal(plain.row_ids, ivf.row_ids) and torch.equal(h16.row_ids, ivf.row_ids))
    sizes = res.list_sizes
    out["cells"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}

    out["configs"] = []
    for Q in a.queries:
        q = qs[:Q]
        for nprobe in a.nprobes:
            if nprobe > a.nlist:
                continue
            probes = res.quantizer.search(q, nprobe)[1].cpu().numpy()
            once = int(sizes[np.unique(probes)].sum())
            ms = timed(lambda: res.search(q, k, nprobe=nprobe))
            ivf_ms = timed(lambda: ivf.search(q, k, nprobe=nprobe))
            h16_ms = timed(lambda: h16.search(q, k, nprobe=nprobe))
            ms_plain = timed(lambda: plain.search(q, k, nprobe=nprobe))
            coarse_ms = timed(lambda: res.quantizer.search(q, nprobe))
            ivf_coarse_ms = timed(lambda: ivf.quantizer.search(q, nprobe))
            # the scans alone, over the probe lists and scores of one coarse search made beforehand
            ps, pr = res.quantizer.search(q, nprobe)
            scan_rows = res.max_scan_rows(nprobe)
            scan_ms = timed(lambda: ops.ivf_sq8_ip_topk(q, res.stored_codes(), res.trained, res._qt, res.list_off, res.row_ids, pr, ps, True, k, scan_rows,
                                                        ws_slots=vars(res)))
            scan_ms_plain = timed(lambda: ops.ivf_sq8_ip_topk(q, plain.stored_codes(), plain.trained, plain._qt, plain.list_off, plain.row_ids, pr, None, False, k,
                                                              scan_rows, ws_slots=vars(plain)))
            ivf_scan_ms = timed(lambda: ops.ivf_flat_ip_topk(q, ivf.stored_rows(), ivf.list_off, ivf.row_ids, pr, k, scan_rows, ws_slots=vars(ivf)))
            h16_scan_ms = timed(lambda: ops.ivf_sq_fp16_ip_topk(q, h16.stored_codes(), h16.list_off, h16.row_ids, pr, ps, True, k, scan_rows, ws_slots=vars(h16)))
            out["configs"].append({"Q": Q, "nprobe": nprobe, "ms": round(ms, 4), "ms_no_residual": round(ms_plain, 4), "ivf_flat_ms": round(ivf_ms, 4),
                                   "ivf_sq_fp16_ms": round(h16_ms, 4), "coarse_ms": round(coarse_ms, 4), "ivf_flat_coarse_ms": round(ivf_coarse_ms, 4),
                                   "scan_ms": round(scan_ms, 4), "scan_ms_no_residual": round(scan_ms_plain, 4), "ivf_flat_scan_ms": round(ivf_scan_ms, 4),
                                   "ivf_sq_fp16_scan_ms": round(h16_scan_ms, 4), "flat_ms": round(flat_ms[Q], 4),
                                   f"recall_at_{k}": round(recall(res.search(q, k, nprobe=nprobe)[1], ref[:Q]), 4),
                                   f"recall_at_{k}_no_residual": round(recall(plain.search(q, k, nprobe=nprobe)[1], ref[:Q]), 4),
                                   f"ivf_flat_recall_at_{k}": round(recall(ivf.search(q, k, nprobe=nprobe)[1], ref[:Q]), 4),
                                   f"ivf_sq_fp16_recall_at_{k}": round(recall(h16.search(q, k, nprobe=nprobe)[1], ref[:Q]), 4),
                                   "max_scan_rows": scan_rows, "scanned_gb_cells_once": round(once * D / 1e9, 4),
                                   "gbps_cells_once": round(once * D / (ms * 1e-3) / 1e9, 1)})
    out["flat_ms"] = {str(Q): round(v, 4) for Q, v in flat_ms.items()}
    out["flat_ms_again"] = {str(Q): round(timed(lambda: flat.search(qs[:Q], k)), 4) for Q in a.queries}     # (A-B-A: drift shows as a difference)
    out["spread"] = {str(Q): round(abs(out["flat_ms_again"][str(Q)] - out["flat_ms"][str(Q)]) / out["flat_ms"][str(Q)], 4) for Q in a.queries}
    out["resident_gb"] = {"flat_with_shadow": round(N * D * 6 / 1e9, 2), "ivf_flat_rows": round(N * D * 4 / 1e9, 2), "ivf_sq_fp16_codes": round(N * D * 2 / 1e9, 2),
                          "sq8_codes": round(N * D / 1e9, 2), "ivf_sq8_codes": round(res.stored_codes().numel() / 1e9, 2),
                          "ivf_sq8_ids_and_cells": round(N * 16 / 1e9, 3), "ivf_sq8_trained": round(res.trained.numel() * 4 / 1e9, 6),
                          "centroids_with_shadow": round(a.nlist * D * 6 / 1e9, 4)}
    out["device_errors"] = int(_lib.lib().lrx_device_error_count(0))
    print(json.dumps(out), flush=True)
