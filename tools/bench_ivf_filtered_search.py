#!/usr/bin/env python3
"""Row-selector filtered search of the four inverted-file indexes, same process, same rows: ONE JSON line for the clustered
corpus of DESIGN §5.4 (N x 2048 unit rows in 1000 clusters, default 1M; queries drawn near corpus rows), nlist = 1024, k = 100.  Per family
(flat, sq_fp16, sq8, pq), (Q, nprobe) in {1, 100, 1000} x {8, 32}, selectivity in {1.0, 0.5, 0.1, 0.01} and selection pattern -- `rows`
drawn at random, or whole `cells` (cells drawn at random until they hold that share of the rows) --
  ms             search(q, k, nprobe, sel=selector)
  unfiltered_ms  search(q, k, nprobe) in the same run (once per (Q, nprobe), taken before and after its selectivities: A-B-A)
  workaround_ms  what a caller did before: range_search_probed(q, -inf, nprobe), the mask on the hits, a dense top-k over what is left
  staged_share   the share of the probed cells' row groups that hold a selected row (what the cell-major scans still read)
and the time to build a selector from a mask and from row numbers.  --unfiltered-only times the unfiltered searches alone (no selector is
made: it runs on a build without one, which is how the cost of the feature to a search without a selector is measured against its parent).
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

import lightretriever_amd as A
from lightretriever_amd import _lib
from lightretriever_amd.synth import clustered_corpus

FLT_MAX = float(np.finfo(np.float32).max)
INF = float("inf")


def timed(fn, budget_ms=200.0):
    """Median event ms of fn after two warm-up calls, over 3 .. 20 calls that take about budget_ms."""
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
        if len(ts) >= max(3, min(20, int(budget_ms / max(ts[0], 1e-3)))):
            return statistics.median(ts)


def make(fam, d, nlist, M, N):
    if fam == "flat":
        return A.IVFFlatIndex(d, nlist, capacity=N)
    if fam == "sq_fp16":
        return A.IVFSQIndex(d, nlist, capacity=N)
    if fam == "sq8":
        return A.IVFSQ8Index(d, nlist, capacity=N)
    return A.IVFPQIndex(d, nlist, M, capacity=N)


def group_rows(fam, d):
    lib = _lib.lib()
    return {"flat": max(1, min(128, 16384 // d)), "sq_fp16": lib.lrx_ivf_sq_fp16_group_rows(d), "sq8": lib.lrx_ivf_sq8_group_rows(d), "pq": None}[fam]


def masks(idx, N, share, rng):
    """pattern -> bool [N] on the device over the ORIGINAL rows."""
    if share >= 1.0:
        full = torch.ones(N, dtype=torch.bool, device=idx.device)
        return {"rows": full, "cells": full}
    rows = torch.from_numpy(rng.random(N) < share).to(idx.device)
    order, chosen, held = rng.permutation(idx.nlist), [], 0
    for c in order:                                                          # whole cells until they hold the share
        if held >= share * N:
            break
        chosen.append(c)
        held += int(idx.list_sizes[c])
    cells = torch.isin(idx._assign[:N], torch.from_numpy(np.array(chosen, np.int64)).to(idx.device))
    return {"rows": rows, "cells": cells}


def staged_share(idx, probes, mask, G):
    """Of the row groups of the cells `probes` names, the share that holds a selected row."""
    if G is None:
        return None
    off = idx.list_off.cpu().numpy()
    sel_pos = mask[idx.row_ids].cpu().numpy()                                # by stored position
    groups = hit = 0
    for c in np.unique(probes[probes >= 0]):
        seg = sel_pos[off[c]:off[c + 1]]
        if len(seg):
            pad = np.zeros(-(-len(seg) // G) * G, bool)
            pad[:len(seg)] = seg
            per = pad.reshape(-1, G).any(axis=1)
            groups += len(per)
            hit += int(per.sum())
    return round(hit / max(groups, 1), 4)


def workaround(idx, q, k, nprobe, mask):
    """The caller's own filter over range_search_probed(q, -inf): every scanned pair is materialised, masked, and cut to the top k."""
    lims, D, I = idx.range_search_probed(q, -INF, nprobe)
    Q = q.shape[0]
    counts = lims[1:] - lims[:-1]
    width = max(int(counts.max()), 1)
    seg = torch.repeat_interleave(torch.arange(Q, device=q.device), counts)
    pos = torch.arange(D.numel(), device=q.device) - lims[:-1][seg]
    keep = mask[I]
    dense = torch.full((Q, width), -FLT_MAX, device=q.device)
    ids = torch.full((Q, width), -1, dtype=torch.int64, device=q.device)
    dense[seg, pos] = torch.where(keep, D, torch.full_like(D, -FLT_MAX))
    ids[seg, pos] = torch.where(keep, I, torch.full_like(I, -1))
    top = torch.topk(dense, min(k, width), dim=1)
    return top.values, ids.gather(1, top.indices)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--pq-m", type=int, default=64)
    ap.add_argument("--families", nargs="+", default=["flat", "sq_fp16", "sq8", "pq"])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--nprobes", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--selectivities", type=float, nargs="+", default=[1.0, 0.5, 0.1, 0.01])
    ap.add_argument("--niter", type=int, default=None, help="k-means iterations of the training (default: the classes' own)")
    ap.add_argument("--budget-ms", type=float, default=200.0)
    ap.add_argument("--unfiltered-only", action="store_true")
    ap.add_argument("--no-workaround", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N, D, k = a.rows, a.d, a.k
    out = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{D}", "nlist": a.nlist, "k": k, "corpus": "1000 clusters, intra_cos 0.9, unit rows",
           "unfiltered_only": bool(a.unfiltered_only), "families": {}}
    x = torch.empty(N, D, dtype=torch.float32, device=dev)
    clustered_corpus(x, n_clusters=1000, intra_cos=0.9, dup_frac=0.01, seed=5)
    Qmax = max(a.queries)
    g = torch.Generator(device=dev).manual_seed(1)
    near = x[torch.randint(0, N, (Qmax,), generator=g, device=dev)]
    u = torch.nn.functional.normalize(torch.randn(Qmax, D, generator=g, device=dev), dim=-1)
    qs = torch.nn.functional.normalize(math.sqrt(0.9) * near + math.sqrt(0.1) * u, dim=-1).contiguous()
    del near, u
    T = lambda fn: round(timed(fn, a.budget_ms), 4)

    if not a.unfiltered_only:
        rng = np.random.default_rng(0)
        m = torch.from_numpy(rng.random(N) < 0.1).to(dev)
        r = torch.nonzero(m)[:, 0].contiguous()
        sel = A.RowSelector(N)
        out["selector_ms"] = {"from_mask": T(lambda: sel.set_mask_(m)), "from_rows_10pct": T(lambda: sel.set_rows_(r)), "invert": T(sel.invert)}

    for fam in a.families:
        print(f"[bench_ivf_filtered_search] {fam}: train + add", file=sys.stderr, flush=True)
        idx = make(fam, D, a.nlist, a.pq_m, N)
        idx.train(x, niter=a.niter)
        for s in range(0, N, 262144):
            idx.add(x[s:s + 262144])
        idx._finalize()
        G = group_rows(fam, D)
        res = {"group_rows": G, "configs": []}
        rng = np.random.default_rng(7)
        all_masks = None if a.unfiltered_only else {s: masks(idx, N, s, rng) for s in a.selectivities}
        for Q in a.queries:
            q = qs[:Q]
            for nprobe in a.nprobes:
                print(f"[bench_ivf_filtered_search] {fam}: Q={Q} nprobe={nprobe}", file=sys.stderr, flush=True)
                cfg = {"Q": Q, "nprobe": nprobe, "unfiltered_ms": T(lambda: idx.search(q, k, nprobe=nprobe)), "max_scan_rows": idx.max_scan_rows(nprobe)}
                if not a.unfiltered_only:
                    probes = idx.quantizer.search(q, nprobe)[1].cpu().numpy()
                    sel = A.RowSelector(N)
                    cfg["filtered"] = []
                    for share, by_pattern in all_masks.items():
                        for pattern, mask in by_pattern.items():
                            if share >= 1.0 and pattern == "cells":
                                continue                                     # (the same mask as `rows`)
                            sel.set_mask_(mask)
                            e = {"selectivity": share, "pattern": pattern, "selected": sel.count(), "ms": T(lambda: idx.search(q, k, nprobe=nprobe, sel=sel)),
                                 "staged_share": staged_share(idx, probes, mask, G)}
                            if not a.no_workaround:
                                e["workaround_ms"] = T(lambda: workaround(idx, q, k, nprobe, mask))
                            cfg["filtered"].append(e)
                    cfg["unfiltered_ms_again"] = T(lambda: idx.search(q, k, nprobe=nprobe))
                    for e in cfg["filtered"]:
                        e["vs_unfiltered"] = round(e["ms"] / cfg["unfiltered_ms"], 3)
                        if "workaround_ms" in e:
                            e["vs_workaround"] = round(e["ms"] / e["workaround_ms"], 3)
                res["configs"].append(cfg)
        out["families"][fam] = res
        del idx
        torch.cuda.empty_cache()
    out["device_errors"] = int(_lib.lib().lrx_device_error_count(0))
    print(json.dumps(out), flush=True)
