#!/usr/bin/env python3
"""RefineFlatIndex against FlatIPIndex, same process, same rows: ONE JSON line for the planted-spectrum corpus of tools/bench_pca_search.py
(N x 2048, default 1M), Q = 100, k = 100.  Two bases -- PreTransformIndex(PCAMatrix(2048 -> 256), FlatIPIndex(256)) and PQIndex(2048, 128) --
each at k_factor 1, 4 and 10; per configuration
  base_ms      base.search(q, k_base), k_base = int(k * k_factor)
  rerank_ms    the rerank entry point over those candidates (and the bytes of the gathered fp32 rows over that time)
  total_ms     RefineFlatIndex.search(q, k, k_factor): the two stages as the index runs them
  recall       recall@k against FlatIPIndex.search (and the base's own, without the rerank)
and the flat search's own time, taken before and after the rest (A-B-A).  The refine store is the flat index itself (its fp32 rows; the
shadow is not touched by the rerank), so both sides read the same memory.  CUDA events, medians after warm-up."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_pca_search import planted, timed
from lightretriever_amd import FlatIPIndex, PCAMatrix, PQIndex, PreTransformIndex, RefineFlatIndex
from lightretriever_amd.refine import k_base_of, rerank


def recall(I: torch.Tensor, ref: torch.Tensor) -> float:
    I, ref = I.cpu().numpy(), ref.cpu().numpy()
    return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(I, ref)) / ref.size


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--d-pca", type=int, default=256)
    ap.add_argument("--pq-m", type=int, default=128)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--k-factors", type=float, nargs="+", default=[1, 4, 10])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    N, D, Q, k = a.rows, a.d, a.queries, a.k
    allrows = planted(N + Q, D, a.d_pca, 0)
    x, q = allrows[:N], allrows[N:].contiguous()

    flat = FlatIPIndex(D, capacity=N)
    flat.add(x)
    flat_ms = timed(lambda: flat.search(q, k), a.reps)
    ref = flat.search(q, k)[1]

    bases = {f"pca{a.d_pca}_flat": PreTransformIndex(PCAMatrix(D, a.d_pca), FlatIPIndex(a.d_pca, capacity=N)), f"pq{a.pq_m}": PQIndex(D, a.pq_m, capacity=N)}
    out = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{D}", "Q": Q, "k": k, "reps": a.reps, "store": "fp32 rows of the flat index",
           "configs": []}
    for name, base in bases.items():
        base.train(x)
        for s in range(0, N, 262144):
            base.add(x[s:s + 262144])
        idx = RefineFlatIndex(base, flat)
        for kf in a.k_factors:
            kb = k_base_of(k, kf)
            cand = base.search(q, kb)[1].clone()
            valid = int(((cand >= 0) & (cand < N)).sum())
            base_ms = timed(lambda: base.search(q, kb), a.reps)
            rerank_ms = timed(lambda: rerank(q, flat, cand, k, ws_slots=vars(idx)), a.reps)
            total_ms = timed(lambda: idx.search(q, k, k_factor=kf), a.reps)
            out["configs"].append({"base": name, "k_factor": kf, "k_base": kb, "base_ms": round(base_ms, 4), "rerank_ms": round(rerank_ms, 4),
                                   "total_ms": round(total_ms, 4), "rerank_rows": valid, "rerank_gather_tbps": round(valid * D * 4 / rerank_ms / 1e9, 2),
                                   f"recall_at_{k}": round(recall(idx.search(q, k, k_factor=kf)[1], ref), 4),
                                   f"base_recall_at_{k}": round(recall(base.search(q, k)[1], ref), 4)})
        del idx, base
    out["flat_ms"] = round(flat_ms, 4)
    out["flat_ms_again"] = round(timed(lambda: flat.search(q, k), a.reps), 4)     # (A-B-A: drift shows as flat_ms != flat_ms_again)
    out["resident_gb"] = {"flat_with_shadow": round(N * D * 6 / 1e9, 2), "refine_store_fp32": round(N * D * 4 / 1e9, 2), "refine_store_fp16": round(N * D * 2 / 1e9, 2),
                          f"pca{a.d_pca}_flat": round(N * a.d_pca * 6 / 1e9, 2), f"pq{a.pq_m}": round(N * a.pq_m / 1e9, 3)}
    print(json.dumps(out), flush=True)
