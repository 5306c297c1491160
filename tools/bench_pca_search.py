#!/usr/bin/env python3
"""PreTransformIndex(PCAMatrix(2048 -> 256), FlatIPIndex(256)) against FlatIPIndex(2048), same process, same rows: JSON lines for a planted-
spectrum corpus of N x 2048 (default 1M; 256 directions of scale 4 .. 2, the others 0.5 .. 0.05, a rotated basis, a mean of 0.3 N(0, 1)),
Q = 100, k = 100 --
  transform   lrx_linear_transform over the whole corpus: ms, TFLOP/s and its share of the 157 TFLOP/s f32-MFMA spec peak
  train       PCAMatrix.train over the corpus (Gram chunks on the GPU, eigh on the host), one run
  add         PreTransformIndex.add (transform into the base's slot) / FlatIPIndex(256).add of already reduced rows / FlatIPIndex(2048).add
  search      the two indexes, A-B-A
  overlap     overlap@100 of the two result lists
CUDA events, medians after warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lightretriever_amd import FlatIPIndex, PCAMatrix, PreTransformIndex

SPEC_PEAK_TF = 157.0


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


def planted(n, d, top, seed, chunk=65536):
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = torch.cat([torch.linspace(4.0, 2.0, top), torch.linspace(0.5, 0.05, d - top)]).cuda()
    basis = torch.linalg.qr(torch.randn(d, d, device="cuda", generator=g))[0]
    mean = 0.3 * torch.randn(d, device="cuda", generator=g)
    x = torch.empty(n, d, device="cuda")
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        x[s:e] = (torch.randn(e - s, d, device="cuda", generator=g) * scale) @ basis.T + mean
    return x


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d-in", type=int, default=2048)
    ap.add_argument("--d-out", type=int, default=256)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    N, D, d, Q, k = a.rows, a.d_in, a.d_out, a.queries, a.k
    print(json.dumps({"device": torch.cuda.get_device_name(0), "shape": f"{N}x{D}->{d}", "Q": Q, "k": k}), flush=True)
    allrows = planted(N + Q, D, d, 0)
    x, q = allrows[:N], allrows[N:].contiguous()

    pca = PCAMatrix(D, d)
    t0 = time.time()
    pca.train(x)
    torch.cuda.synchronize()
    print(json.dumps({"train_s": round(time.time() - t0, 2), "rows_used": min(N, pca.max_points_per_d * D),
                      "eigenvalue_0": round(float(pca.eigenvalues[0]), 3), "eigenvalue_d_out": round(float(pca.eigenvalues[d - 1]), 3),
                      "eigenvalue_next": round(float(pca.eigenvalues[d]), 3)}), flush=True)

    y = torch.empty(N, d, device="cuda")
    ms = timed(lambda: pca.apply_into(x, y), a.reps)
    tf = 2.0 * N * D * d / ms / 1e9
    print(json.dumps({"transform_ms": round(ms, 3), "transform_tflops": round(tf, 1), "share_of_spec_peak": round(tf / SPEC_PEAK_TF, 3),
                      "x_read_gbps": round(N * D * 4 / ms / 1e6)}), flush=True)
    msq = timed(lambda: pca.apply(q), a.reps)
    print(json.dumps({"transform_queries_ms": round(msq, 4)}), flush=True)

    pre = PreTransformIndex(pca, FlatIPIndex(d, capacity=N))
    small = FlatIPIndex(d, capacity=N)
    big = FlatIPIndex(D, capacity=N)

    def add(idx, rows):
        idx.reset()
        idx.add(rows)
    t_pre, t_small, t_big = timed(lambda: add(pre, x), 5), timed(lambda: add(small, y), 5), timed(lambda: add(big, x), 5)
    print(json.dumps({"add_ms_pre_transform": round(t_pre, 2), "add_ms_flat_reduced_rows": round(t_small, 2), "add_ms_flat_full": round(t_big, 2),
                      "resident_gb_pre_transform": round(N * d * 6 / 1e9, 2), "resident_gb_flat_full": round(N * D * 6 / 1e9, 2)}), flush=True)

    s_pre = timed(lambda: pre.search(q, k), a.reps)
    s_big = timed(lambda: big.search(q, k), a.reps)
    s_pre2 = timed(lambda: pre.search(q, k), a.reps)               # (A-B-A: drift shows as ms_pre_transform != ms_pre_transform_again)
    Ip, Ib = pre.search(q, k)[1].cpu().numpy(), big.search(q, k)[1].cpu().numpy()
    overlap = sum(len(set(Ip[i]) & set(Ib[i])) for i in range(Q)) / (Q * k)
    print(json.dumps({"search_ms_pre_transform": round(s_pre, 4), "search_ms_flat_full": round(s_big, 4), "search_ms_pre_transform_again": round(s_pre2, 4),
                      "pre_transform_over_flat": round(min(s_pre, s_pre2) / s_big, 3), f"overlap_at_{k}": round(overlap, 4)}), flush=True)
