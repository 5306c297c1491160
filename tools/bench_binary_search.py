#!/usr/bin/env python3
"""BinaryFlatIndex (IndexBinaryFlat + float rerank) beside FlatIPIndex and SQFp16Index on the same rows, same process: one JSON line per
(shape, Q, k) -- 1M x 2048 and 10M x 2048, Q in {1, 100, 1000}, k in {100, 1000}, binary_k = 1000.  CUDA events, medians after warm-up, order
binary / flat / sq / binary again.  The binary search is timed whole and up to the end of the candidate selection (LRX_BINARY_SELECT_ONLY:
pack + three scans + cutoff + prefix); the rerank is the difference.  Resident bytes of the three indexes, and recall@10 / recall@100 of
binary + rerank against the flat index's exact hits -- a property of the method on this clustered synthetic corpus, for information."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lightretriever_amd import BinaryFlatIndex, FlatIPIndex, SQFp16Index, _lib

N_CLUSTERS = 4096


def centres(D):
    return torch.randn(N_CLUSTERS, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))


def chunks(N, D, cen, seed, chunk=1 << 18):
    """Clustered rows: a centre plus Gaussian noise of the same norm, normalised."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s in range(0, N, chunk):
        n = min(chunk, N - s)
        c = cen[torch.randint(0, N_CLUSTERS, (n,), device="cuda", generator=g)]
        yield torch.nn.functional.normalize(c + torch.randn(n, D, generator=g, device="cuda"), dim=-1)


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


def recall(I_got, I_want, k):
    hit = (I_got[:, :k, None] == I_want[:, None, :k]).any(dim=2).float().sum(dim=1)
    return float((hit / k).mean())


def run(N, D, reps, qs, ks, binary_k, with_sq):
    cen = centres(D)
    binary = BinaryFlatIndex(D, capacity=N)
    flat = FlatIPIndex(D, capacity=N)
    sq = SQFp16Index(D, capacity=N) if with_sq else None
    for x in chunks(N, D, cen, 0):
        binary.add(x)
        flat.add(x)
        if sq is not None:
            sq.add(x)
    torch.cuda.synchronize()
    res = {"resident_gb_binary": round(binary._codes.numel() / 1e9, 4), "resident_gb_flat": round((flat._x.numel() * 4 + flat._xb.numel() * 2) / 1e9, 3),
           "resident_gb_sq": round(sq._xb.numel() * 2 / 1e9, 3) if sq is not None else None}
    for Q in qs:
        q = next(chunks(Q, D, cen, 1, chunk=Q))                 # queries drawn like the rows
        for k in ks:
            bk = max(binary_k, k)
            t_bin = timed(lambda: binary.search(q, k, binary_k=bk), reps)
            t_sel = timed(lambda: binary.search(q, k, binary_k=bk, flags=_lib.BINARY_SELECT_ONLY), reps)
            t_flat = timed(lambda: flat.search(q, k), reps)
            t_sq = timed(lambda: sq.search(q, k), reps) if sq is not None else None
            t_bin2 = timed(lambda: binary.search(q, k, binary_k=bk), reps)
            I_b, I_f = binary.search(q, k, binary_k=bk)[1], flat.search(q, k)[1]
            line = {"shape": f"{N}x{D}", "Q": Q, "k": k, "binary_k": bk, "ms_binary": round(t_bin, 4), "ms_binary_scan_select": round(t_sel, 4),
                    "ms_binary_rerank": round(t_bin - t_sel, 4), "ms_flat": round(t_flat, 4), "ms_sq": None if t_sq is None else round(t_sq, 4),
                    "ms_binary_again": round(t_bin2, 4), "binary_over_flat": round(min(t_bin, t_bin2) / t_flat, 4),
                    "code_gb_per_s_one_pass": round(binary.ntotal * binary.Mp / 1e9 / (t_sel / 1e3), 1),
                    "recall_at_10": round(recall(I_b, I_f, 10), 4), "recall_at_100": round(recall(I_b, I_f, min(100, k)), 4), **res}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=str, default="1000000,10000000")
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--queries", type=str, default="1,100,1000")
    ap.add_argument("--k", type=str, default="100,1000")
    ap.add_argument("--binary-k", type=int, default=1000)
    ap.add_argument("--no-sq", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for N in [int(v) for v in a.rows.split(",")]:
        run(N, a.dim, a.reps, [int(v) for v in a.queries.split(",")], [int(v) for v in a.k.split(",")], a.binary_k, not a.no_sq)
        torch.cuda.empty_cache()
