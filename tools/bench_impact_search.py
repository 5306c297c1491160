#!/usr/bin/env python3
"""ImpactIndex.search against torch.sparse on the same GPU, same process: one JSON line per leg.  Synthetic corpus: 1M documents x (about)
128 distinct terms drawn Zipf-like (P(rank) ~ 1 / rank) from a 128 k vocabulary, weights 1 .. 255.  Queries: `tok`-like (16 terms, counts
1 .. 3) and `spr`-like (64 terms, counts 100 .. 400), terms drawn like the documents'; Q in {1, 100, 1000} x k in {100, 1000}.  Baseline:
the documents as a torch sparse CSR matrix [N, V] times the dense queries [V, Q] (the product [Q, V] @ [V, N], transposed) followed by
torch.topk -- fp32, so exact for these scores (< 2^24).  `postings_per_s` counts the postings of the queries' terms (what a
term-at-a-time scan must read) over the whole search time; `floor_ms` is that many 8-byte postings at the stream-read ceiling of the same
run (the fastest read leg of tools/bench_hbm.py).  Also: the build (add + finalize) time, and --windows: the same legs with the scan's
window forced to 2048 / 8192 / 32768 rows next to the library's rule.  CUDA events, medians after warm-up."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from lightretriever_amd import ImpactIndex
from lightretriever_amd.impact_index import query_csr


def zipf_terms(shape, V, g):
    return torch.exp(torch.rand(shape, device="cuda", generator=g) * math.log(V)).long().clamp_(1, V) - 1


def corpus(N, V, nnz, seed=0, chunk=65536):
    """Per chunk of documents: (terms, weights, offsets) on the device, a term at most once per document."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s in range(0, N, chunk):
        n = min(chunk, N - s)
        key = torch.unique(torch.arange(n, device="cuda")[:, None] * V + zipf_terms((n, nnz), V, g))      # sorted by (document, term)
        doc, terms = key // V, key % V
        weights = torch.randint(1, 256, terms.shape, device="cuda", generator=g)
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        off[1:] = torch.cumsum(torch.bincount(doc, minlength=n), 0)
        yield terms, weights, off


def make_queries(Q, V, kind, seed=1):
    rng = np.random.default_rng(seed)
    nt, lo, hi = (16, 1, 4) if kind == "tok" else (64, 100, 401)
    out = []
    for _ in range(Q):
        t = np.unique(np.minimum(np.exp(rng.random(2 * nt) * math.log(V)).astype(np.int64), V) - 1)
        t = rng.permutation(t)[:nt]
        out.append((t, rng.integers(lo, hi, t.size)))
    return out


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


def stream_ceiling():
    import bench_hbm
    legs = bench_hbm.legs()
    best = max((n for n in legs if "copy" not in n), key=lambda n: legs[n][1])
    return {"stream_read_ceiling_leg": best, "stream_read_ceiling_gbps": round(legs[best][1])}


def build(N, V, nnz):
    parts = list(corpus(N, V, nnz))
    idx = ImpactIndex()

    def run():
        idx.reset()
        for p in parts:
            idx.add(*p)
        idx.finalize()
    ms = timed(run, 3)
    return idx, {"rows": N, "vocab": V, "nnz": idx.nnz, "build_ms": round(ms, 1), "resident_gb": round(idx.nnz * 8 / 1e9, 3)}


def sparse_baseline(idx, V):
    """The documents as a torch sparse CSR [N, V] fp32 matrix (rows = documents), from the index's own postings."""
    rows, w = idx._postings[:, 0].long(), idx._postings[:, 1].float()
    terms = torch.repeat_interleave(torch.arange(idx.n_terms, device="cuda"), idx._term_off[1:] - idx._term_off[:-1])
    order = torch.argsort(rows * V + terms)
    crow = torch.zeros(idx.ntotal + 1, dtype=torch.int64, device="cuda")
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=idx.ntotal), 0)
    return torch.sparse_csr_tensor(crow, terms[order], w[order], size=(idx.ntotal, V))


def leg(idx, docs_csr, V, Q, k, kind, reps, ceiling_gbps, window=0, baseline=True):
    queries = make_queries(Q, V, kind)
    csr = query_csr(queries)
    idx.window_rows = window
    ms = timed(lambda: idx.search(*csr, k), reps)
    idx.window_rows = 0
    df = np.diff(idx.term_off_host)
    touched = int(sum(df[t[t < idx.n_terms]].sum() for t, _ in queries))
    out = {"kind": kind, "Q": Q, "k": k, "window_rows": window, "ms_impact": round(ms, 4), "postings": touched,
           "postings_per_s": round(touched / ms * 1e3), "floor_ms": round(touched * 8 / ceiling_gbps / 1e6, 4) if ceiling_gbps else None}
    if baseline:
        qd = torch.zeros(V, Q, device="cuda")
        for i, (t, c) in enumerate(queries):
            qd[torch.from_numpy(t).cuda(), i] = torch.from_numpy(c).float().cuda()
        try:
            fn = lambda: torch.topk(torch.sparse.mm(docs_csr, qd).t(), k, dim=1)
            tb = timed(fn, max(2, reps // 4))
            D, I = idx.search(*csr, k)
            Db = fn()[0]
            out.update({"ms_torch_sparse": round(tb, 4), "impact_over_torch": round(ms / tb, 4),
                        "scores_equal": bool(torch.equal(torch.where(I >= 0, D, torch.zeros_like(D)), Db))})
        except Exception as e:                                    # (the baseline is a yardstick of this tool, not a path of the package)
            out["torch_sparse_error"] = repr(e)[:200]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=131072)
    ap.add_argument("--nnz", type=int, default=128)
    ap.add_argument("--one-leg", action="store_true", help="tok-like, Q = 100, k = 100 on ImpactIndex only (the profiled leg)")
    ap.add_argument("--windows", action="store_true", help="also time the legs with the window forced to 2048 / 8192 / 32768 rows")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    if a.one_leg:
        idx, info = build(a.rows, a.vocab, a.nnz)
        leg(idx, None, a.vocab, 100, 100, "tok", a.reps, 0, baseline=False)
        sys.exit(0)
    ceiling = stream_ceiling()
    print(json.dumps(ceiling), flush=True)
    torch.cuda.empty_cache()
    idx, info = build(a.rows, a.vocab, a.nnz)
    print(json.dumps(info), flush=True)
    docs_csr = sparse_baseline(idx, a.vocab)
    for kind in ("tok", "spr"):
        for Q in (1, 100, 1000):
            for k in (100, 1000):
                leg(idx, docs_csr, a.vocab, Q, k, kind, a.reps, ceiling["stream_read_ceiling_gbps"])
    if a.windows:
        for kind in ("tok", "spr"):
            for Q in (1, 100, 1000):
                for W in (2048, 8192, 32768):
                    leg(idx, None, a.vocab, Q, 100, kind, a.reps, ceiling["stream_read_ceiling_gbps"], window=W, baseline=False)
