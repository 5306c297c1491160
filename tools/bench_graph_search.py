#!/usr/bin/env python3
"""GraphFlatIndex against FlatIPIndex and IVFFlatIndex(nlist 1024, nprobe 32), same process, same rows: ONE JSON line per corpus of DESIGN
§5.4 (N x 2048 unit rows, default 1M) -- "isotropic" (iid Gaussian directions, iid queries) and "clustered" (1000 clusters with 1 % exact
duplicates; queries drawn near corpus rows) -- at k = 100.
  build_s       the graph build, split into kNN lists (flat searches) / detour counts (lrx_graph_detour_counts) / prune + reverse-edge merge
  per (Q, ef_search) in {1, 16, 100, 1000} x {64, 128, 256}
    ms          GraphFlatIndex.search(q, k, ef_search): the entry search and the traversal, as the index runs them (and the entry search alone)
    recall      recall@k against FlatIPIndex.search
    rows / steps  mean rows scored and steps per query (out_stats of lrx_graph_ip_search), and the GB/s the scored rows imply over ms
next to FlatIPIndex.search's own ms per Q (taken before and after the rest: A-B-A) and IVFFlatIndex.search's with its recall, and the read
rate lrx_probe_stream_read reaches in this run.  HIP events, medians after warm-up."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from lightretriever_amd import FlatIPIndex, GraphFlatIndex, IVFFlatIndex, _lib
from lightretriever_amd.synth import clustered_corpus
from bench_ivf_search import recall, stream_rate, timed, wall


def corpus_and_queries(kind: str, flat: FlatIPIndex, N: int, D: int, Qmax: int, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    slot = flat.append_slot(N)
    if kind == "clustered":
        clustered_corpus(slot, n_clusters=1000, intra_cos=0.9, dup_frac=0.01, seed=5)
        flat.commit(N)
        near = flat.vectors[torch.randint(0, N, (Qmax,), generator=g, device=dev)]
        u = torch.nn.functional.normalize(torch.randn(Qmax, D, generator=g, device=dev), dim=-1)
        return torch.nn.functional.normalize(math.sqrt(0.9) * near + math.sqrt(0.1) * u, dim=-1).contiguous()
    gx = torch.Generator(device=dev).manual_seed(0)
    for s in range(0, N, 65536):
        e = min(s + 65536, N)
        slot[s:e] = torch.nn.functional.normalize(torch.randn(e - s, D, generator=gx, device=dev), dim=-1)
    flat.commit(N)
    return torch.nn.functional.normalize(torch.randn(Qmax, D, generator=g, device=dev), dim=-1).contiguous()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=["isotropic", "clustered"], default="clustered")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--intermediate_degree", type=int, default=64)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--n_entry", type=int, default=None)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 100, 1000])
    ap.add_argument("--ef_search", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--no_ivf", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N, D, k = a.rows, a.d, a.k
    out = {"device": torch.cuda.get_device_name(0), "shape": f"{N}x{D}", "corpus": a.corpus, "k": k, "degree": a.degree,
           "intermediate_degree": a.intermediate_degree, "width": a.width}
    out["stream_read_gbps"] = round(stream_rate(dev), 1)

    flat = FlatIPIndex(D, capacity=N)
    qs = corpus_and_queries(a.corpus, flat, N, D, max(a.queries), dev)
    x = flat.vectors
    flat_ms = {Q: timed(lambda: flat.search(qs[:Q], k)) for Q in a.queries}
    ref = flat.search(qs, k)[1].clone()

    graph = GraphFlatIndex(D, degree=a.degree, intermediate_degree=a.intermediate_degree, search_width=a.width, n_entry=a.n_entry, capacity=N)
    for s in range(0, N, 262144):
        graph.add(x[s:s + 262144])
    out["build_s"] = {"total": round(wall(graph._finalize), 3), **{step: round(t, 3) for step, t in graph.build_times.items()}}
    out["n_entry"] = int(graph.entry_rows.numel())
    out["edges_per_row"] = round(float((graph.graph >= 0).sum()) / max(N, 1), 2)

    out["configs"] = []
    for Q in a.queries:
        q = qs[:Q]
        for ef in a.ef_search:
            beam = max(ef, k)
            ms = timed(lambda: graph.search(q, k, ef_search=ef))
            entry_ms = timed(lambda: graph._entries.search(q, min(beam, out["n_entry"], 2048)))
            _, I, S = graph._search(q, k, ef, None, True)
            S = S.float().mean(dim=0).tolist()
            out["configs"].append({"Q": Q, "ef_search": ef, "ms": round(ms, 4), "entry_ms": round(entry_ms, 4), "flat_ms": round(flat_ms[Q], 4),
                                   f"recall_at_{k}": round(recall(I, ref[:Q]), 4), "steps": round(S[0], 1), "rows_scored": round(S[1], 1),
                                   "gbps_rows_scored": round(S[1] * Q * D * 4 / (ms * 1e-3) / 1e9, 1)})
    if not a.no_ivf:
        ivf = IVFFlatIndex(D, a.nlist, nprobe=a.nprobe, capacity=N)
        ivf.train(x)
        for s in range(0, N, 262144):
            ivf.add(x[s:s + 262144])
        ivf._finalize()
        out["ivf"] = [{"Q": Q, "nlist": a.nlist, "nprobe": a.nprobe, "ms": round(timed(lambda: ivf.search(qs[:Q], k)), 4),
                       f"recall_at_{k}": round(recall(ivf.search(qs[:Q], k)[1], ref[:Q]), 4)} for Q in a.queries]
    out["flat_ms"] = {str(Q): round(v, 4) for Q, v in flat_ms.items()}
    out["flat_ms_again"] = {str(Q): round(timed(lambda: flat.search(qs[:Q], k)), 4) for Q in a.queries}     # (A-B-A: drift shows as a difference)
    out["resident_gb"] = {"flat_with_shadow": round(N * D * 6 / 1e9, 2), "graph": round((N * D * 6 + N * a.degree * 4 + out["n_entry"] * D * 6) / 1e9, 2),
                          "ivf_rows": round(N * D * 4 / 1e9, 2)}
    out["device_errors"] = int(_lib.lib().lrx_device_error_count(0))
    print(json.dumps(out), flush=True)
