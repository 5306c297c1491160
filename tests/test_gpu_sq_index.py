"""fp16 scalar-quantised inner-product index (SQFp16Index, lrx_sq_fp16_ip_search, torch.ops.lrx.sq_fp16_ip_topk, SQFaissSearch): exact
top-k of (float) sum (double) q_i (double) c_i over the codes c = fp16(x), against an fp64 evaluation on the GPU -- ids and score BITS."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def rows(n, d, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, device="cuda", generator=g)
    return x / x.norm(dim=1, keepdim=True)


def queries(nq, d, seed=1):
    return rows(nq, d, seed)


def fp64_topk(q, c, k, chunk=1 << 18):
    """Yardstick: (q.double() @ c.double().T).float() in row chunks; the best k per query, ties to the lower row."""
    n = c.shape[0]
    qd = q.double()
    S = torch.empty(q.shape[0], n, dtype=torch.float32, device=q.device)
    for s in range(0, n, chunk):
        S[:, s:s + chunk] = (qd @ c[s:s + chunk].double().T).float()
    kk = min(k, n)
    D = torch.full((q.shape[0], k), -FLT_MAX, dtype=torch.float32, device=q.device)
    I = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=q.device)
    for i in range(q.shape[0]):
        v, j = torch.sort(S[i], descending=True, stable=True)
        D[i, :kk], I[i, :kk] = v[:kk], j[:kk]
    return D, I


def assert_same(got, want):
    Dg, Ig = got
    Dw, Iw = want
    assert torch.equal(Ig, Iw)
    assert torch.equal(Dg.view(torch.int32), Dw.view(torch.int32))


def build_sq(x, chunk=65536):
    from lightretriever_amd import SQFp16Index
    idx = SQFp16Index(x.shape[1], capacity=x.shape[0])
    for s in range(0, x.shape[0], chunk):
        idx.add(x[s:s + chunk])
    return idx


@pytest.mark.parametrize("n,d,nq,k", [
    (1_000_000, 2048, 100, 100),       # score-free filter, persistent emit
    (100_000, 2048, 1000, 1000),       # GEMM main pass, wide chunks (the reference's evaluation point)
    (10_000_000, 256, 100, 100),
    (1_000_000, 4096, 16, 100),        # fused launch
    (1_000_000, 2048, 1, 100),         # a single query
    (5_000, 2048, 100, 100),           # score-matrix filter (tiny shard)
    (300, 256, 10, 1000),              # k > ntotal
])
def test_search_is_exact_over_the_codes(n, d, nq, k):
    x = rows(n, d)
    idx = build_sq(x)
    q = queries(nq, d)
    got = idx.search(q, k)
    c = x.half()
    del x
    assert_same(got, fp64_topk(q, c, k))
    if k > n:
        assert (got[1][:, n:] == -1).all() and (got[0][:, n:] == -FLT_MAX).all()


def test_fallback_is_exact_on_a_clustered_corpus_with_duplicates():
    from lightretriever_amd import _lib
    lib = _lib.lib()
    d, n = 2048, 200_000
    centres = rows(20, d, seed=5)
    x = centres.repeat_interleave(n // 20, dim=0)                  # 10 000 identical rows per cluster
    x[::7] += 1e-3 * rows(x[::7].shape[0], d, seed=6)
    x = x / x.norm(dim=1, keepdim=True)
    idx = build_sq(x)
    q = centres[:8] + 1e-2 * queries(8, d, seed=7)
    lib.lrx_search_fallback_count(1)
    got = idx.search(q, 100)
    torch.cuda.synchronize()
    assert lib.lrx_search_fallback_count(1) > 0
    assert_same(got, fp64_topk(q, x.half(), 100))


@pytest.mark.parametrize("n,nq,k", [(300_000, 100, 100), (100_000, 300, 1000), (3_000, 40, 50)])
def test_bit_identical_to_the_flat_index_on_fp16_rows(n, nq, k):
    from lightretriever_amd import FlatIPIndex
    d = 2048
    x = rows(n, d).half().float()                                  # exactly fp16-representable
    flat = FlatIPIndex(d, capacity=n)
    flat.add(x)
    sq = build_sq(x)
    q = queries(nq, d)
    assert_same(sq.search(q, k), flat.search(q, k))
    wf = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    ws = torch.empty_like(wf)
    assert_same(sq.search(q, k, wire_out=ws), flat.search(q, k, wire_out=wf))
    assert torch.equal(ws, wf)


def test_codes_equal_x_half_and_the_flat_shadow():
    from lightretriever_amd import FlatIPIndex
    d, n = 512, 70_000
    x = rows(n, d) * 3.0
    sq = build_sq(x, chunk=30_000)
    assert torch.equal(sq.codes().view(torch.int16), x.half().view(torch.int16))
    flat = FlatIPIndex(d, capacity=n)
    flat.add(x)
    assert torch.equal(sq.codes().view(torch.int16), flat.shadow_rows().view(torch.int16))
    assert torch.equal(sq.reconstruct_n(100, 50), x[100:150].half().float())


def test_encoder_writes_the_codes_through_index_in_place():
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd.retriever import FlatIPFaissSearch, SQFaissSearch
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, hm, model = build_stack(cfg_o, w)
    rng = np.random.default_rng(0)
    corpus = synth_corpus(rng, 50)
    docs = list(corpus.values())
    sq = SQFaissSearch(model, batch_size=16)
    dim = enc.cfg.hidden_size
    sq._index_in_place(docs, list(range(len(docs))), dim)
    fl = FlatIPFaissSearch(model, batch_size=16)
    fl._index_in_place(docs, list(range(len(docs))), dim)
    sidx, fidx = sq.faiss_index.index, fl.faiss_index.index
    assert sidx.ntotal == fidx.ntotal == len(docs)
    assert sidx._x.numel() == 0                                    # staging released
    assert torch.equal(sidx.codes().view(torch.int16), fidx.vectors.half().view(torch.int16))
    assert torch.equal(sidx.codes().view(torch.int16), fidx.shadow_rows().view(torch.int16))


def test_resident_memory_is_two_bytes_per_element():
    d, n, chunk = 2048, 1_000_000, 65536
    from lightretriever_amd import SQFp16Index
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    idx = SQFp16Index(d, capacity=n)
    g = torch.Generator(device="cuda").manual_seed(3)
    for s in range(0, n, chunk):
        xs = torch.randn(min(chunk, n - s), d, device="cuda", generator=g)
        idx.add(xs)
        del xs
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    codes = -(-n // 128) * 128 * d * 2
    assert grown <= codes + chunk * d * 4 + (4 << 20), (grown, codes)
    assert grown < 6 * n * d * 0.5                                  # (the flat index needs 6 B/element)


def test_wire_words_torch_op_and_ctypes_agree_with_the_class():
    from lightretriever_amd import _lib, torch_ops  # noqa: F401
    lib = _lib.lib()
    d, n, nq, k = 1024, 200_000, 50, 64
    x = rows(n, d)
    idx = build_sq(x)
    idx.id_base = 1000
    q = queries(nq, d)
    row_map = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 7
    wire = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    D, I = idx.search(q, k, wire_out=wire, row_map=row_map)
    packed = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    _lib.check(lib.lrx_pack_topk(_lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map), 1000, nq * k, _lib.ptr(packed), _lib.current_stream()))
    assert torch.equal(wire, packed)
    Dt, It, Wt = torch.ops.lrx.sq_fp16_ip_topk(q, idx._xb, n, idx._bounds, k, 1000, row_map, 0)
    assert_same((Dt, It), (D, I))
    assert torch.equal(Wt, wire)
    wsb = lib.lrx_sq_fp16_ip_workspace_bytes(n, d, nq, k, 0)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    Dc = torch.empty(nq, k, device="cuda")
    Ic = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    _lib.check(lib.lrx_sq_fp16_ip_search(_lib.ptr(idx._xb), n, d, _lib.ptr(idx._bounds), _lib.ptr(q), nq, k, 1000, _lib.ptr(Dc), _lib.ptr(Ic),
                                         None, None, _lib.ptr(ws), wsb, 0, _lib.current_stream()))
    assert_same((Dc, Ic), (D, I))
    counts = idx.last_list_counts()
    assert counts.shape == (nq,) and (counts > 0).all()


def test_save_load_round_trip(tmp_path):
    from lightretriever_amd import SQFp16Index
    d, n = 768 + 256, 50_000
    x = rows(n, d)
    idx = build_sq(x)
    path = str(tmp_path / "a.sq.faiss")
    idx.save(path)
    assert os.path.getsize(path) == 37 + 28 + 8 + 8 + n * d * 2
    back = SQFp16Index.load(path)
    assert torch.equal(back.codes().view(torch.int16), idx.codes().view(torch.int16))
    q = queries(20, d)
    assert_same(back.search(q, 30), idx.search(q, 30))


def test_searchers_end_to_end_equal_the_fp64_yardstick(tmp_path):
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd.retriever import HybridSearch, SQFaissSearch
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, hm, model = build_stack(cfg_o, w)
    rng = np.random.default_rng(1)
    corpus = synth_corpus(rng, 60)
    qs = {"q0": "capital of france", "q1": "dense retrieval models", "q2": "a"}
    cids = sorted(corpus, key=lambda c: len(corpus[c]["text"]), reverse=True)
    emb = model.encode_corpus([corpus[c] for c in cids], batch_size=16)["dense_reps"]
    enc_q = model.encode_queries(list(qs.values()), batch_size=8)

    def want_for(q):
        D, I = fp64_topk(q, emb.half(), 10)
        return {qid: {cids[j]: float(s) for s, j in zip(D[i].tolist(), I[i].tolist())} for i, qid in enumerate(qs)}
    q_sq = (enc_q["dense_reps"] if "dense_reps" in enc_q else enc_q["emb_reps"]).to(emb.device).float()
    q_hy = (enc_q["emb_reps"] if enc_q.get("emb_reps") is not None else enc_q["dense_reps"]).to(emb.device).float()
    assert SQFaissSearch(model, batch_size=16).search(corpus, qs, top_k=10) == want_for(q_sq)
    assert HybridSearch(model, batch_size=16, faiss_search_map="sq").search(corpus, qs, top_k=10) == want_for(q_hy)
    qe = q_sq
    # index / save / load of the searcher
    s = SQFaissSearch(model, batch_size=16)
    s.index(emb, cids)
    s.save(str(tmp_path), "p")
    assert s.get_index_name() == "sq_faiss_index" and os.path.exists(tmp_path / "p.sq.faiss")
    t = SQFaissSearch(model, batch_size=16)
    t.load(str(tmp_path), "p")
    assert t.retrieve_with_emb(qe, list(qs), 10) == s.retrieve_with_emb(qe, list(qs), 10)
