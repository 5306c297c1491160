"""8-bit scalar-quantised inner-product index (SQ8Index, lrx_sq8_*, torch.ops.lrx.sq8_ip_topk, SQFaissSearch(quantizer_type="QT_8bit_uniform")):
training, codes and reconstruction against the numpy yardstick (tests/sq8_yardstick.py) bit for bit; search against an fp64 evaluation on the
GPU over the decoded rows -- ids and score BITS.
The band-overflow (streaming) path of k_sq8_select_rescore is reached with a realistic input: the clustered corpus below puts 10 000
identical rows inside every query's band, more than the 4096-entry list; the fallback counter shows it ran."""
import os

import numpy as np
import pytest
import torch

import sq8_yardstick as Y

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


def build(x, qtype="QT_8bit", chunk=65536, train_rows=None):
    from lightretriever_amd import SQ8Index
    idx = SQ8Index(x.shape[1], qtype, capacity=x.shape[0])
    idx.train(x if train_rows is None else x[:train_rows])
    for s in range(0, x.shape[0], chunk):
        idx.add(x[s:s + chunk])
    return idx


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("qtype", ["QT_8bit", "QT_8bit_uniform"])
def test_training_codes_and_reconstruction_equal_the_yardstick(qtype):
    from lightretriever_amd import SQ8Index
    uniform = qtype == "QT_8bit_uniform"
    d, n = 512, 70_000
    x = rows(n, d) * 3.0
    x[:, 5] = 0.125                                                 # a constant column: vdiff = 0
    x[17, 9] = float("nan")                                         # ignored by the training, code 0
    x[40_000, 11] = -0.0
    n_train = 50_000
    x[:n_train, 13] = float("nan")                                  # no training value at all: vmin = vdiff = 0, code 0, decoded 0
    x[n_train:] *= 1.5                                              # rows 50 000 .. lie partly outside the trained range
    xn = x.cpu().numpy()
    want = Y.train(xn[:n_train], uniform)
    idx = SQ8Index(d, qtype)
    idx.train(x[:n_train])
    assert torch.equal(bits(idx.trained), bits(torch.from_numpy(want).cuda()))
    pieces = SQ8Index(d, qtype)
    pieces.train(x[:1000])
    pieces.train(x[1000:30_001], more=True)
    pieces.train(x[30_001:n_train], more=True)
    assert torch.equal(bits(pieces.trained), bits(idx.trained))
    again = SQ8Index(d, qtype)
    again.train(x[:n_train].flip(0))                               # the order of the rows does not matter
    assert torch.equal(bits(again.trained), bits(idx.trained))
    nan_only = SQ8Index(d, qtype)
    nan_only.train(torch.full((3, d), float("nan"), device="cuda"))
    assert (nan_only.trained == 0).all() and np.array_equal(Y.train(np.full((3, d), np.nan, np.float32), uniform), nan_only.trained.cpu().numpy())
    with pytest.raises(ValueError):
        SQ8Index(d, qtype).train(x[:0])
    with pytest.raises(RuntimeError, match="not trained"):
        SQ8Index(d, qtype).add(x[:10])
    for s in range(0, n, 30_000):
        idx.add(x[s:s + 30_000])
    codes = Y.encode(xn, want)
    assert uniform or ((codes[n_train:] == 255).sum() > 100 and (codes[n_train:] == 0).sum() > 100)
    assert torch.equal(idx.codes(), torch.from_numpy(codes).cuda())
    assert torch.equal(idx.encode(x[123:4567]), torch.from_numpy(codes[123:4567]).cuda())
    rec = Y.decode(codes, want)
    assert torch.equal(bits(idx.reconstruct_n(0, n)), bits(torch.from_numpy(rec).cuda()))
    assert torch.equal(bits(idx.reconstruct_n(129, 300)), bits(torch.from_numpy(rec[129:429]).cuda()))
    if not uniform:                                                 # (the uniform quantiser has one range: a constant column is not special)
        assert want[13] == 0 and want[d + 13] == 0 and (idx.codes()[:, 13] == 0).all() and (idx.reconstruct_n(n_train, 10)[:, 13] == 0).all()
        assert (idx.codes()[:, 5] == 0).all() and (idx.reconstruct_n(0, 10)[:, 5] == 0.125).all()
    # a small search against the numpy yardstick end to end
    q = queries(7, d)
    Dw, Iw = Y.search(q.cpu().numpy(), codes[:3000], want, 20)
    small = SQ8Index(d, qtype)
    small.set_contents(torch.from_numpy(want), torch.from_numpy(codes[:3000]))
    D, I = small.search(q, 20)
    assert np.array_equal(I.cpu().numpy(), Iw) and np.array_equal(D.cpu().numpy().view(np.int32), Dw.view(np.int32))
    idx.reset()
    assert idx.ntotal == 0 and idx.is_trained


@pytest.mark.parametrize("n,d,nq,k,qtype", [
    (1_000_000, 2048, 100, 100, "QT_8bit"),
    (100_000, 2048, 1000, 1000, "QT_8bit"),       # the reference's evaluation point: 8 library chunks of 128 queries
    (10_000_000, 256, 100, 100, "QT_8bit"),       # three row chunks, merged
    (1_000_000, 4096, 16, 100, "QT_8bit"),
    (1_000_000, 2048, 1, 100, "QT_8bit"),         # a single query
    (5_000, 2048, 100, 100, "QT_8bit"),           # a tiny shard
    (300, 256, 10, 1000, "QT_8bit"),              # k > ntotal
    (1_000_000, 2048, 100, 100, "QT_8bit_uniform"),
    (5_000, 2048, 40, 100, "QT_8bit_uniform"),
    (300, 256, 10, 1000, "QT_8bit_uniform"),
])
def test_search_is_exact_over_the_decoded_rows(n, d, nq, k, qtype):
    x = rows(n, d)
    idx = build(x, qtype)
    del x
    q = queries(nq, d)
    got = idx.search(q, k)
    y = idx.vectors                                                 # (reconstruct_n equals the yardstick's decode: the test above)
    assert_same(got, fp64_topk(q, y, k))
    if k > n:
        assert (got[1][:, n:] == -1).all() and (got[0][:, n:] == -FLT_MAX).all()


def test_id_base_and_row_map():
    d, n, nq, k = 1024, 200_000, 50, 64
    x = rows(n, d)
    idx = build(x)
    q = queries(nq, d)
    D0, I0 = idx.search(q, k)
    idx.id_base = 1000
    D1, I1 = idx.search(q, k)
    assert torch.equal(I1, I0 + 1000) and torch.equal(bits(D1), bits(D0))
    row_map = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 7
    D2, I2 = idx.search(q, k, row_map=row_map)
    assert torch.equal(I2, I0 * 3 + 7) and torch.equal(bits(D2), bits(D0))


def test_band_overflow_is_exact_on_a_clustered_corpus_with_duplicates():
    from lightretriever_amd import _lib
    lib = _lib.lib()
    d, n = 2048, 200_000
    centres = rows(20, d, seed=5)
    x = centres.repeat_interleave(n // 20, dim=0)                  # 10 000 identical rows per cluster
    x[::7] += 1e-3 * rows(x[::7].shape[0], d, seed=6)
    x = x / x.norm(dim=1, keepdim=True)
    idx = build(x)
    q = centres[:8] + 1e-2 * queries(8, d, seed=7)
    lib.lrx_search_fallback_count(1)
    got = idx.search(q, 100)
    torch.cuda.synchronize()
    assert lib.lrx_search_fallback_count(1) > 0
    assert_same(got, fp64_topk(q, idx.vectors, 100))


def test_torch_op_and_ctypes_agree_with_the_class():
    from lightretriever_amd import _lib, torch_ops  # noqa: F401
    lib = _lib.lib()
    d, n, nq, k = 1024, 200_000, 50, 64
    for qtype in ("QT_8bit", "QT_8bit_uniform"):
        idx = build(rows(n, d), qtype)
        idx.id_base = 1000
        q = queries(nq, d)
        row_map = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 7
        D, I = idx.search(q, k, row_map=row_map)
        Dt, It = torch.ops.lrx.sq8_ip_topk(q, idx._codes, n, idx.trained, k, 1000, row_map)
        assert_same((Dt, It), (D, I))
        Dt, It = torch.ops.lrx.sq8_ip_topk(q[:5], idx._codes, n, idx.trained, k, 1000)
        assert_same((Dt, It), idx.search(q[:5], k))
        wsb = lib.lrx_sq8_ip_workspace_bytes(n, d, nq, k)
        assert lib.lrx_sq8_ip_chunk_queries(n, d, nq, k) == nq and lib.lrx_sq8_ip_chunk_queries(n, d, 1000, k) == 128
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        Dc = torch.empty(nq, k, device="cuda")
        Ic = torch.empty(nq, k, dtype=torch.int64, device="cuda")
        _lib.check(lib.lrx_sq8_ip_search(_lib.ptr(idx._codes), n, _lib.ptr(idx.trained), d, idx._qt, _lib.ptr(q), nq, k, 1000, _lib.ptr(Dc), _lib.ptr(Ic),
                                         _lib.ptr(row_map), _lib.ptr(ws), wsb, 0, _lib.current_stream()))
        assert_same((Dc, Ic), (D, I))
        assert lib.lrx_sq8_ip_search(_lib.ptr(idx._codes), n, _lib.ptr(idx.trained), d, idx._qt, _lib.ptr(q), nq, k, 1000, _lib.ptr(Dc), _lib.ptr(Ic),
                                     None, _lib.ptr(ws), wsb - 1, 0, _lib.current_stream()) != 0          # workspace too small: refused
        assert lib.lrx_sq8_ip_search(_lib.ptr(idx._codes), n, _lib.ptr(idx.trained), d, 1, _lib.ptr(q), nq, k, 1000, _lib.ptr(Dc), _lib.ptr(Ic),
                                     None, _lib.ptr(ws), wsb, 0, _lib.current_stream()) != 0              # QT_4bit: refused
    with pytest.raises(RuntimeError):
        torch.ops.lrx.sq8_ip_topk(q, idx._codes[:-1], n, idx.trained, k, 0, None)


@pytest.mark.parametrize("qtype", ["QT_8bit", "QT_8bit_uniform"])
def test_save_load_round_trip_and_a_yardstick_written_file(tmp_path, qtype):
    from lightretriever_amd import SQ8Index, index_io
    d, n = 768 + 256, 50_000
    x = rows(n, d)
    idx = build(x, qtype)
    path = str(tmp_path / "a.sq.faiss")
    idx.save(path)
    nt = 2 if qtype == "QT_8bit_uniform" else 2 * d
    assert os.path.getsize(path) == 37 + 28 + 8 + 4 * nt + 8 + n * d
    back = SQ8Index.load(path)
    assert back.qtype == qtype and back.ntotal == n and back.is_trained
    assert torch.equal(back.codes(), idx.codes()) and torch.equal(bits(back.trained), bits(idx.trained))
    q = queries(20, d)
    assert_same(back.search(q, 30), idx.search(q, 30))
    # a file written from the yardstick's training and codes loads and searches identically
    xn = x.cpu().numpy()
    trained = Y.train(xn, qtype == "QT_8bit_uniform")
    path2 = str(tmp_path / "b.sq.faiss")
    index_io.write_sq8(path2, trained, [Y.encode(xn, trained)], d, n, idx._qt)
    assert open(path2, "rb").read() == open(path, "rb").read()
    assert_same(SQ8Index.load(path2).search(q, 30), idx.search(q, 30))


def test_resident_memory_is_one_byte_per_element():
    d, n, chunk = 2048, 1_000_000, 65536
    from lightretriever_amd import SQ8Index
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    idx = SQ8Index(d, capacity=n)
    g = torch.Generator(device="cuda").manual_seed(3)
    for s in range(0, n, chunk):
        xs = torch.randn(min(chunk, n - s), d, device="cuda", generator=g)
        if s == 0:
            idx.train(xs)
        idx.add(xs)
        del xs
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    codes = -(-n // 128) * 128 * d
    assert grown <= codes + chunk * d * 4 + (4 << 20), (grown, codes)


def test_searchers_end_to_end_equal_the_yardstick(tmp_path):
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd import SQ8Index
    from lightretriever_amd.retriever import HybridSearch, SQFaissSearch
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, hm, model = build_stack(cfg_o, w)
    rng = np.random.default_rng(1)
    corpus = synth_corpus(rng, 60)
    qs = {"q0": "capital of france", "q1": "dense retrieval models", "q2": "a"}
    cids = sorted(corpus, key=lambda c: len(corpus[c]["text"]), reverse=True)
    emb = model.encode_corpus([corpus[c] for c in cids], batch_size=16)["dense_reps"]
    enc_q = model.encode_queries(list(qs.values()), batch_size=8)
    en = emb.float().cpu().numpy()

    def want_for(q, uniform=True):
        trained = Y.train(en, uniform)
        D, I = Y.search(q.cpu().numpy(), Y.encode(en, trained), trained, 10)
        return {qid: {cids[j]: float(s) for s, j in zip(D[i].tolist(), I[i].tolist())} for i, qid in enumerate(qs)}
    q_sq = (enc_q["dense_reps"] if "dense_reps" in enc_q else enc_q["emb_reps"]).to(emb.device).float()
    q_hy = (enc_q["emb_reps"] if enc_q.get("emb_reps") is not None else enc_q["dense_reps"]).to(emb.device).float()
    kw = dict(batch_size=16, quantizer_type="QT_8bit_uniform")
    assert SQFaissSearch(model, **kw).search(corpus, qs, top_k=10) == want_for(q_sq)
    assert HybridSearch(model, faiss_search_map="sq", **kw).search(corpus, qs, top_k=10) == want_for(q_hy)
    # _index_in_place: trained on the staged rows at commit, staging released
    s = SQFaissSearch(model, **kw)
    s._index_in_place([corpus[c] for c in cids], list(range(len(cids))), emb.shape[1])
    sidx = s.faiss_index.index
    assert isinstance(sidx, SQ8Index) and sidx.ntotal == len(cids) and sidx._stage is None and sidx.is_trained
    tr = Y.train(en, True)
    assert torch.equal(sidx.codes(), torch.from_numpy(Y.encode(en, tr)).cuda())
    # index / save / load of the searcher
    s = SQFaissSearch(model, **kw)
    s.index(emb, cids)
    s.save(str(tmp_path), "p")
    assert s.get_index_name() == "sq_faiss_index" and os.path.exists(tmp_path / "p.sq.faiss")
    t = SQFaissSearch(model, batch_size=16)                          # (constructed for QT_fp16: the file's qtype decides)
    t.load(str(tmp_path), "p")
    assert isinstance(t.faiss_index.index, SQ8Index) and t.qname == "QT_8bit_uniform"
    assert t.retrieve_with_emb(q_sq, list(qs), 10) == s.retrieve_with_emb(q_sq, list(qs), 10) == want_for(q_sq)
    # a per-dimension QT_8bit file loads through the searcher as well
    per_dim = SQ8Index(emb.shape[1], "QT_8bit")
    per_dim.train(emb.float())
    per_dim.add(emb.float())
    s.faiss_index.index = per_dim
    s.save(str(tmp_path), "d")
    t.load(str(tmp_path), "d")
    assert t.qname == "QT_8bit" and t.retrieve_with_emb(q_sq, list(qs), 10) == want_for(q_sq, uniform=False)
    # ... and a QT_fp16 file still gives the fp16 shard
    f = SQFaissSearch(model, batch_size=16)
    f.index(emb, cids)
    f.save(str(tmp_path), "h")
    t.load(str(tmp_path), "h")
    assert type(t.faiss_index.index).__name__ == "SQFp16Index" and t.qname == "QT_fp16"
