"""Product-quantised inner-product index (PQIndex, lrx_pq_ip_search / lrx_pq_encode / lrx_pq_lut, torch.ops.lrx.pq_ip_topk, PQFaissSearch):
codes, tables, ids and score BITS against the restatement of the contract in tests/pq_yardstick.py; training determinism and quality."""
import os

import numpy as np
import pytest
import torch

import pq_yardstick as Y

pytestmark = pytest.mark.gpu


def fixed(d, M, n, seed=0):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, size=(n, M)).astype(np.uint8)
    return C, codes


def queries(nq, d, seed=1):
    return np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)


def lut_torch(q, C):
    """Y.lut with torch fp64 elementwise ops on the device (the same sequential sum over i)."""
    M, _, dsub = C.shape
    acc = torch.zeros(q.shape[0], M, 256, dtype=torch.float64, device=q.device)
    qv = q.view(q.shape[0], M, dsub).double()
    for i in range(dsub):
        acc = acc + qv[:, :, i, None] * C[None, :, :, i].double()
    return acc.float()


def want_topk(q, C, codes, k, id_base=0, row_map=None):
    """Yardstick (D, I) on the device: Y.lut, Y.scores (sequential fp32 adds in m), stable descending sort (ties to the lower row)."""
    S = Y.scores_torch(lut_torch(q, C), codes)
    n = S.shape[1]
    kk = min(k, n)
    D = torch.full((q.shape[0], k), -Y.FLT_MAX, dtype=torch.float32, device=q.device)
    I = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=q.device)
    v, j = torch.sort(S, dim=1, descending=True, stable=True)
    D[:, :kk] = v[:, :kk]
    I[:, :kk] = (row_map[j[:, :kk]] if row_map is not None else j[:, :kk] + id_base)
    return D, I


def assert_same(got, want):
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


def make(d, M, n, seed=0):
    from lightretriever_amd import PQIndex
    C, codes = fixed(d, M, n, seed)
    idx = PQIndex(d, M)
    idx.set_contents(torch.from_numpy(C), torch.from_numpy(codes))
    return idx, torch.from_numpy(C).cuda(), torch.from_numpy(codes).cuda()


@pytest.mark.parametrize("d,M", [(768, 96), (2048, 64), (64, 8)])
def test_codes_equal_the_yardstick_including_forced_ties(d, M):
    from lightretriever_amd import PQIndex
    rng = np.random.default_rng(d)
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    C[:, 200] = C[:, 17]                                        # duplicate centroids: the lower j wins
    C[:, 5] = C[:, 4]
    x = rng.standard_normal((1001, d)).astype(np.float32)
    x[:50] = C[np.arange(M)[None, :], rng.choice([4, 5, 17, 200], size=(50, M))].reshape(50, d)   # rows sitting exactly on a duplicate
    idx = PQIndex(d, M)
    got = idx.encode(torch.from_numpy(x), torch.from_numpy(C)).cpu().numpy()
    want = Y.encode(x, C)
    assert np.array_equal(got, want)
    assert not np.isin(got[:50], [5, 200]).any()


def test_lut_equals_the_yardstick():
    from lightretriever_amd import _lib
    lib = _lib.lib()
    d, M = 1536, 96
    C, _ = fixed(d, M, 1)
    q = queries(7, d)
    lut = torch.empty(7, M, 256, device="cuda")
    Cg, qg = torch.from_numpy(C).cuda(), torch.from_numpy(q).cuda()
    _lib.check(lib.lrx_pq_lut(_lib.ptr(qg), 7, _lib.ptr(Cg), d, M, _lib.ptr(lut), _lib.current_stream()))
    assert np.array_equal(lut.cpu().numpy().view(np.int32), Y.lut(q, C).view(np.int32))


@pytest.mark.parametrize("d,M", [(768, 96), (1536, 96), (2048, 64), (2048, 256)])
@pytest.mark.parametrize("nq", [1, 7, 100, 1000])
def test_search_is_bit_identical_to_the_yardstick(d, M, nq):
    n = 20003                                                   # not a multiple of the 128-row block
    idx, C, codes = make(d, M, n, seed=nq)
    q = torch.from_numpy(queries(nq, d, seed=d)).cuda()
    for k in (1, 10, 100, 1000):
        assert_same(idx.search(q, k), want_topk(q, C, codes, k))


def want_range(q, C, codes, radius, id_base=0):
    """Yardstick (lims, D, I) on the device: the scores of want_topk, every row with s > radius, rows ascending inside a query."""
    S = Y.scores_torch(lut_torch(q, C), codes)
    mask = S > radius
    lims = torch.zeros(q.shape[0] + 1, dtype=torch.int64, device=q.device)
    lims[1:] = torch.cumsum(mask.sum(dim=1), 0)
    qi, rows = torch.nonzero(mask, as_tuple=True)               # row-major: queries ascending, rows ascending inside a query
    return lims, S[qi, rows], rows + id_base


def assert_same_range(got, want):
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


# M = 200 > PQ_SCAN_MC = 128: k_pq_scan loads the query's table in TWO passes per tile (sub-spaces [0, 128) and [128, 200)), and 200 % 16 = 8:
# the last 16-sub-space group of the second pass is half padding bytes (Mp = 208) -- the two at once, which M = 8 / 64 / 96 / 256 never give.
# n = 1029: two 1024-row tiles, the second with 5 rows (its block maxima cover 1 of 8 blocks); n = 127: less than one code block.
# (64, 8): one pass, ONE partial group and nothing else.
@pytest.mark.parametrize("d,M", [(400, 200), (64, 8)])
@pytest.mark.parametrize("n", [1029, 127])
@pytest.mark.parametrize("nq", [1, 5])
def test_two_pass_scan_with_a_padded_last_group_is_bit_identical_to_the_yardstick(d, M, n, nq):
    idx, C, codes = make(d, M, n, seed=M + n)
    q = torch.from_numpy(queries(nq, d, seed=d + nq)).cuda()
    for k in (1, 100, 1029 + 3):
        assert_same(idx.search(q, k), want_topk(q, C, codes, k))
    idx.id_base = 70
    S = Y.scores_torch(lut_torch(q, C), codes)
    top = torch.sort(S.reshape(-1), descending=True).values
    # radii: nothing passes (the largest score itself: strictly greater), ~20 rows per query, a stored score in the middle, everything
    for radius in (float(top[0]), float(top[min(20 * nq, top.numel() - 1)]), float(top[top.numel() // 2]), float("-inf")):
        assert_same_range(idx.range_search(q, radius), want_range(q, C, codes, radius, id_base=70))


# dsub = 1 and 3 (row pieces of 2 and 4 floats in LDS), dsub = 64: the largest served, whose dynamic LDS of (256 * 64 + 256 * 65) * 4 =
# 132 096 B is the only size above the 64 KiB default limit.  n = 257: a second workgroup with one row.
@pytest.mark.parametrize("d,M", [(16, 16), (48, 16), (1024, 16)])
def test_codes_at_the_smallest_and_largest_sub_space_widths(d, M):
    from lightretriever_amd import PQIndex
    rng = np.random.default_rng(d + 3)
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    C[:, 200] = C[:, 17]                                        # duplicate centroids: the lower j wins
    C[:, 255] = C[:, 0]
    x = rng.standard_normal((257, d)).astype(np.float32)
    x[:40] = C[np.arange(M)[None, :], rng.choice([0, 17, 200, 255], size=(40, M))].reshape(40, d)   # rows sitting exactly on a duplicate
    x[256] = C[np.arange(M), 255].reshape(d)                    # the lone row of the second workgroup too
    idx = PQIndex(d, M)
    got = idx.encode(torch.from_numpy(x), torch.from_numpy(C)).cpu().numpy()
    assert np.array_equal(got, Y.encode(x, C))
    assert not np.isin(got[:40], [200, 255]).any() and not np.isin(got[256], [200, 255]).any()
    # through add(): the same codes in the index's own blocks, rows [128, 257) in a second and third code block
    idx.set_contents(torch.from_numpy(C), torch.zeros(0, M, dtype=torch.uint8))
    idx.add(torch.from_numpy(x))
    assert np.array_equal(idx.codes().cpu().numpy(), got)


def test_sub_space_width_65_is_refused_by_the_library():
    from lightretriever_amd import _lib
    lib = _lib.lib()
    d, M = 65 * 16, 16
    x = torch.zeros(4, d, device="cuda")
    C = torch.zeros(M, 256, 65, device="cuda")
    codes = torch.full((128 * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.LrxError, match=r"pq_encode: dsub=65 > 64 is not served"):
        _lib.check(lib.lrx_pq_encode(_lib.ptr(x), 4, d, _lib.ptr(C), d, M, _lib.ptr(codes), 0, _lib.current_stream()))
    assert bool((codes == 0xAB).all())                          # refused before anything was launched


def test_fewer_rows_than_k_pads_and_duplicate_rows_tie_to_the_lower_row():
    d, M = 768, 96
    idx, C, codes = make(d, M, 300)
    rows = codes.clone()
    rows[250:] = rows[:50]                                      # rows 250.. duplicate rows 0..49: equal scores, the lower row first
    from lightretriever_amd import PQIndex
    idx = PQIndex(d, M)
    idx.set_contents(C, rows)
    q = torch.from_numpy(queries(9, d)).cuda()
    D, I = idx.search(q, 400)
    assert_same((D, I), want_topk(q, C, rows, 400))
    assert (I[:, 300:] == -1).all() and (D[:, 300:] == -Y.FLT_MAX).all()
    for i in range(9):
        pos = {int(r): p for p, r in enumerate(I[i, :300].tolist())}
        assert all(pos[j] < pos[250 + j] for j in range(50))
    empty = PQIndex(d, M)
    De, Ie = empty.search(q, 5)
    assert (Ie == -1).all() and (De == -Y.FLT_MAX).all()


def test_id_base_row_map_query_chunks_and_the_torch_op():
    from lightretriever_amd import _lib, torch_ops
    torch_ops.load()
    lib = _lib.lib()
    d, M, n = 768, 96, 300001
    idx, C, codes = make(d, M, n)
    nq, k = 1000, 50
    assert lib.lrx_pq_ip_chunk_queries(n, d, M, nq, k) < nq               # the call walks more than one query chunk (894 here)
    q = torch.from_numpy(queries(nq, d)).cuda()
    idx.id_base = 1000
    assert_same(idx.search(q, k), want_topk(q, C, codes, k, id_base=1000))
    row_map = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 7
    got = idx.search(q, k, row_map=row_map)
    assert_same(got, want_topk(q, C, codes, k, row_map=row_map))
    Dt, It = torch.ops.lrx.pq_ip_topk(q, idx._codes, idx.centroids, n, k, 1000, row_map)
    assert_same((Dt, It), got)
    Dt, It = torch.ops.lrx.pq_ip_topk(q[:5], idx._codes, idx.centroids, n, k, 1000)
    assert_same((Dt, It), idx.search(q[:5], k))


def test_row_chunks_are_merged():
    d, M, n = 64, 16, 5 * (1 << 20) + 77                         # more than one 4 Mi-row score matrix
    idx, C, codes = make(d, M, n)
    q = torch.from_numpy(queries(3, d)).cuda()
    for k in (10, 1000):
        assert_same(idx.search(q, k), want_topk(q, C, codes, k))


def test_full_size_1m_x_1536_m96_q100():
    d, M, n = 1536, 96, 1 << 20
    idx, C, codes = make(d, M, n)
    q = torch.from_numpy(queries(100, d)).cuda()
    assert_same(idx.search(q, 100), want_topk(q, C, codes, 100))


def test_add_encodes_like_the_yardstick_and_reconstructs():
    from lightretriever_amd import PQIndex
    d, M = 768, 96
    C, _ = fixed(d, M, 1)
    x = queries(777, d, seed=5)
    idx = PQIndex(d, M)
    with pytest.raises(RuntimeError, match="not trained"):
        idx.add(x)
    idx.set_contents(torch.from_numpy(C), torch.zeros(0, M, dtype=torch.uint8))
    idx.add(x[:300])
    idx.add(torch.from_numpy(x[300:]).cuda())
    codes = Y.encode(x, C)
    assert np.array_equal(idx.codes().cpu().numpy(), codes)
    rec = C[np.arange(M)[None, :], codes.astype(np.int64)].reshape(777, d)
    assert np.array_equal(idx.reconstruct_n(0, 777).cpu().numpy(), rec)
    assert np.array_equal(idx.reconstruct_n(100, 5).cpu().numpy(), rec[100:105])


def test_training_is_deterministic_lowers_the_objective_and_meets_the_recall_bar():
    from lightretriever_amd import PQIndex
    d, M = 64, 8
    x = Y.prototype_corpus(4000, d, M, seed=0)
    rng = np.random.default_rng(5)
    q = (x[rng.permutation(4000)[:50]] + 0.05 * rng.standard_normal((50, d))).astype(np.float32)
    a, b, init = PQIndex(d, M), PQIndex(d, M), PQIndex(d, M)
    a.train(x)
    b.train(x)
    init.train(x, niter=0)
    assert torch.equal(a.centroids, b.centroids)
    Ca, C0 = a.centroids.cpu().numpy(), init.centroids.cpu().numpy()
    # the yardstick's own run on this corpus: 1842 at initialisation -> 125 after 25 iterations
    assert Y.objective(x, Ca, Y.encode(x, Ca)) < 0.2 * Y.objective(x, C0, Y.encode(x, C0))
    a.add(x)
    _, Ip = a.search(q, 10)
    _, If = Y.topk((q.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32), 10)
    # bar: the CPU yardstick's k-means (pq_yardstick.kmeans) reaches recall@10 = 0.988 on this corpus and these queries
    assert Y.recall_at(Ip.cpu().numpy(), If, 10) >= 0.95
    with pytest.raises(ValueError, match="training rows"):
        PQIndex(d, M).train(x[:255])


def test_staging_slot_trains_then_encodes():
    from lightretriever_amd import PQIndex
    d, M = 64, 8
    x = torch.from_numpy(Y.prototype_corpus(1000, d, M, seed=2)).cuda()
    idx = PQIndex(d, M)
    idx.append_slot(1000).copy_(x)
    idx.commit(1000)
    ref = PQIndex(d, M)
    ref.train(x)
    ref.add(x)
    assert idx.is_trained and idx.ntotal == 1000 and idx._stage is None
    assert torch.equal(idx.centroids, ref.centroids) and torch.equal(idx.codes(), ref.codes())


def test_save_load_keeps_search_bit_identical(tmp_path):
    from lightretriever_amd import PQIndex
    d, M, n = 768, 96, 5000
    idx, C, codes = make(d, M, n)
    path = str(tmp_path / "a.pq.faiss")
    idx.save(path)
    assert os.path.getsize(path) == 37 + 24 + 8 + 4 * d * 256 + 8 + n * M + 9
    back = PQIndex.load(path)
    assert torch.equal(back.codes(), idx.codes()) and torch.equal(back.centroids, idx.centroids)
    q = torch.from_numpy(queries(20, d)).cuda()
    assert_same(back.search(q, 30), idx.search(q, 30))


def test_searchers_end_to_end_equal_the_yardstick(tmp_path):
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd.retriever import HybridSearch, PQFaissSearch
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, hm, model = build_stack(cfg_o, w)
    rng = np.random.default_rng(1)
    corpus = synth_corpus(rng, 300)                            # >= 256 rows: the chunk trains its own codebooks
    qs = {"q0": "capital of france", "q1": "dense retrieval models", "q2": "a"}
    cids = sorted(corpus, key=lambda c: len(corpus[c]["text"]), reverse=True)
    emb = model.encode_corpus([corpus[c] for c in cids], batch_size=16)["dense_reps"]
    enc_q = model.encode_queries(list(qs.values()), batch_size=8)
    M = 16

    def keep(searcher):                                         # (a search releases its shard: keep the last one for the yardstick)
        inner = searcher._index_in_place

        def wrapped(*a):
            r = inner(*a)
            idx = searcher.faiss_index.index
            searcher.kept = (idx.centroids.clone(), idx.codes())  # (copies: the searcher resets the shard after the search)
            return r
        searcher._index_in_place = wrapped
        return searcher

    def want_for(searcher, q):
        C, codes = searcher.kept
        assert np.array_equal(codes.cpu().numpy(), Y.encode(emb.float().cpu().numpy(), C.cpu().numpy()))
        D, I = want_topk(q, C, codes, 10)
        return {qid: {cids[j]: float(s) for s, j in zip(D[i].tolist(), I[i].tolist())} for i, qid in enumerate(qs)}
    q_pq = (enc_q["dense_reps"] if "dense_reps" in enc_q else enc_q["emb_reps"]).to(emb.device).float()
    q_hy = (enc_q["emb_reps"] if enc_q.get("emb_reps") is not None else enc_q["dense_reps"]).to(emb.device).float()
    s = keep(PQFaissSearch(model, batch_size=16, num_of_centroids=M))
    assert s.search(corpus, qs, top_k=10) == want_for(s, q_pq)
    h = HybridSearch(model, batch_size=16, faiss_search_map="pq", num_of_centroids=M)
    keep(h.dense_search)
    assert h.search(corpus, qs, top_k=10) == want_for(h.dense_search, q_hy)
    # index (train + add) / save / load of the searcher
    s = PQFaissSearch(model, batch_size=16, num_of_centroids=M)
    s.index(emb, cids)
    s.save(str(tmp_path), "p")
    assert s.get_index_name() == "pq_faiss_index" and os.path.exists(tmp_path / "p.pq.faiss")
    t = PQFaissSearch(model, batch_size=16, num_of_centroids=M)
    t.load(str(tmp_path), "p")
    assert t.retrieve_with_emb(q_pq, list(qs), 10) == s.retrieve_with_emb(q_pq, list(qs), 10)
