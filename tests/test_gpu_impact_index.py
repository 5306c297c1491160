"""GPU: the impact index (lrx_impact_search, ImpactIndex, ImpactSearch, HybridSearch(sparse_search="gpu"), torch.ops.lrx.impact_topk) against
the numpy yardstick of its contract (tests/impact_yardstick.py) -- bit-equal scores, equal ids -- and, where no tie straddles rank k, against
the Python stand-in of the fusion tests.  Shapes are the smallest at which the scan can go wrong: rows around every window cut, a posting
list spanning three windows, the 128-row block boundary, scores around 2^24 and at 2^31 - 1, more than one 4 Mi-row score matrix."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import impact_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    D, I = (torch.from_numpy(a) for a in want)
    assert torch.equal(got[1].cpu(), I)
    assert torch.equal(got[0].cpu().view(torch.int32), D.view(torch.int32))


def make(docs, window_rows=0, **kw):
    """docs: [(term ids, weights), ...] -> (ImpactIndex, Yardstick) over the same rows."""
    from lightretriever_amd import ImpactIndex
    csr = Y.csr_of(docs)
    idx = ImpactIndex(**kw)
    idx.window_rows = window_rows
    idx.add(*csr)
    return idx, Y.Yardstick(*csr)


def search(idx, queries, k, **kw):
    from lightretriever_amd.impact_index import query_csr
    return idx.search(*query_csr(queries), k, **kw)


def random_docs(rng, n, vocab, nnz, wmax=300):
    return [(rng.choice(vocab, nnz, replace=False), rng.integers(1, wmax, nnz)) for _ in range(n)]


@pytest.mark.parametrize("forced,W,ks", [(512, 512, (1, 10, 2 * 512 + 6)), (0, 2048, (1, 10, 2048)), (32768, 32768, (1, 10))])
def test_window_edges(forced, W, ks):
    """N = 2 W + 1 rows: term 0 sits in every row with one weight (a posting list spanning three windows, row ties across both cuts), terms
    1 .. 4 only in rows W - 1, W, W + 1 and 2 W.  k = N + 5 (padding, k > ntotal) fits the selection's k <= 2048 only at a window forced
    down to 512 rows; the library's own rule gives 2048-row windows to so few queries, and 32768 is the largest window there is."""
    N = 2 * W + 1
    docs = [([0], [3]) for _ in range(N)]
    for j, r in enumerate((W - 1, W, W + 1, 2 * W)):
        docs[r] = ([0, 1 + j], [3, 10 + j])
    idx, y = make(docs, window_rows=forced)
    queries = [([0], [2]), ([0, 1, 2, 3, 4], [1, 1, 2, 1, 3]), ([4, 1, 3, 2], [1, 5, 1, 1]), ([2], [7])]
    for k in ks:
        assert_same(search(idx, queries, k), y.search(queries, k))


@pytest.mark.parametrize("N", [130, 4096 + 130])
def test_block_maxima_across_the_128_row_boundary(N):
    """The single best row is the last one, in a block of two valid rows (N = 130: the whole row fits the selection's candidate buffer;
    4226: the selection walks the block maxima)."""
    rng = np.random.default_rng(N)
    docs = random_docs(rng, N, 40, 6)
    docs[N - 1] = (np.arange(40), np.full(40, 1000))
    idx, y = make(docs)
    queries = [(rng.choice(40, 5, replace=False), rng.integers(1, 4, 5)) for _ in range(4)]
    for k in (1, 3, 100):
        got = search(idx, queries, k)
        assert (got[1][:, 0] == N - 1).all()
        assert_same(got, y.search(queries, k))


def test_query_shapes():
    rng = np.random.default_rng(11)
    N = 1000
    docs = random_docs(rng, N, 200, 8)
    docs = [(np.where(t == 77, 200, t), w) for t, w in docs]                    # term 77 is inside the dictionary's range but in no document
    for r in (5, 400, 999):
        docs[r] = (np.append(docs[r][0], 300), np.append(docs[r][1], 9))        # term 300: three rows only
    idx, y = make(docs)
    few = [([300], [2]), ([300, 77], [1, 4])]                                  # fewer than k hits
    shapes = [([], []), ([77, 5000], [3, 1]), ([5000], [1])] + few + [([3, 3, 9], [1, 2, 1])]   # empty / unknown only / ... / a term twice
    for k in (1, 10):
        got = search(idx, shapes, k)
        assert_same(got, y.search(shapes, k))
        assert (got[1][:3] == -1).all() and (got[0][:3] == -Y.FLT_MAX).all()
    assert_same(search(idx, [([3], [3]), ([9], [1])], 10), y.search([([3, 3], [1, 2]), ([9], [1])], 10))      # repeated terms add their counts up
    many = [(rng.choice(201, 3, replace=False), rng.integers(1, 5, 3)) for _ in range(300)]
    assert_same(search(idx, many, 10), y.search(many, 10))
    assert_same(search(idx, many[:1], 50), y.search(many[:1], 50))              # Q = 1 on its own
    # a duplicate token in pseudo text, through the engine
    from lightretriever_amd.retriever import ImpactSearch
    eng = ImpactSearch()
    dicts = [{str(int(t)): int(w) for t, w in zip(*d)} for d in docs[:50]]
    eng.index(dicts, list(range(50)))
    assert eng.retrieve_with_emb(["3 9 3 unseen", ""], ["a", "b"], top_k=5) == Y.search_dicts(dicts, list(range(50)), [{"3": 2, "9": 1}, {}], ["a", "b"], 5)


def test_score_range_rounding_ties_and_the_int32_limit():
    T = 1 << 24
    docs = [([0], [T + 1]), ([0], [T - 1]), ([0], [T]), ([1], [(1 << 31) - 1]), ([2, 3], [1 << 30, (1 << 30) - 1]), ([2], [5])]
    idx, y = make(docs)
    queries = [([0], [1]), ([1], [1]), ([2, 3], [1, 1])]
    got = search(idx, queries, 4)
    assert_same(got, y.search(queries, 4))
    assert got[1][0].tolist() == [0, 2, 1, -1] and got[0][0].tolist()[:3] == [float(T), float(T), float(T - 1)]     # 2^24 + 1 -> 2^24: a tie, row 0 first
    assert got[1][1].tolist() == [3, -1, -1, -1] and got[0][1, 0].item() == float(1 << 31)                         # S = 2^31 - 1 exactly, one conversion
    assert got[1][2].tolist() == [4, 5, -1, -1] and got[0][2, 0].item() == float(1 << 31)                          # ... and as a sum of two postings
    for over in ([([1], [2])], [([2, 3], [1, 2])], [([0], [1]), ([1, 2], [1, 1])]):
        with pytest.raises(ValueError, match="2\\^31"):
            search(idx, over, 4)


def test_row_chunks_are_merged():
    """4 Mi + 77 documents x 4 terms, added as device arrays: two score matrices; the last 77 rows carry the heaviest weights, so every list mixes
    both chunks, and small integer scores tie across the chunk cut."""
    from lightretriever_amd import ImpactIndex
    n, V = (1 << 22) + 77, 1000
    g = torch.Generator().manual_seed(5)
    base = torch.randint(0, V, (n, 1), generator=g)
    terms = ((base + torch.arange(4) * 250) % V).reshape(-1).to(torch.int32).cuda()                   # four distinct terms per document
    weights = torch.randint(1, 4, (n, 4), generator=g)
    weights[-77:] += torch.randint(0, 3, (77, 4), generator=g) * 50
    weights = weights.reshape(-1).to(torch.int32).cuda()
    off = torch.arange(n + 1, device="cuda", dtype=torch.int64) * 4
    idx = ImpactIndex()
    idx.add(terms, weights, off)
    assert (idx.ntotal, idx.nnz) == (n, 4 * n)
    y = Y.Yardstick(terms.cpu().numpy(), weights.cpu().numpy(), off.cpu().numpy())
    rng = np.random.default_rng(6)
    queries = [(rng.choice(V, 8, replace=False), rng.integers(1, 3, 8)) for _ in range(3)]
    for k in (10, 1000):
        got, want = search(idx, queries, k), y.search(queries, k)
        assert (want[1] >= 1 << 22).any() and (want[1][:, -1] < 1 << 22).all()
        assert_same(got, want)


def test_lifecycle_refinalise_reset_id_base_and_row_map():
    rng = np.random.default_rng(21)
    docs = random_docs(rng, 700, 60, 5)
    queries = [(rng.choice(60, 4, replace=False), rng.integers(1, 4, 4)) for _ in range(6)]
    idx, y_first = make(docs[:300])
    assert (idx.ntotal, idx.nnz) == (300, 1500)
    assert_same(search(idx, queries, 20), y_first.search(queries, 20))
    idx.add(*Y.csr_of(docs[300:]))                                            # an add after a search: the next search re-finalises
    assert (idx.ntotal, idx.nnz) == (700, 3500)
    y = Y.Yardstick(*Y.csr_of(docs))
    want = y.search(queries, 20)
    assert_same(search(idx, queries, 20), want)
    hit = want[1] >= 0
    idx.id_base = 1000
    assert_same(search(idx, queries, 20), (want[0], np.where(hit, want[1] + 1000, -1)))
    idx.id_base = 0
    row_map = torch.from_numpy(rng.permutation(700) + 5000).cuda()
    assert_same(search(idx, queries, 20, row_map=row_map), (want[0], np.where(hit, row_map.cpu().numpy()[np.maximum(want[1], 0)], -1)))
    idx.reset()
    assert (idx.ntotal, idx.nnz, idx.n_terms) == (0, 0, 0)
    D, I = search(idx, queries, 5)
    assert (I == -1).all() and (D == -Y.FLT_MAX).all()
    idx.add(*Y.csr_of(docs[:10]))                                             # ... and the index is usable again, rows from 0
    assert_same(search(idx, queries, 5), Y.Yardstick(*Y.csr_of(docs[:10])).search(queries, 5))


def test_engine_equals_the_stand_in_on_distinct_scores():
    from test_gpu_fusion import _DictImpactEngine
    from test_impact_index_host import as_pseudo_text, distinct_score_case
    from lightretriever_amd.retriever import ImpactSearch
    docs, dids, queries, qids = distinct_score_case()
    ref, eng = _DictImpactEngine(), ImpactSearch()
    for e in (ref, eng):
        e.index(docs[:120], dids[:120])
        e.index(docs[120:], dids[120:])
    for k in (10, len(docs)):
        want = ref.retrieve_with_emb(queries, qids, top_k=k)
        assert eng.retrieve_with_emb(queries, qids, top_k=k) == want
        assert eng.retrieve_with_emb([as_pseudo_text(q) for q in queries], qids, top_k=k) == want
    eng._clear()
    assert eng.retrieve_with_emb(queries, qids, top_k=3) == {q: {} for q in qids}


@pytest.mark.parametrize("mode", ["tok", "spr"])
def test_hybrid_search_serves_sparse_hits_with_its_own_engine(mode):
    """HybridSearch(sparse_search="gpu") on the stack, corpus and queries of the fusion tests (three chunks of 25): tok / spr equal the
    yardstick fed with the same encoded vectors in the searcher's row order (longest text first), emb_tok / den_spr the linear fusion of the
    two final lists; where the stand-in's 10th and 11th scores differ its list is the same."""
    from test_gpu_api import build_stack, synth_corpus
    from test_gpu_fusion import _DictImpactEngine
    from helpers import load_model_golden
    from lightretriever_amd.modeling import LrxExactSearchModel, LrxHybridModel
    from lightretriever_amd.retriever import HybridSearch, ImpactSearch, _sorted_corpus
    from lightretriever_amd.score_fuse_utils import fuse_scores_linear
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, _, _ = build_stack(cfg_o, w)
    if mode == "tok":
        hm = LrxHybridModel(enc, normalize=True, pad_token_id=tok.pad_token_id, encode_sparse=True, sparse_top_k_psg=24)
        model = LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=32, p_max_len=64, eval_batch_size_embedding_bag=100)
        model.query_prompt = "query: "
        dense, sparse, fused, q_key = "emb", "tok", "emb_tok", "token_id_reps"
    else:
        hm = LrxHybridModel(enc, normalize=True, pad_token_id=tok.pad_token_id, encode_sparse=True, sparse_top_k_psg=24, hybrid_use_sparse_vector=True,
                            hybrid_use_dense_vector=True, hybrid_use_emb_vector=False, sparse_top_k_qry=12)
        model = LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=32, p_max_len=64)
        dense, sparse, fused, q_key = "den", "spr", "den_spr", "sparse_reps"
    corpus = synth_corpus(np.random.default_rng(2), 60)
    queries = {"q0": "capital of france paris", "q1": "dense retrieval with large language models", "q2": "amd instinct memory search"}
    searcher = HybridSearch(model, batch_size=8, corpus_chunk_size=25, fuse_weights=[0.6, 0.4], return_all_results=True, sparse_search="gpu")
    res = searcher.search(corpus, queries, top_k=10)
    assert list(res) == [dense, sparse, fused] and isinstance(searcher.sparse_search, ImpactSearch)
    assert searcher.sparse_search.impact_index.ntotal == 0 and searcher.sparse_search.rev_mapping == []       # three chunks went in, cleared at the end
    ids, docs = _sorted_corpus(corpus)
    doc_vecs = model.encode_corpus(docs, batch_size=8)["sparse_reps"]
    q_vecs = model.encode_queries(list(queries.values()), batch_size=8)[q_key]
    want = Y.search_dicts(doc_vecs, ids, q_vecs, list(queries), 10)
    assert res[sparse] == want and all(len(v) > 0 for v in want.values())
    dense_only = HybridSearch(model, batch_size=8, corpus_chunk_size=25, return_all_results=True).search(corpus, queries, top_k=10)[dense]
    assert res[dense] == dense_only and res[fused] == fuse_scores_linear([dense_only, want], weights=[0.6, 0.4])
    ref = _DictImpactEngine()
    ref.index(doc_vecs, ids)
    top11 = ref.retrieve_with_emb(q_vecs, list(queries), 11)
    clear = [q for q, hits in top11.items() if len(hits) < 11 or sorted(hits.values())[0] != sorted(hits.values())[1]]
    assert clear                                                                # at least one query without a tie across rank 10
    top10 = ref.retrieve_with_emb(q_vecs, list(queries), 10)
    for q in clear:
        assert res[sparse][q] == top10[q]
    assert HybridSearch(model, batch_size=8, corpus_chunk_size=25, fuse_weights=[0.6, 0.4], sparse_search="gpu").search(corpus, queries, top_k=10) == res[fused]


def test_torch_op_returns_what_the_index_returns():
    from lightretriever_amd import torch_ops  # noqa: F401
    from lightretriever_amd.impact_index import query_csr
    rng = np.random.default_rng(31)
    docs = random_docs(rng, 5000, 100, 6)
    idx, _ = make(docs)
    queries = [(rng.choice(100, 4, replace=False), rng.integers(1, 9, 4)) for _ in range(7)]
    D, I = search(idx, queries, 33)
    off, term, cnt = (torch.from_numpy(a.astype(np.int32)).cuda() for a in query_csr(queries))
    for window_rows in (0, 256):
        D2, I2 = torch.ops.lrx.impact_topk(idx._postings, idx._term_off, idx.ntotal, off, term, cnt, 33, 0, None, window_rows)
        assert torch.equal(I, I2) and torch.equal(D.view(torch.int32), D2.view(torch.int32))
    row_map = torch.arange(5000, device="cuda") * 2
    D3, I3 = torch.ops.lrx.impact_topk(idx._postings, idx._term_off, idx.ntotal, off, term, cnt, 33, row_map=row_map)
    assert torch.equal(torch.where(I >= 0, I * 2, I), I3) and torch.equal(D, D3)
    with pytest.raises(RuntimeError, match="q_off"):
        torch.ops.lrx.impact_topk(idx._postings, idx._term_off, idx.ntotal, off, term[:-1], cnt[:-1], 33)
