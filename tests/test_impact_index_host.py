"""CPU: the impact index's host side (include/lrx.h lrx_impact_search) -- the numpy yardstick against the Python stand-in
the fusion tests use, pseudo-text parsing, the term dictionary, the overflow refusal, the constructor refusals, the HybridSearch wiring and
the agreement of header, ctypes table and torch op.  Nothing here touches a GPU."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import impact_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def distinct_score_case(seed=3, n=200, q=5):
    """200 documents of 12 terms from a 50-term vocabulary with weights that are multiples of 256, plus one shared term "s" of weight
    1 + perm(d) <= 200 < 256; every query counts "s" once: S = 256 x + 1 + perm(d), so the scores of a query are pairwise distinct and
    the pid-string tie rule of the stand-in cannot differ from the row rule of the contract."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    docs = []
    for d in range(n):
        doc = {str(int(t)): 256 * int(w) for t, w in zip(rng.choice(50, 12, replace=False), rng.integers(1, 300, 12))}
        doc["s"] = 1 + int(perm[d])
        docs.append(doc)
    queries = []
    for _ in range(q):
        qv = {str(int(t)): int(c) for t, c in zip(rng.choice(50, 4, replace=False), rng.integers(1, 4, 4))}
        qv["s"] = 1
        queries.append(qv)
    return docs, ["d%d" % i for i in range(n)], queries, ["q%d" % i for i in range(q)]


def as_pseudo_text(qv: dict) -> str:
    return " ".join(" ".join([t] * c) for t, c in qv.items())


def test_yardstick_equals_the_dict_stand_in_when_scores_are_distinct():
    from test_gpu_fusion import _DictImpactEngine
    docs, dids, queries, qids = distinct_score_case()
    engine = _DictImpactEngine()
    engine.index(docs[:120], dids[:120])
    engine.index(docs[120:], dids[120:])
    everything = engine.retrieve_with_emb(queries, qids, top_k=len(docs))
    for qid in qids:                                           # the condition under which the two tie rules agree, for the stand-in alone
        assert len(everything[qid]) == len(docs) and len(set(everything[qid].values())) == len(docs)
    for k in (1, 10, len(docs), len(docs) + 7):
        want = engine.retrieve_with_emb(queries, qids, top_k=k)
        assert Y.search_dicts(docs, dids, queries, qids, k) == want
        assert Y.search_dicts(docs, dids, [as_pseudo_text(q) for q in queries], qids, k) == want
        assert engine.retrieve_with_emb([as_pseudo_text(q) for q in queries], qids, top_k=k) == want


def test_yardstick_hits_only_rounding_and_row_ties():
    # rows 0..3: term 0 with weights 2^24 + 1, 2^24, 5, and a row without the query's term
    y = Y.Yardstick(*Y.csr_of([([0], [(1 << 24) + 1]), ([0], [1 << 24]), ([0, 1], [5, 9]), ([1], [7])]))
    D, I = y.search([([0], [1]), ([5], [3]), ([], [])], 4)
    assert I.tolist() == [[0, 1, 2, -1], [-1] * 4, [-1] * 4]               # 2^24 + 1 rounds to 2^24: a tie, the lower row first; row 3 is no hit
    assert D[0].tolist() == [float(1 << 24), float(1 << 24), 5.0, -Y.FLT_MAX] and (D[1:] == -Y.FLT_MAX).all()


def test_pseudo_text_is_split_on_whitespace_and_counted():
    from lightretriever_amd.retriever import ImpactSearch
    eng = ImpactSearch()
    eng.index([{"a": 3, "b": 1, "-1": 2}, {"c": 5}], ["x", "y"])
    text = "a b  a\tc\n a -1 zz -1"
    terms, counts = eng._query_terms(text)
    want = Counter(text.split())
    assert {t: c for t, c in zip(terms, counts)} == {eng.vocab[t]: c for t, c in want.items() if t != "zz"}
    assert (terms, counts) == Y.query_pairs(eng.vocab, text) == eng._query_terms(dict(want))


def test_dictionary_first_seen_order_unknown_terms_and_the_empty_marker():
    from lightretriever_amd.retriever import ImpactSearch
    eng = ImpactSearch()
    assert eng.name() == "impact_search"
    eng.index([{"7": 3, "-1": 1}, {"tok": 2, "7": 9}], ["a", "b"])
    eng.index([{"new": 4, "-1": 6}], ["c"])
    assert eng.vocab == {"7": 0, "-1": 1, "tok": 2, "new": 3} and list(eng.vocab) == ["7", "-1", "tok", "new"]     # first seen, over both calls
    assert eng.rev_mapping == ["a", "b", "c"]
    ix = eng.impact_index
    assert (ix.ntotal, ix.nnz, ix.n_terms) == (3, 6, 4) and ix.maxw.tolist() == [9, 6, 2, 4]                      # "-1" is a term like any other
    assert eng._query_terms({"never": 2, "7": 1, "-1": 3}) == ([0, 1], [1, 3])                                    # unknown terms are dropped
    assert eng._query_terms("never seen") == ([], [])
    assert Y.vocabulary([{"7": 3, "-1": 1}, {"tok": 2, "7": 9}, {"new": 4, "-1": 6}]) == eng.vocab
    eng._clear()
    assert (ix.ntotal, ix.nnz, eng.rev_mapping) == (0, 0, []) and list(eng.vocab) == ["7", "-1", "tok", "new"]
    with pytest.raises(ValueError, match="not an integer"):
        eng.index([{"7": 1.5}], ["d"])


def test_overflow_is_refused_on_the_host_before_the_device_is_touched():
    from lightretriever_amd import ImpactIndex
    from lightretriever_amd.impact_index import query_csr
    ix = ImpactIndex()
    # term 0: largest weight 2^30; term 1: largest weight 3; term 2 appears in no document
    ix.add(np.array([0, 1, 0, 1]), np.array([1 << 30, 3, 5, 1]), np.array([0, 2, 4]))
    assert ix.maxw.tolist() == [1 << 30, 3]
    # B_q = 2^30 + 3 * 357913941 = 2^31 - 1: allowed; one count more: 2^31 + 2, refused -- although no single document scores that much
    off, term, cnt = ix.check_queries(*query_csr([([0, 1], [1, 357913941]), ([2, 1], [1 << 40, 1])]))
    assert (off.tolist(), term.tolist(), cnt.tolist()) == ([0, 2, 3], [0, 1, 1], [1, 357913941, 1])     # the unseen term is dropped, whatever its count
    for bad in ([([0, 1], [1, 357913942])], [([1], [1]), ([0], [2])], [([0], [1 << 62])]):
        with pytest.raises(ValueError, match="2\\^31"):
            ix.search(*query_csr(bad), 10)
    assert ix._postings is None and ix.lib is None and ix._ws is None                                    # nothing was finalised, loaded or allocated
    with pytest.raises(ValueError):
        ix.check_queries([0, 1], [0], [0])                                                               # a count of 0
    with pytest.raises(ValueError):
        ix.add(np.array([0]), np.array([0]), np.array([0, 1]))                                           # a weight of 0
    with pytest.raises(ValueError):
        ix.search(*query_csr([([0], [1])]), 4096)                                                        # k beyond the selection's limit


def test_bm25_and_other_collections_are_refused():
    from lightretriever_amd.retriever import HybridSearch, ImpactSearch
    with pytest.raises(NotImplementedError, match="BM25"):
        ImpactSearch(anserini_impact_search=False)
    with pytest.raises(NotImplementedError, match="JsonVectorCollection"):
        ImpactSearch(anserini_vector_type="AclAnthology")
    with pytest.raises(NotImplementedError, match="BM25"):
        HybridSearch(model=None, sparse_search="gpu", anserini_impact_search=False)
    assert isinstance(ImpactSearch(anserini_impact_search=True, anserini_vector_type="JsonVectorCollection"), ImpactSearch)


def test_hybrid_search_builds_the_gpu_engine_on_request_only():
    from lightretriever_amd.retriever import HybridSearch, ImpactSearch
    from lightretriever.retriever.anserini_search import ImpactSearch as shim
    assert shim is ImpactSearch
    hs = HybridSearch(model=None, batch_size=16, sparse_search="gpu")
    assert isinstance(hs.sparse_search, ImpactSearch) and hs.sparse_search.batch_size == 16
    assert HybridSearch(model=None, sparse_search=None).sparse_search is None and HybridSearch(model=None).sparse_search is None
    engine = object()
    assert HybridSearch(model=None, sparse_search=engine).sparse_search is engine
    with pytest.raises(ValueError):
        HybridSearch(model=None, sparse_search="lucene")


def test_header_ctypes_table_and_torch_op_agree():
    import torch
    from lightretriever_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lrx.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lrx_impact_[a-z0-9_]+)\s*\(", src)))
    assert names == ["lrx_impact_chunk_queries", "lrx_impact_search", "lrx_impact_workspace_bytes"]
    l = _lib.lib()
    for name in names:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(l, name)
    assert _lib.ABI_VERSION == 9 and l.lrx_abi_version() == 9                                           # additive: the version stays
    # argument errors come back on the host
    assert l.lrx_impact_search(None, None, 0, 10, None, None, None, 1, 0, 0, None, None, None, None, 0, 0, None) == -1 and b"k=0" in l.lrx_last_error()
    assert l.lrx_impact_search(None, None, 0, 10, None, None, None, 1, 5, 0, None, None, None, None, 0, 100, None) == -1 and b"window_rows" in l.lrx_last_error()
    assert l.lrx_impact_search(None, None, 0, 1 << 31, None, None, None, 1, 5, 0, None, None, None, None, 0, 0, None) == -1
    assert l.lrx_impact_workspace_bytes(1000, 3, 10) >= 3 * 1024 * 4 and l.lrx_impact_chunk_queries(1000, 3, 10) == 3
    assert os.path.exists(build.build_torch_ops(verbose=False))
    from lightretriever_amd import torch_ops
    assert "impact_topk" in torch_ops.OPS
    schema = str(torch.ops.lrx.impact_topk.default._schema)
    assert schema.startswith("lrx::impact_topk(Tensor postings, Tensor term_off, int n_rows, Tensor q_off, Tensor q_term, Tensor q_cnt, int k")
