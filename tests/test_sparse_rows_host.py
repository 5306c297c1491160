"""CPU: SparseRows (cat, row ranges, to_dicts), the identity numbering of ImpactSearch for host-side query strings, the engine's bookkeeping
with SparseRows on CPU tensors (nothing touches the GPU before a search), HybridSearch(sparse_format=...) at construction, and the header /
ctypes / torch-op declarations of the CSR compaction."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 50


def rows_of(dicts, vocab_size=V):
    """[{token id | -1: weight}] -> SparseRows on the CPU (the marker -1 becomes term vocab_size)."""
    from lightretriever_amd.sparse_rows import SparseRows
    off, terms, weights = [0], [], []
    for d in dicts:
        terms += [vocab_size if t == -1 else t for t in d]
        weights += list(d.values())
        off.append(len(terms))
    return SparseRows(torch.tensor(off, dtype=torch.int64), torch.tensor(terms, dtype=torch.int32), torch.tensor(weights, dtype=torch.int32), vocab_size)


DOCS = [{3: 7, 10: 2, 49: 1}, {-1: 1}, {0: 5}, {3: 1, 4: 1, 5: 1, 6: 9}, {-1: 1}, {10: 4, 11: 4}]
AS_JSON = [{"3": 7, "10": 2, "49": 1}, {"-1": 1}, {"0": 5}, {"3": 1, "4": 1, "5": 1, "6": 9}, {"-1": 1}, {"10": 4, "11": 4}]


def test_len_ranges_cat_and_to_dicts():
    from lightretriever_amd import SparseRows
    r = rows_of(DOCS)
    assert len(r) == 6 and r.nnz == 12 and r.vocab_size == V and r.device.type == "cpu"
    assert r.to_dicts() == AS_JSON and [list(d) for d in r.to_dicts()] == [list(d) for d in AS_JSON]
    for a, b in ((0, 6), (1, 4), (2, 2), (5, 6), (0, 1), (4, 99), (-2, None)):
        part = r[a:b]
        assert part.to_dicts() == AS_JSON[a:b] and part.row_off[0].item() == 0 and part.row_off[-1].item() == part.nnz and len(part) == len(AS_JSON[a:b])
    assert len(r[6:]) == 0 and r[6:].row_off.tolist() == [0] and r[4:2].to_dicts() == []
    with pytest.raises(TypeError):
        r[2]
    with pytest.raises(ValueError):
        r[::2]
    whole = SparseRows.cat([r[:2], r[2:2], r[2:5], r[5:]])
    assert whole.to_dicts() == AS_JSON and whole.row_off.tolist() == r.row_off.tolist() and torch.equal(whole.terms, r.terms)
    assert SparseRows.cat([r]) is r and SparseRows.cat([r, r]).to_dicts() == AS_JSON + AS_JSON
    with pytest.raises(ValueError, match="vocab sizes"):
        SparseRows.cat([r, rows_of(DOCS, vocab_size=V + 1)])
    with pytest.raises(ValueError):
        SparseRows.cat([])
    with pytest.raises(ValueError, match="int64"):
        SparseRows(r.row_off.to(torch.int32), r.terms, r.weights, V)
    with pytest.raises(ValueError):
        SparseRows(r.row_off, r.terms, r.weights[:-1], V)


def test_identity_numbering_of_host_query_strings():
    """Only the canonical decimal form of a token id in [0, V) is that term, "-1" is the marker term V.  "007" is REFUSED (dropped), not 7: to
    the dict numbering and to Lucene it is a string no document holds, and the two numberings must give the same hits."""
    from lightretriever_amd.sparse_rows import identity_term
    assert [identity_term(t, V) for t in ("0", "7", "49")] == [0, 7, 49]
    assert identity_term("-1", V) == V
    for t in ("007", "00", "+7", "7 ", " 7", "7.0", "-2", "-0", "-01", "50", "51", "99999999999999999999", "tok", "", "٧", "²", "1e1", "0x7"):
        assert identity_term(t, V) is None, t


def test_engine_maps_host_queries_by_the_numbering_in_force():
    from lightretriever_amd.retriever import ImpactSearch
    by_rows, by_dicts = ImpactSearch(), ImpactSearch()
    by_rows.index(rows_of(DOCS), list("abcdef"))
    by_dicts.index(AS_JSON, list("abcdef"))
    assert by_rows.identity_vocab_size == V and by_rows.vocab == {} and by_dicts.identity_vocab_size is None
    ix = by_rows.impact_index
    assert (ix.ntotal, ix.nnz, ix.n_terms) == (6, 12, V + 1) and ix.maxw[[3, 10, V]].tolist() == [7, 4, 1] and by_rows.rev_mapping == list("abcdef")
    assert ix._postings is None and ix.lib is None                                   # nothing was finalised or loaded
    query = {"3": 2, "007": 1, "-1": 4, "-2": 1, "50": 1, "tok": 3, "10": 1}
    assert by_rows._query_terms(query) == ([3, V, 10], [2, 4, 1])
    assert by_rows._query_terms("3 tok 3 -1 50 -1 007 10 -1 -1 -2") == ([3, V, 10], [2, 4, 1])
    assert by_dicts._query_terms(query) == ([by_dicts.vocab[t] for t in ("3", "-1", "10")], [2, 4, 1])
    # queries as SparseRows: the arrays themselves under the identity numbering, renumbered through `vocab` otherwise -- same terms either way
    q = rows_of([{3: 2, -1: 4, 10: 1}, {}, {7: 1, 8: 2}, {11: 1, 2: 5}])             # (7, 8 and 2 are in no document)
    off, term, cnt = by_rows._query_rows(q)
    assert off is q.row_off and term is q.terms and cnt is q.weights
    name = {i: t for t, i in by_dicts.vocab.items()}
    off, term, cnt = by_dicts.impact_index.check_queries(*by_dicts._query_rows(q))
    assert off.tolist() == [0, 3, 3, 3, 4] and [name[t] for t in term.tolist()] == ["3", "-1", "10", "11"] and cnt.tolist() == [2, 4, 1, 1]
    off, term, cnt = by_rows.impact_index.check_queries(*by_rows._query_rows(q))
    assert off.tolist() == [0, 3, 3, 3, 4] and term.tolist() == [3, V, 10, 11] and cnt.tolist() == [2, 4, 1, 1]
    assert by_dicts._query_rows(q)[1].tolist() == [by_dicts.vocab[t] for t in ("3", "-1", "10", "11")]       # the unknown ids are gone already


def test_engine_refuses_to_mix_kinds_until_cleared():
    from lightretriever_amd.retriever import ImpactSearch
    eng = ImpactSearch()
    eng.index(AS_JSON[:3], list("abc"))
    with pytest.raises(ValueError, match="SparseRows after dicts"):
        eng.index(rows_of(DOCS[3:]), list("def"))
    assert eng.impact_index.ntotal == 3 and eng.identity_vocab_size is None
    eng._clear()
    eng.index(rows_of(DOCS[:3]), list("abc"))
    eng.index(rows_of(DOCS[3:]), list("def"))                                        # the same kind appends
    assert eng.impact_index.ntotal == 6 and eng.identity_vocab_size == V
    with pytest.raises(ValueError, match="dicts after SparseRows"):
        eng.index(AS_JSON[:1], ["g"])
    with pytest.raises(ValueError, match="token ids"):
        eng.index(rows_of(DOCS[:1], vocab_size=V + 7), ["g"])
    assert eng.impact_index.ntotal == 6 and eng.rev_mapping == list("abcdef")
    eng._clear()
    eng.index(rows_of([{3: 1}], vocab_size=V + 7), ["g"])                            # an empty engine takes another vocabulary size
    assert eng.identity_vocab_size == V + 7
    eng._clear()
    eng.index(AS_JSON, list("abcdef"))
    assert eng.identity_vocab_size is None and eng.impact_index.ntotal == 6


class _ForeignEngine:
    def index(self, corpus_emb, corpus_ids): ...
    def retrieve_with_emb(self, query_emb, query_ids, top_k): ...
    def _clear(self): ...


def test_hybrid_search_takes_csr_with_its_own_engine_only():
    from lightretriever_amd.retriever import HybridSearch, ImpactSearch
    hs = HybridSearch(model=None, sparse_search="gpu", sparse_format="csr")
    assert hs.sparse_format == "csr" and hs.dense_search.encode_kwargs == {"sparse_format": "csr"}
    assert HybridSearch(model=None, sparse_search=ImpactSearch(), sparse_format="csr").sparse_format == "csr"
    for engine in (_ForeignEngine(), None):
        with pytest.raises(ValueError, match="sparse_format='csr'"):
            HybridSearch(model=None, sparse_search=engine, sparse_format="csr")
    with pytest.raises(ValueError, match="sparse_format"):
        HybridSearch(model=None, sparse_search="gpu", sparse_format="coo")
    for hs in (HybridSearch(model=None, sparse_search="gpu"), HybridSearch(model=None, sparse_search=_ForeignEngine(), sparse_format="json")):
        assert hs.sparse_format == "json" and hs.dense_search.encode_kwargs == {} and hs._encode_kwargs == {}     # nothing new reaches the model


def test_csr_format_reaches_the_model_and_json_passes_nothing_new():
    """A stand-in model that records the arguments of its encode calls."""
    from lightretriever_amd.retriever import HybridSearch
    calls = []

    class Model:
        def encode_queries(self, queries, batch_size, **kw):
            calls.append(("q", kw))
            return {}

        def encode_corpus(self, corpus, batch_size, **kw):
            calls.append(("c", kw))
            return {}
    for fmt, extra in (("json", {}), ("csr", {"sparse_format": "csr"})):
        del calls[:]
        hs = HybridSearch(model=Model(), sparse_search="gpu", sparse_format=fmt)
        hs.encode_queries(["a"], batch_size=2)
        hs.encode_corpus(["a"], batch_size=2, show_progress_bar=False)
        assert calls == [("q", extra), ("c", dict(extra, show_progress_bar=False))]


def test_header_ctypes_table_and_torch_op_agree():
    from lightretriever_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lrx.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lrx_sparse_csr_[a-z0-9_]+)\s*\(", src)))
    assert names == ["lrx_sparse_csr_count", "lrx_sparse_csr_fill"]
    l = _lib.lib()
    for name in names:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(_lib.SIGNATURES[name][1]) and hasattr(l, name), name
    assert _lib.ABI_VERSION == 9 and l.lrx_abi_version() == 9                       # additive: the version stays
    # argument errors come back on the host, nothing is launched
    assert l.lrx_sparse_csr_count(None, 1, 8, 8, 100, 1, None, None) == -1 and b"sparse_csr_count" in l.lrx_last_error()
    assert l.lrx_sparse_csr_fill(None, 1, 8, 8, 100, 1, None, None, None, None) == -1 and b"sparse_csr_fill" in l.lrx_last_error()
    one = np.zeros(1, dtype=np.int64).ctypes.data
    assert l.lrx_sparse_csr_count(one, 1, 8, 4, 100, 1, one, None) == -1            # row_stride < vocab_size
    assert l.lrx_sparse_csr_count(one, 1, 8, 8, 0, 1, one, None) == -1              # quantization_factor 0
    assert l.lrx_sparse_csr_count(one, 0, 8, 8, 100, 1, one, None) == 0             # no rows: nothing to do
    assert l.lrx_sparse_csr_fill(one, 0, 8, 8, 100, 1, one, None, None, None) == 0
    assert os.path.exists(build.build_torch_ops(verbose=False))
    from lightretriever_amd import torch_ops
    assert "sparse_compact_csr" in torch_ops.OPS
    schema = str(torch.ops.lrx.sparse_compact_csr.default._schema)
    assert schema.startswith("lrx::sparse_compact_csr(Tensor reps, int quantization_factor") and schema.endswith("-> (Tensor, Tensor, Tensor)")
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.lrx.sparse_compact_csr(torch.zeros(2, 8), 100, True)              # CPU tensors have no kernel registered
