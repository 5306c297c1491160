"""GPU: sparse vectors from the encoder to the impact index without leaving the device -- lrx_sparse_csr_count / lrx_sparse_csr_fill
(ops.sparse_compact_csr, torch.ops.lrx.sparse_compact_csr), SparseRows, ImpactSearch over SparseRows, HybridSearch(sparse_format="csr").
Everything is integer arithmetic on fp32 products that numpy reproduces bit for bit, so every comparison is torch.equal / ==.
Shapes: V = 1500 (one full 1024-column stretch plus a tail; rows of V + 8 floats keep the 16-byte loads), V = 1024, V = 1 (rows of 9 floats:
the element-wise loads), V = 9000 and 12291 (more than one 8192-column sweep, 70 rows: more than one workgroup)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

HALF_EVEN = [0.5, 1.5, 2.5, 0.49999997, 1e-9]        # x * q of the rounding row -> 0, 2, 2, 0, 0 (half to even, fp32)


def case_rows(V: int, q: int) -> np.ndarray:
    """fp32 [6, V + 8] (the rows are the first V columns; the 8 pad columns hold values that must not be read as entries): all zeros, all
    negative, every entry non-zero, non-zeros at columns 0 and V - 1 only, a random row of about 3 % non-zeros, the half-even row."""
    rng = np.random.default_rng(V * 1000 + q)
    x = np.zeros((6, V + 8), dtype=np.float32)
    x[:, V:] = 7.0
    x[1, :V] = -rng.random(V, dtype=np.float32) - 0.01
    x[2, :V] = rng.random(V, dtype=np.float32) + 0.02
    x[3, 0], x[3, V - 1] = 0.37, 2.5
    x[4, :V] = np.where(rng.random(V) < 0.03, rng.random(V, dtype=np.float32) * 3, 0) * np.where(rng.random(V) < 0.1, -1, 1)   # a few of them negative
    vals = (np.asarray(HALF_EVEN, dtype=np.float32) / np.float32(q)).astype(np.float32)
    x[5, :min(V, len(vals))] = vals[:V]
    return x


def expected_csr(x: np.ndarray, V: int, q: int, empty_marker: bool):
    w = np.rint(np.maximum(x[:, :V], np.float32(0)) * np.float32(q)).astype(np.int64)       # fp32 product, half to even
    off, terms, weights = [0], [], []
    for row in w:
        nz = np.flatnonzero(row)
        if nz.size == 0 and empty_marker:
            terms.append(np.array([V])), weights.append(np.array([1]))
        else:
            terms.append(nz), weights.append(row[nz])
        off.append(off[-1] + len(terms[-1]))
    return (torch.tensor(off, dtype=torch.int64), torch.from_numpy(np.concatenate(terms).astype(np.int32)),
            torch.from_numpy(np.concatenate(weights).astype(np.int32)))


def device_rows(x: np.ndarray, V: int) -> torch.Tensor:
    return torch.from_numpy(x).cuda()[:, :V]                       # row_stride = V + 8


@pytest.mark.parametrize("q", [100, 64])
@pytest.mark.parametrize("V", [1500, 1024, 1, 9000])
def test_kernels_against_numpy(V, q):
    from lightretriever_amd import ops
    x = case_rows(V, q)
    if q == 64 and V >= len(HALF_EVEN):      # a power of two: x = value / q and x * q are exact, so the row is what its name says
        assert np.rint(x[5, :5] * np.float32(q)).tolist() == [0, 2, 2, 0, 0] and (x[5, :5] * np.float32(q)).tolist() == np.float32(HALF_EVEN).tolist()
    reps = device_rows(x, V)
    assert reps.stride(0) == V + 8
    for marker in (False, True):
        off, terms, weights = expected_csr(x, V, q, marker)
        got = ops.sparse_compact_csr(reps, q, empty_marker=marker)
        assert got.vocab_size == V and len(got) == 6
        assert torch.equal(got.row_off.cpu(), off)
        assert torch.equal(got.terms.cpu(), terms)
        assert torch.equal(got.weights.cpu(), weights)
    # rows that are not 16-byte aligned (a view one float into the buffer) take the element-wise loads: same result
    shifted = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), x.reshape(-1)])).cuda()[1:].view(6, V + 8)[:, :V]
    assert shifted.data_ptr() % 16 == 4
    got = ops.sparse_compact_csr(shifted, q, empty_marker=True)
    assert all(torch.equal(a.cpu(), b) for a, b in zip((got.row_off, got.terms, got.weights), expected_csr(x, V, q, True)))


def test_many_rows_over_more_than_one_sweep():
    """70 rows (more workgroups than one) of V = 8192 + 4096 + 3 columns: two sweeps, the second one partly filled, a tail of 3; the last row and
    a middle one are empty, so a marker is the final pair."""
    from lightretriever_amd import ops
    V, B, q = 8192 + 4096 + 3, 70, 100
    rng = np.random.default_rng(5)
    x = np.where(rng.random((B, V)) < 0.03, rng.random((B, V)) * 4 - 0.5, 0).astype(np.float32)
    x[[31, B - 1]] = 0
    x[7, -3:] = 1.0                                                # the tail columns
    got = ops.sparse_compact_csr(torch.from_numpy(x).cuda(), q)
    off, terms, weights = expected_csr(x, V, q, True)
    assert torch.equal(got.row_off.cpu(), off) and torch.equal(got.terms.cpu(), terms) and torch.equal(got.weights.cpu(), weights)
    assert got.terms[-1].item() == V and got.weights[-1].item() == 1


def test_no_rows_and_argument_errors():
    from lightretriever_amd import ops
    got = ops.sparse_compact_csr(torch.zeros(0, 40, device="cuda"), 100)
    assert len(got) == 0 and got.nnz == 0 and got.row_off.tolist() == [0]
    with pytest.raises(ValueError):
        ops.sparse_compact_csr(torch.zeros(2, 40, device="cuda", dtype=torch.float64), 100)
    with pytest.raises(ValueError):
        ops.sparse_compact_csr(torch.zeros(40, 2, device="cuda").t(), 100)


@pytest.mark.parametrize("V", [1500, 1024, 1])
def test_agreement_with_the_capacity_kernel(V):
    from lightretriever_amd import ops
    x = case_rows(V, 100)
    reps = device_rows(x, V)
    ids, w, cnt = (t.cpu() for t in ops.sparse_compact(reps, 100))
    rows = ops.sparse_compact_csr(reps, 100, empty_marker=True).to("cpu")
    for b in range(len(rows)):
        n = int(cnt[b])
        lo, hi = int(rows.row_off[b]), int(rows.row_off[b + 1])
        if n == 0:
            assert (rows.terms[lo:hi].tolist(), rows.weights[lo:hi].tolist()) == ([V], [1])
        else:
            assert torch.equal(rows.terms[lo:hi], ids[b, :n]) and torch.equal(rows.weights[lo:hi], w[b, :n])
    bare = ops.sparse_compact_csr(reps, 100, empty_marker=False)
    assert torch.equal((bare.row_off[1:] - bare.row_off[:-1]).cpu(), cnt.to(torch.int64))


class _Converter:
    """convert_sparse_reps_to_json / _to_csr are methods of LrxHybridModel that only use its device."""
    device = torch.device("cuda")


def test_to_dicts_equals_the_json_form():
    from lightretriever_amd.modeling import LrxHybridModel
    from lightretriever_amd.sparse_rows import SparseRows
    V = 1500
    reps = device_rows(case_rows(V, 100), V)
    want = LrxHybridModel.convert_sparse_reps_to_json(_Converter(), reps, quantization_factor=100)
    rows = LrxHybridModel.convert_sparse_reps_to_csr(_Converter(), reps, quantization_factor=100)
    assert isinstance(rows, SparseRows) and rows.device.type == "cuda" and rows.vocab_size == V
    got = rows.to_dicts()
    assert got == want and [list(d) for d in got] == [list(d) for d in want]           # ... and in the same (ascending id) order
    assert want[0] == want[1] == {"-1": 1} and want[3] == {"0": 37, str(V - 1): 250}
    assert rows[2:5].to_dicts() == want[2:5] and SparseRows.cat([rows[:4], rows[4:]]).to_dicts() == want
    one = LrxHybridModel.convert_sparse_reps_to_csr(_Converter(), reps[3], quantization_factor=100)      # a single vector is one row
    assert one.to_dicts() == [want[3]]


# ---- engine ------------------------------------------------------------------------------------------------------------------------
V_ENGINE = 1500


@pytest.fixture(scope="module")
def engine_case():
    """About 300 documents over V = 1500 as fp32 rows (some empty), compacted once to SparseRows and to dicts; 20 queries in three forms."""
    from lightretriever_amd import ops
    from lightretriever_amd.sparse_rows import SparseRows
    rng = np.random.default_rng(77)
    n, V = 301, V_ENGINE
    x = np.where(rng.random((n, V)) < 0.02, rng.random((n, V)) * 2.5, 0).astype(np.float32)
    x[[0, 17, 150, 300]] = 0                                         # empty documents: the marker
    rows = ops.sparse_compact_csr(torch.from_numpy(x).cuda(), 100)
    dicts = rows.to_dicts()
    assert dicts[17] == {"-1": 1} and sum(len(d) for d in dicts) == rows.nnz
    qd = [{str(int(t)): int(c) for t, c in zip(rng.choice(V, 6, replace=False), rng.integers(1, 5, 6))} for _ in range(16)]
    qd.append({"3": 2, "99999": 4, "word": 1, "7": 1})              # unknown terms: an id beyond V, a non-numeric token
    qd.append({"-1": 1})                                            # the empty query
    qd.append({"-1": 2, "11": 1})
    qd.append({"5": 3, "8": 1})                                     # "5 8 5 5" as text, (5, 1) (8, 1) (5, 2) as rows: a repeated term
    text = [" ".join(t for t, c in q.items() for _ in range(c)) for q in qd]
    text[-1] = "5 8 5 5"
    off, terms, cnts = [0], [], []
    for q in qd[:-1]:
        known = [(V if t == "-1" else int(t), c) for t, c in q.items() if t == "-1" or (t.isdigit() and int(t) < V)]
        terms += [t for t, _ in known]
        cnts += [c for _, c in known]
        off.append(len(terms))
    terms += [5, 8, 5]
    cnts += [1, 1, 2]
    off.append(len(terms))
    qrows = SparseRows(torch.tensor(off, dtype=torch.int64), torch.tensor(terms, dtype=torch.int32), torch.tensor(cnts, dtype=torch.int32), V).to("cuda")
    return rows, dicts, [f"d{i}" for i in range(n)], {"dicts": qd, "text": text, "rows": qrows}, [f"q{i}" for i in range(len(qd))]


def test_engine_gives_the_same_hits_for_every_document_and_query_form(engine_case):
    from lightretriever_amd.impact_index import query_csr
    from lightretriever_amd.retriever import ImpactSearch
    rows, dicts, dids, queries, qids = engine_case
    results, lists = {}, {}
    for kind, docs in (("dicts", dicts), ("rows", rows)):
        eng = ImpactSearch()
        eng.index(docs[:120], dids[:120])                            # two calls: the second appends
        eng.index(docs[120:], dids[120:])
        assert (eng.identity_vocab_size is None) == (kind == "dicts") and eng.impact_index.ntotal == len(dids)
        for form, q in queries.items():
            for k in (10, len(dids)):
                results[kind, form, k] = eng.retrieve_with_emb(q, qids, top_k=k)
            csr = eng._query_rows(q) if form == "rows" else query_csr([eng._query_terms(x) for x in q])
            lists[kind, form] = tuple(t.cpu() for t in eng.impact_index.search(*csr, 10))
    first = results["dicts", "dicts", 10]
    assert all(len(first[q]) == 10 for q in qids[:16]) and first["q17"] == {d: 1.0 for d in ("d0", "d17", "d150", "d300")}
    for (kind, form, k), r in results.items():
        assert r == results["dicts", "dicts", k], (kind, form, k)
        assert list(r) == qids and [list(h) for h in r.values()] == [list(h) for h in results["dicts", "dicts", k].values()], (kind, form, k)
    for key, (D, I) in lists.items():                                # the numbering does not show in (D, I) either
        assert torch.equal(D, lists["dicts", "dicts"][0]) and torch.equal(I, lists["dicts", "dicts"][1]), key


def test_engine_keeps_one_numbering_until_cleared(engine_case):
    from lightretriever_amd.retriever import ImpactSearch
    from lightretriever_amd.sparse_rows import SparseRows
    rows, dicts, dids, queries, qids = engine_case
    eng = ImpactSearch()
    eng.index(dicts[:50], dids[:50])
    with pytest.raises(ValueError, match="SparseRows after dicts"):
        eng.index(rows[50:60], dids[50:60])
    want = eng.retrieve_with_emb(queries["dicts"], qids, top_k=5)
    eng._clear()
    eng.index(rows[:50], dids[:50])                                  # the other kind after _clear(): the identity numbering from here on
    assert eng.identity_vocab_size == V_ENGINE
    assert eng.retrieve_with_emb(queries["text"], qids, top_k=5) == want == eng.retrieve_with_emb(queries["rows"], qids, top_k=5)
    with pytest.raises(ValueError, match="dicts after SparseRows"):
        eng.index(dicts[50:60], dids[50:60])
    other = SparseRows(rows.row_off[:3].clone(), rows.terms[:int(rows.row_off[2])].clone(), rows.weights[:int(rows.row_off[2])].clone(), V_ENGINE + 1)
    with pytest.raises(ValueError, match="token ids"):
        eng.index(other, ["x", "y"])
    assert eng.impact_index.ntotal == 50 and len(eng.rev_mapping) == 50      # the refused calls left nothing behind
    eng._clear()
    eng.index(dicts[:50], dids[:50])
    assert eng.identity_vocab_size is None and eng.retrieve_with_emb(queries["rows"], qids, top_k=5) == want


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["tok", "spr"])
def test_hybrid_search_csr_equals_json(mode, monkeypatch):
    """HybridSearch(sparse_search="gpu") over the tiny model of the fusion tests, three chunks of 25 documents: sparse_format="csr" returns the
    dicts of sparse_format="json" key for key and score for score, and what reaches ImpactSearch.index is a SparseRows."""
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd.modeling import LrxExactSearchModel, LrxHybridModel
    from lightretriever_amd.retriever import HybridSearch, ImpactSearch
    from lightretriever_amd.sparse_rows import SparseRows
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, _, _ = build_stack(cfg_o, w)
    if mode == "tok":
        hm = LrxHybridModel(enc, normalize=True, pad_token_id=tok.pad_token_id, encode_sparse=True, sparse_top_k_psg=24)
        model = LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=32, p_max_len=64, eval_batch_size_embedding_bag=100)
        model.query_prompt = "query: "
        names = ["emb", "tok", "emb_tok"]
    else:
        hm = LrxHybridModel(enc, normalize=True, pad_token_id=tok.pad_token_id, encode_sparse=True, sparse_top_k_psg=24, hybrid_use_sparse_vector=True,
                            hybrid_use_dense_vector=True, hybrid_use_emb_vector=False, sparse_top_k_qry=12)
        model = LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=32, p_max_len=64)
        names = ["den", "spr", "den_spr"]
    corpus = synth_corpus(np.random.default_rng(2), 60)
    queries = {"q0": "capital of france paris", "q1": "dense retrieval with large language models", "q2": "amd instinct memory search"}
    seen = []
    real_index = ImpactSearch.index

    def spy(self, corpus_emb, corpus_ids):
        seen.append((type(corpus_emb), len(corpus_emb), corpus_emb.device.type if isinstance(corpus_emb, SparseRows) else None))
        return real_index(self, corpus_emb, corpus_ids)
    monkeypatch.setattr(ImpactSearch, "index", spy)
    kw = dict(batch_size=8, corpus_chunk_size=25, fuse_weights=[0.6, 0.4], return_all_results=True, sparse_search="gpu")
    want = HybridSearch(model, **kw).search(corpus, queries, top_k=10)
    assert [t for t, _, _ in seen] == [list] * 3
    del seen[:]
    searcher = HybridSearch(model, sparse_format="csr", **kw)
    got = searcher.search(corpus, queries, top_k=10)
    assert seen == [(SparseRows, 25, "cuda"), (SparseRows, 25, "cuda"), (SparseRows, 10, "cuda")]
    assert list(got) == names == list(want) and all(len(h) > 0 for h in got[names[1]].values())
    for name in names:
        assert got[name] == want[name], name
        assert [list(h.items()) for h in got[name].values()] == [list(h.items()) for h in want[name].values()], name
    # the encoder surface on its own: same vectors in either format, queries as rows without pseudo text
    docs = list(corpus.values())[:11]
    js, cs = (model.encode_corpus(docs, batch_size=4, sparse_format=f)["sparse_reps"] for f in ("json", "csr"))
    assert isinstance(cs, SparseRows) and cs.device.type == "cuda" and cs.to_dicts() == js and model.encode_corpus(docs, batch_size=4)["sparse_reps"] == js
    if mode == "spr":
        qj, qc = (model.encode_queries(list(queries.values()), batch_size=2, sparse_format=f)["sparse_reps"] for f in ("json", "csr"))
        assert isinstance(qc, SparseRows) and len(qc) == 3
        assert [" ".join(t for t, c in d.items() for _ in range(c)) for d in qc.to_dicts()] == qj
    with pytest.raises(ValueError, match="sparse_format"):
        model.encode_corpus(docs, batch_size=4, sparse_format="coo")


# ---- torch op ----------------------------------------------------------------------------------------------------------------------
def test_torch_op_and_graph_capture():
    from lightretriever_amd import _lib, ops, torch_ops  # noqa: F401
    V = 1500
    reps = device_rows(case_rows(V, 100), V)
    for marker in (True, False):
        want = ops.sparse_compact_csr(reps, 100, empty_marker=marker)
        got = torch.ops.lrx.sparse_compact_csr(reps, 100, marker)
        assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(got, (want.row_off, want.terms, want.weights)))
    off, terms, weights = torch.ops.lrx.sparse_compact_csr(torch.zeros(0, 8, device="cuda"), 100, True)
    assert off.tolist() == [0] and terms.numel() == weights.numel() == 0
    torch.cuda.synchronize()
    # the length of the result is read back to the host: refused under capture before anything is launched (one eager call has run above)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.LrxError, match="graph capture"):
        with torch.cuda.graph(g):
            ops.sparse_compact_csr(reps, 100)
    del g
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="graph capture"):         # the op layer reports through TORCH_CHECK like all of its ops
        with torch.cuda.graph(g):
            torch.ops.lrx.sparse_compact_csr(reps, 100, True)
    del g
    torch.cuda.synchronize()
    again = ops.sparse_compact_csr(reps, 100, empty_marker=False)                                 # the stream is usable afterwards
    assert torch.equal(again.terms, want.terms) and torch.equal(again.row_off, want.row_off)
