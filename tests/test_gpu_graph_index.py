"""GPU: the graph index (lrx_graph_ip_search, lrx_graph_detour_counts, GraphFlatIndex, HNSWFaissSearch) against the Python model
(tests/graph_yardstick.py), bit for bit: ids, scores and the step count of the traversal over score tables taken from lrx_flat_ip_rerank, heavy
ties, a visited table that had to forget, the edges (padding, rows that do not exist, strides, ids), batch independence, the detour counts, the
build, persistence, the searcher and the workspace contract.  Observed figures: DESIGN §5.4.17."""
import numpy as np
import pytest
import torch

import graph_yardstick as Y
from ws_guard import Guarded

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
TABLE_ROWS = 3072                 # what the kernel's visited table holds before it forgets (GRAPH_HASH_FILL, csrc/lrx_search_graph.h)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def errors(reset=True):
    from lightretriever_amd import _lib
    torch.cuda.synchronize()
    return int(_lib.lib().lrx_device_error_count(1 if reset else 0))


def score_table(x, q):
    """S fp32 [Q, n]: the score lrx_flat_ip_rerank reports for every (query, row), 2048 candidates per call."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    X, qd = dev(x), dev(q)
    (n, d), Q = x.shape, q.shape[0]
    S = torch.empty(Q, n, dtype=torch.float32, device="cuda")
    for c0 in range(0, n, 2048):
        nc = min(2048, n - c0)
        cand = torch.arange(c0, c0 + nc, dtype=torch.int64, device="cuda").repeat(Q, 1)
        Do = torch.empty(Q, nc, dtype=torch.float32, device="cuda")
        Io = torch.empty(Q, nc, dtype=torch.int64, device="cuda")
        ws = torch.empty(l.lrx_ip_rerank_workspace_bytes(Q, nc, nc), dtype=torch.uint8, device="cuda")
        _lib.check(l.lrx_flat_ip_rerank(_lib.ptr(X), n, d, d, _lib.ptr(qd), Q, _lib.ptr(cand), nc, nc, nc, 0, _lib.ptr(Do), _lib.ptr(Io), None, _lib.ptr(ws),
                                        ws.numel(), _lib.current_stream()))
        S.scatter_(1, Io, Do)
    return S.cpu().numpy()


def graph_search(x, graph, q, entries, k, beam, width, max_it=0, id_base=0, row_map=None, n_rows=None, guard=None):
    """lrx_graph_ip_search through ctypes with ldx = d + 8 (padding columns 1e30: never read into a result) and ld_entry = n_entry + 3 (padding
    entries name row 0: read, they would be starts).  guard: a ws_guard.Guarded whose inner block is the workspace."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    x, graph, q, entries = (t if isinstance(t, torch.Tensor) else dev(t) for t in (x, graph, q, entries))
    (Q, d), n, ne = q.shape, x.shape[0], entries.shape[1]
    xb = torch.full((n, d + 8), 1e30, dtype=torch.float32, device="cuda")
    xb[:, :d] = x
    eb = torch.zeros(Q, ne + 3, dtype=torch.int64, device="cuda")
    eb[:, :ne] = entries
    Do = torch.full((Q, k), 7.5, dtype=torch.float32, device="cuda")
    Io = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    So = torch.full((Q, 2), -7, dtype=torch.int32, device="cuda")
    need = int(l.lrx_graph_ip_workspace_bytes(Q, ne, graph.shape[1], beam, width))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if guard is None else guard.ws
    assert ws.numel() == need
    ws_ptr = None if need == 0 else _lib.ptr(ws)
    _lib.check(l.lrx_graph_ip_search(_lib.ptr(xb), n if n_rows is None else n_rows, d + 8, d, _lib.ptr(graph.contiguous()), graph.shape[1],
                                     _lib.ptr(q.contiguous()) if Q else None, Q, _lib.ptr(eb) if Q else None, ne, ne + 3, k, beam, width, max_it, id_base,
                                     _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(row_map), _lib.ptr(So), ws_ptr, need, _lib.current_stream()))
    torch.cuda.synchronize()
    return Do.cpu().numpy(), Io.cpu().numpy(), So.cpu().numpy()


def model_search(S, graph, entries, k, beam, width, max_it=0):
    out = [Y.beam_search(S[i], graph, entries[i], k, beam, width, max_it) for i in range(S.shape[0])]
    return (np.stack([o[1] for o in out]), np.stack([o[0] for o in out]), np.array([[o[2], o[3]] for o in out], dtype=np.int32))


def assert_model(got, want, width, degree, n_entry, ids=None):
    """ids, score bits and step counts are the model's; rows scored too while the kernel's table cannot have filled, no fewer after that."""
    D, I, St = got
    assert np.array_equal(I, want[1] if ids is None else ids)
    assert np.array_equal(D.view(np.int32), want[0].view(np.int32))
    assert np.array_equal(St[:, 0], want[2][:, 0])
    fits = want[2][:, 1] + max(width * degree, min(n_entry, 1024)) <= TABLE_ROWS
    assert np.array_equal(St[fits, 1], want[2][fits, 1]) and (St[:, 1] >= want[2][:, 1]).all()


def built(x, degree, K, **kw):
    from lightretriever_amd import GraphFlatIndex
    idx = GraphFlatIndex(x.shape[1], degree=degree, intermediate_degree=K, **kw)
    idx.add(x)
    idx._finalize()
    return idx


def entries_of(S, n, n_entry, m):
    rows = Y.entry_rows(n, n_entry)
    return np.stack([Y.best_entries(S[i], rows, m) for i in range(S.shape[0])])


# ---- the issue's corpus: n = 4096, d = 64, 64 Gaussian clusters; 33 queries; the score table of the rerank ---------------------------------
@pytest.fixture(scope="module")
def corpus():
    x, q = Y.clustered_corpus(4096, 64, 64, 1000, seed=0)
    idx = built(x, 16, 32, n_entry=512)
    return dict(x=x, q=q, idx=idx, graph=idx.graph.cpu().numpy(), S=score_table(x, q[:33]))


@pytest.mark.parametrize("beam,width,k,max_it", [(64, 4, 10, 0), (128, 4, 100, 0), (1, 1, 1, 0), (64, 4, 10, 3)])
def test_search_equals_the_model(corpus, beam, width, k, max_it):
    S, graph = corpus["S"], corpus["graph"]
    ent = entries_of(S, 4096, 512, min(beam, 512))
    got = graph_search(corpus["x"], graph, corpus["q"][:33], ent, k, beam, width, max_it)
    want = model_search(S, graph, ent, k, beam, width, max_it)
    assert_model(got, want, width, 16, ent.shape[1])
    if max_it:
        assert (got[2][:, 0] == max_it).all()                     # the cap was what stopped every query
    else:
        assert (got[2][:, 0] < -(-beam // width) + 32).all()      # ... and here it was not


@pytest.fixture(scope="module")
def wide(corpus):
    """The same rows under degree 128 (K = 128): with width 8 one step gathers up to 1024 rows."""
    return built(corpus["x"], 128, 128, n_entry=512).graph.cpu().numpy()


def test_search_where_one_step_brings_more_rows_than_the_beam_holds(corpus, wide):
    S = corpus["S"][:9]
    ent = entries_of(S, 4096, 512, 16)
    got = graph_search(corpus["x"], wide, corpus["q"][:9], ent, 16, 16, 8)
    assert_model(got, model_search(S, wide, ent, 16, 16, 8), 8, 128, 16)


def test_search_after_the_visited_table_forgot(corpus, wide):
    """beam 1024, width 8, degree 128 over 4096 rows: a query meets nearly the whole corpus, more than the 3072 rows the kernel's table holds, and
    a step may bring 1024 -- so the table is cleared several times (rows scored > the exact-set model's) and ids, scores and steps are still
    the model's."""
    S = corpus["S"][:4]
    ent = entries_of(S, 4096, 512, 512)
    got = graph_search(corpus["x"], wide, corpus["q"][:4], ent, 100, 1024, 8)
    want = model_search(S, wide, ent, 100, 1024, 8)
    assert (want[2][:, 1] > TABLE_ROWS).all()
    assert_model(got, want, 8, 128, 512)
    assert (got[2][:, 1] > want[2][:, 1]).all()


def test_entry_list_longer_than_one_slice(corpus):
    S, graph = corpus["S"][:5], corpus["graph"]
    ent = entries_of(S, 4096, 2048, 2048)                         # 2048 entries: two slices of 1024, merged into a beam of 2048
    got = graph_search(corpus["x"], graph, corpus["q"][:5], ent, 50, 2048, 8, 2)
    assert_model(got, model_search(S, graph, ent, 50, 2048, 8, 2), 8, 16, 2048)


# ---- ties: every score an exact small integer ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ties():
    rng = np.random.default_rng(5)
    x = rng.integers(-1, 2, (1024, 32)).astype(np.float32)
    q = rng.integers(-1, 2, (33, 32)).astype(np.float32)
    return dict(x=x, q=q, idx=built(x, 8, 16, n_entry=64), S=score_table(x, q))


def test_ties_go_to_the_lower_row_in_the_beam_and_in_the_output(ties):
    S, graph = ties["S"], ties["idx"].graph.cpu().numpy()
    assert len(np.unique(S)) < 40 and np.array_equal(S, np.round(S))
    for beam, width, k in ((32, 2, 32), (8, 1, 5)):
        ent = entries_of(S, 1024, 64, min(beam, 64))
        got = graph_search(ties["x"], graph, ties["q"], ent, k, beam, width)
        assert_model(got, model_search(S, graph, ent, k, beam, width), width, 8, ent.shape[1])


def test_knn_lists_equal_the_model_under_ties(ties):
    from lightretriever_amd import graph as G
    S = score_table(ties["x"], ties["x"])
    assert np.array_equal(G.knn_lists(ties["idx"].store, 16).cpu().numpy(), Y.knn_lists(S, 16))


# ---- edges ------------------------------------------------------------------------------------------------------------------------------------
def test_one_row_and_padding():
    x = np.ones((1, 32), dtype=np.float32)
    graph = np.full((1, 8), -1, dtype=np.int32)
    D, I, St = graph_search(x, graph, x, np.array([[0, 0, -1]]), 3, 4, 2)
    assert I.tolist() == [[0, -1, -1]] and D.tolist() == [[32.0, -FLT_MAX, -FLT_MAX]] and St.tolist() == [[1, 1]]
    D, I, St = graph_search(x, graph, np.zeros((0, 32), np.float32), np.zeros((0, 3), np.int64), 3, 4, 2)       # no queries: nothing is launched
    assert D.shape == (0, 3) and I.shape == (0, 3)


def test_fewer_rows_than_the_degree():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((9, 64)).astype(np.float32)
    idx = built(x, 16, 16)
    graph = idx.graph.cpu().numpy()
    assert (graph[:, 8:] == -1).all() and all(sorted(graph[u, :8].tolist()) == [v for v in range(9) if v != u] for u in range(9))
    q = rng.standard_normal((4, 64)).astype(np.float32)
    S = score_table(x, q)
    ent = entries_of(S, 9, 3, 3)
    got = graph_search(x, graph, q, ent, 12, 12, 2)
    assert_model(got, model_search(S, graph, ent, 12, 12, 2), 2, 16, 3)
    assert (got[1][:, :9] >= 0).all() and (got[1][:, 9:] == -1).all()


def test_entries_that_name_no_row_and_rows_that_do_not_exist(corpus):
    S, graph, x, q = corpus["S"][:6], corpus["graph"], corpus["x"], corpus["q"][:6]
    ent = entries_of(S, 4096, 512, 64)
    errors()
    D, I, St = graph_search(x, graph, q, np.full((6, 5), -1, dtype=np.int64), 4, 8, 2)
    assert (I == -1).all() and (D == -FLT_MAX).all() and (St == 0).all() and errors() == 0
    # an entry >= n_rows, planted in a copy: skipped, counted, the rest as the model has it
    bad = ent.copy()
    bad[:, 7] = 4096 + np.arange(6)
    got = graph_search(x, graph, q, bad, 10, 64, 4)
    assert errors() == 6
    assert_model(got, model_search(S, graph, bad, 10, 64, 4), 4, 16, 64)
    # a graph entry >= n_rows, planted in a copy, in rows the searches pass through: each query's best hit
    want = model_search(S, graph, ent, 10, 64, 4)
    g2 = graph.copy()
    g2[want[1][:, 0], 3] = 4096 + 17
    got = graph_search(x, g2, q, ent, 10, 64, 4)
    assert errors() >= 1
    assert_model(got, model_search(S, g2, ent, 10, 64, 4), 4, 16, 64)
    # the same rows cut off by n_rows itself: rows >= 3000 are never read
    low = np.where(graph >= 3000, -1, graph)
    got = graph_search(x, graph, q, ent, 10, 64, 4, n_rows=3000)
    assert errors() > 0 and (got[1] < 3000).all()
    assert_model(got, model_search(S[:, :3000], low[:3000], np.where(ent >= 3000, -1, ent), 10, 64, 4), 4, 16, 64)


def test_ids_through_id_base_and_row_map(corpus):
    S, graph, x, q = corpus["S"][:5], corpus["graph"], corpus["x"], corpus["q"][:5]
    ent = entries_of(S, 4096, 512, 64)
    want = model_search(S, graph, ent, 70, 80, 4)
    assert (want[1] >= 0).all()
    got = graph_search(x, graph, q, ent, 70, 80, 4, id_base=10 ** 10)
    assert_model(got, want, 4, 16, 64, ids=want[1] + 10 ** 10)
    row_map = torch.arange(4096, dtype=torch.int64, device="cuda").flip(0) * 3 + 1
    got = graph_search(x, graph, q, ent, 70, 80, 4, id_base=55, row_map=row_map)
    assert_model(got, want, 4, 16, 64, ids=(4095 - want[1]) * 3 + 1)


def test_query_rows_too_long_for_lds():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((256, 8192)).astype(np.float32)
    q = rng.standard_normal((3, 8192)).astype(np.float32)
    idx = built(x, 8, 16, n_entry=16)
    S, graph = score_table(x, q), idx.graph.cpu().numpy()
    ent = entries_of(S, 256, 16, 16)
    assert_model(graph_search(x, graph, q, ent, 10, 24, 2), model_search(S, graph, ent, 10, 24, 2), 2, 8, 16)
    D, I = idx.search(q, 10, ef_search=24)
    assert np.array_equal(I.cpu().numpy(), model_search(S, graph, ent, 10, 24, 4)[1])


# ---- independence -------------------------------------------------------------------------------------------------------------------------------
def test_a_query_does_not_depend_on_its_batch(corpus):
    idx, q = corpus["idx"], dev(corpus["q"])
    D, I = idx.search(q, 10)
    D1, I1 = idx.search(q[17:18], 10)
    assert torch.equal(I[17:18], I1) and torch.equal(D[17:18].view(torch.int32), D1.view(torch.int32))
    D2, I2 = idx.search(q[10:33], 10)
    assert torch.equal(I[10:33], I2) and torch.equal(D[10:33].view(torch.int32), D2.view(torch.int32))


# ---- the build --------------------------------------------------------------------------------------------------------------------------------------
def random_lists(n, K, seed):
    rng = np.random.default_rng(seed)
    knn = np.full((n, K), -1, dtype=np.int32)
    for u in range(n):
        others = rng.permutation(np.delete(np.arange(n), u))[:K]
        knn[u, :others.shape[0]] = others
    return knn


@pytest.mark.parametrize("n,K", [(300, 64), (600, 256), (20, 32), (70, 1), (65, 100)])
def test_detour_kernel_equals_the_yardstick(n, K):
    from lightretriever_amd import ops
    knn = random_lists(n, K, seed=n)
    want = Y.detour_counts(knn)
    assert want.sum() > 0 or K == 1
    assert np.array_equal(ops.graph_detour_counts(dev(knn)).cpu().numpy(), want)


def test_build_equals_the_yardstick_from_the_same_lists(corpus):
    from lightretriever_amd import graph as G, ops
    idx = corpus["idx"]
    knn = G.knn_lists(idx.store, 32)
    h = knn.cpu().numpy()
    assert (h >= 0).all() and (h != np.arange(4096)[:, None]).all() and all(len(set(r)) == 32 for r in h[:64].tolist())
    counts = Y.detour_counts(h)
    assert np.array_equal(ops.graph_detour_counts(knn).cpu().numpy(), counts)
    pruned = Y.prune(h, counts, 16)
    assert np.array_equal(G.prune(knn, dev(counts), 16).cpu().numpy(), pruned)
    assert np.array_equal(corpus["graph"], Y.merge_reverse(pruned))
    assert np.array_equal(idx.entry_rows.cpu().numpy(), Y.entry_rows(4096, 512)) and idx._entries.ntotal == 512
    assert set(idx.build_times) == {"knn", "detours", "prune_merge"}


# ---- the index ----------------------------------------------------------------------------------------------------------------------------------------
def test_index_search_equals_the_model_and_reaches_the_recall_of_the_model(corpus):
    idx, S, q = corpus["idx"], corpus["S"], corpus["q"][:33]
    errors()
    for k, ef in ((10, 64), (100, 128), (100, 20)):               # beam = max(ef_search, k)
        beam = max(ef, k)
        D, I = idx.search(q, k, ef_search=ef)
        want = model_search(S, corpus["graph"], entries_of(S, 4096, 512, min(beam, 512)), k, beam, 4)
        assert np.array_equal(I.cpu().numpy(), want[1]) and np.array_equal(D.cpu().numpy().view(np.int32), want[0].view(np.int32))
    exact = np.stack([Y.ranking(Y.score_keys(S[i]))[:10] for i in range(33)])
    got = idx.search(q, 10, ef_search=64)[1].cpu().numpy()
    assert np.mean([len(set(a) & set(b)) / 10 for a, b in zip(got.tolist(), exact.tolist())]) >= 0.95
    assert errors(reset=False) == 0
    with pytest.raises(NotImplementedError, match="range_search"):
        idx.range_search(q, 0.5)
    with pytest.raises(NotImplementedError, match="sel"):
        idx.search(q, 10, sel=object())
    with pytest.raises(ValueError, match="ef_search=4000"):
        idx.search(q, 10, ef_search=4000)


def test_every_row_in_the_start_beam_equals_the_flat_search(corpus):
    from lightretriever_amd import FlatIPIndex
    x, q = corpus["x"][:512], corpus["q"][:40]
    idx = built(x, 16, 32, n_entry=512, ef_search=512, id_base=1000)
    flat = FlatIPIndex(64, id_base=1000)
    flat.add(x)
    for k in (1, 100, 512):
        D, I = idx.search(q, k)
        Df, If = flat.search(q, k)
        assert torch.equal(I, If) and torch.equal(D.view(torch.int32), Df.view(torch.int32))


def test_rows_added_after_a_search_are_found_and_slots_work(corpus):
    from lightretriever_amd import GraphFlatIndex
    x, q = corpus["x"][:600], corpus["q"][:8]
    idx = GraphFlatIndex(64, degree=16, intermediate_degree=32, ef_search=64)
    assert idx.search(q, 3)[1].tolist() == [[-1] * 3] * 8 and idx.ntotal == 0                    # an empty index: padding
    idx.add(x[:500])
    first = idx.search(q, 5)[1]
    assert idx.graph.shape == (500, 16) and int(first.max()) < 500
    slot = idx.append_slot(101)
    slot[:100].copy_(dev(x[500:600]))
    slot[100].copy_(dev(q[3] * 4))                                                              # a row no other can outscore for query 3
    idx.commit(101)
    D, I = idx.search(q, 5)
    assert idx.graph.shape == (601, 16) and idx.ntotal == 601 and int(I[3, 0]) == 600
    whole = built(np.concatenate([x, q[3:4] * 4]), 16, 32, ef_search=64)
    assert torch.equal(whole.graph, idx.graph) and torch.equal(whole.search(q, 5)[1], I)
    assert torch.equal(idx.reconstruct_n(598, 3), dev(np.concatenate([x[598:600], q[3:4] * 4])))
    idx.reset()
    assert idx.ntotal == 0 and idx.graph is None and idx.search(q, 2)[1].tolist() == [[-1, -1]] * 8


def test_save_load_round_trip(corpus, tmp_path):
    from lightretriever_amd import FlatIPIndex, GraphFlatIndex
    from lightretriever_amd import graph as G
    x, q = corpus["x"][:700], corpus["q"][:16]
    idx = built(x, 16, 48, n_entry=100, ef_search=40, search_width=2)
    f = str(tmp_path / "g.hnsw.faiss")
    idx.save(f)
    back = GraphFlatIndex.load(f, id_base=7)
    assert (back.d, back.degree, back.intermediate_degree, back.ef_search, back.search_width, back.n_entry, back.ntotal) == (64, 16, 48, 40, 2, 100, 700)
    assert torch.equal(back.graph, idx.graph) and torch.equal(back.entry_rows, idx.entry_rows) and torch.equal(back.vectors, idx.vectors)
    D, I = idx.search(q, 20)
    Db, Ib = back.search(q, 20)
    assert torch.equal(Ib, I + 7) and torch.equal(Db.view(torch.int32), D.view(torch.int32))
    assert FlatIPIndex.load(f).ntotal == 700                                                    # the main file is the flat record
    # a side file that belongs to other rows is refused
    st = G.read_graph_file(f)
    G.write_graph_file(f, np.where(st["graph"][:699] >= 699, -1, st["graph"][:699]), st["entry_rows"], {p: st[p] for p in G.PARAMS} | {"ntotal": 699})
    with pytest.raises(ValueError, match="built for 699 rows, but the store holds 700"):
        GraphFlatIndex.load(f)
    with pytest.raises(ValueError, match="int32"):
        idx.set_graph(st["graph"][:, :8], st["entry_rows"])


class TableModel:
    """encode_corpus / encode_queries by lookup: the embeddings are the test's own."""

    def __init__(self, table):
        self.table = table

    def _rows(self, texts):
        return torch.stack([self.table[t["text"] if isinstance(t, dict) else t] for t in texts]).cuda()

    def encode_queries(self, queries, **kw):
        return {"dense_reps": self._rows(queries)}

    def encode_corpus(self, corpus, **kw):
        return {"dense_reps": self._rows(corpus)}


def test_searcher_over_two_chunks(corpus, tmp_path):
    """Chunks of 100 rows under ef_search 128 with every row an entry: each chunk's beam holds the whole chunk, so the searcher must return the
    flat searcher's dict -- the reference's shape, {qid: {pid: score}}."""
    from lightretriever_amd import GraphFlatIndex
    from lightretriever_amd.retriever import FaissHNSWIndex, FlatIPFaissSearch, HNSWFaissSearch, HybridSearch
    emb, qemb = corpus["x"][:200], corpus["q"][:6]
    ids = [f"d{i:03d}" for i in range(200)]
    docs = {pid: {"text": "x" * (300 - j) + pid} for j, pid in enumerate(ids)}
    qs = {f"q{i}": f"query {i}" for i in range(6)}
    table = {docs[pid]["text"]: torch.from_numpy(emb[j]) for j, pid in enumerate(ids)}
    table.update({t: torch.from_numpy(qemb[i]) for i, t in enumerate(qs.values())})
    model = TableModel(table)
    want = FlatIPFaissSearch(model, batch_size=8, corpus_chunk_size=100, show_progress_bar=False).search(docs, qs, top_k=12)
    h = HybridSearch(model, batch_size=8, corpus_chunk_size=100, faiss_search_map="graph", hnsw_store_n=8, show_progress_bar=False)
    assert isinstance(h.dense_search, HNSWFaissSearch)
    got = h.search(docs, qs, top_k=12)
    assert got == want and all(len(v) == 12 and all(isinstance(s, float) for s in v.values()) for v in got.values())
    s = HNSWFaissSearch(model, batch_size=8, hnsw_store_n=8, hnsw_ef_search=50, hnsw_ef_construction=40, show_progress_bar=False)
    s.index(torch.from_numpy(emb), ids)
    idx = s.faiss_index.index
    assert type(s.faiss_index) is FaissHNSWIndex and type(idx) is GraphFlatIndex
    assert (idx.degree, idx.intermediate_degree, idx.ef_search, idx.ntotal, s.dim_size) == (16, 40, 50, 200, 64)
    qd = dev(qemb)
    res = s.retrieve_with_emb(qd, list(qs), 12)
    s.save(str(tmp_path), "p")
    assert (tmp_path / "p.hnsw.faiss").exists() and (tmp_path / "p.hnsw.faiss.graph.npz").exists() and (tmp_path / "p.hnsw.tsv").exists()
    t = HNSWFaissSearch(model, batch_size=8, show_progress_bar=False)
    t.load(str(tmp_path), "p")
    assert (t.hnsw_store_n, t.hnsw_ef_search, t.hnsw_ef_construction) == (8, 50, 40)
    assert t.retrieve_with_emb(qd, list(qs), 12) == res
    small = HNSWFaissSearch(model, batch_size=8, show_progress_bar=False)                       # the reference's defaults over a 20-row chunk
    small.index(torch.from_numpy(emb[:20]), ids[:20])
    assert (small.faiss_index.index.degree, small.faiss_index.index.intermediate_degree) == (16, 20)
    assert len(small.retrieve_with_emb(qd, list(qs), 5)["q0"]) == 5


# ---- the workspace ----------------------------------------------------------------------------------------------------------------------------------
def test_workspace_is_exactly_the_declared_bytes_and_may_be_dirty(corpus):
    """The entry between guard bands, its block zero-filled, 0xFF-filled and left over from a larger call: the same results, the guards intact.
    (The traversal keeps its state in LDS, so the declared size is 0 today and the two bands touch; the test holds for any size.)"""
    from lightretriever_amd import _lib
    S, graph, x, q = corpus["S"][:7], corpus["graph"], corpus["x"], corpus["q"][:7]
    ent = entries_of(S, 4096, 512, 64)
    want = model_search(S, graph, ent, 10, 64, 4)
    need = int(_lib.lib().lrx_graph_ip_workspace_bytes(7, 64, 16, 64, 4))
    big = int(_lib.lib().lrx_graph_ip_workspace_bytes(33, 512, 16, 128, 4))
    assert big >= need
    for fill in ("0x00", "0xFF", "larger call"):
        g = Guarded(need, "cuda")
        if fill == "larger call":
            gb = Guarded(big, "cuda").fill(0x5A).arm()
            graph_search(x, graph, corpus["q"][:33], entries_of(corpus["S"], 4096, 512, 128), 100, 128, 4, guard=gb)
            assert gb.check().numel() == 0
            g.fill(gb.ws[:need].clone())
        else:
            g.fill(int(fill, 16))
        g.arm()
        got = graph_search(x, graph, q, ent, 10, 64, 4, guard=g)
        assert g.check().numel() == 0, fill
        assert_model(got, want, 4, 16, 64)
