"""CPU side of the graph index (GraphFlatIndex, lrx_graph_ip_search / lrx_graph_detour_counts): the model of the build and of the
beam search (tests/graph_yardstick.py) on hand-worked cases, the licence the kernel's forgetting visited set rests on, the recall condition of
the algorithm itself, the searcher's argument mapping and routes, the argument checks of both C entries and the side file's refusals -- none of
which needs a GPU."""
import ctypes
import os

import numpy as np
import pytest

from lightretriever_amd import _lib, build
from lightretriever_amd import graph as G

import graph_yardstick as Y

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the build on cases small enough to work by hand -------------------------------------------------------------------------------
def test_detour_counts_of_a_hand_worked_example():
    knn = np.array([[1, 2, 3], [2, 3, 0], [3, 1, 0], [2, 4, 5], [3, 5, 1], [4, 3, -1]], dtype=np.int32)
    # row 0 = [1, 2, 3]: 0 -> 1 -> 2 (a = 0, b = 0) reaches position 1; 0 -> 1 -> 3 (0, 1) and 0 -> 2 -> 3 (1, 0) reach position 2; 0 -> 2 -> 1 lands on
    # position 0 < a and counts nowhere.  Row 1 = [2, 3, 0]: 1 -> 2 -> 3 reaches position 1; 1 -> 2 -> 0 has b = 2 = c: not a detour.
    # Row 3 = [2, 4, 5]: 3 -> 4 -> 5 (1, 1) reaches position 2.  Row 5 = [4, 3, -1]: 5 -> 4 -> 3 (0, 0) reaches position 1; the empty slot takes no part.
    want = [[0, 1, 2], [0, 1, 0], [0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 1, 0]]
    assert Y.detour_counts(knn).tolist() == want
    n, K = knn.shape
    brute = np.zeros((n, K), dtype=np.int32)
    for u in range(n):
        for a in range(K):
            for b in range(K):
                v = knn[u, a]
                w = knn[v, b] if v >= 0 else -1
                hits = [c for c in range(K) if w >= 0 and knn[u, c] == w]
                if hits and hits[0] > max(a, b):
                    brute[u, hits[0]] += 1
    assert brute.tolist() == want


def test_prune_and_merge_with_a_duplicate_between_pruned_and_reverse_edges():
    knn = np.array([[1, 2, 3, 4], [0, 2, 3, 5], [0, 1, 3, 4], [0, 1, 2, 5], [0, 2, 5, 1], [1, 3, 4, 0]], dtype=np.int32)
    counts = Y.detour_counts(knn)
    assert counts.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 2, 0], [0, 0, 0, 3], [0, 0, 0, 3]]
    pruned = Y.prune(knn, counts, 4)
    # fewest detours first, ties to the lower position: row 2 (counts 0 1 0 0) -> positions 0 2 3 1, row 3 (0 1 2 0) -> 0 3 1 2
    assert pruned.tolist() == [[1, 2, 3, 4], [0, 2, 3, 5], [0, 3, 4, 1], [0, 5, 1, 2], [0, 2, 5, 1], [1, 3, 4, 0]]
    assert Y.prune(knn, counts, 2).tolist() == [[1, 2], [0, 2], [0, 3], [0, 5], [0, 2], [1, 3]]
    # rev (two entries each, by (position, u)): rev[0] = [1, 2], rev[1] = [0, 5], rev[2] = [0, 1], rev[3] = [2, 5], rev[4] = [2, 5], rev[5] = [3, 4];
    # graph[1] = [0, 2] ++ [0, 5] ++ [3, 5] -> 0 2 5 3 (0 and 5 named twice); graph[3] = [0, 5] ++ [2, 5] ++ [1, 2] -> 0 5 2 1
    assert Y.merge_reverse(pruned).tolist() == [[1, 2, 3, 4], [0, 2, 5, 3], [0, 3, 1, 4], [0, 5, 2, 1], [0, 2, 5, 1], [1, 3, 4, 0]]


def test_prune_and_merge_with_fewer_rows_than_the_list_length():
    knn = np.array([[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]], dtype=np.int32)          # n - 1 = 2 < K = 4
    counts = Y.detour_counts(knn)
    assert counts.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]]                        # 2 -> 1 -> 0
    pruned = Y.prune(knn, counts, 4)
    assert pruned.tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]]                  # empty slots after every row, whatever their count
    assert Y.merge_reverse(pruned).tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]]


def test_knn_lists_drop_the_row_itself_or_the_last_entry():
    S = np.array([[9, 1, 2, 3], [1, 9, 5, 5], [7, 7, 7, 7], [0, 2, 1, -5]], dtype=np.float32)
    # row 2 ties with everything: the lower rows first, itself dropped; row 3 does not reach its own top 3 (its self-score is the lowest): the last goes
    assert Y.knn_lists(S, 2).tolist() == [[3, 2], [2, 3], [0, 1], [1, 2]]
    assert Y.knn_lists(S, 5).tolist() == [[3, 2, 1, -1, -1], [2, 3, 0, -1, -1], [0, 1, 3, -1, -1], [1, 2, 0, -1, -1]]
    assert Y.entry_rows(10, 4).tolist() == [0, 2, 5, 7] and G.entry_row_numbers(10, 4).tolist() == [0, 2, 5, 7]


# ---- the model of the search on the issue's corpus -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """n = 4096, d = 64, 64 Gaussian clusters, 64 queries; K = 32, R = 16, 512 entry rows: the graph and the score table, built once."""
    x, q = Y.clustered_corpus(4096, 64, 64, 64, seed=0)
    knn = Y.knn_lists((x @ x.T).astype(np.float32), 32)
    return dict(graph=Y.build_graph(knn, 16), S=(q @ x.T).astype(np.float32), entries=Y.entry_rows(4096, 512), knn=knn)


def _recall(model, k, beam):
    hits = []
    for i in range(model["S"].shape[0]):
        row = model["S"][i]
        ids = Y.beam_search(row, model["graph"], Y.best_entries(row, model["entries"], min(beam, 512)), k, beam, 4)[0]
        hits.append(len(set(ids.tolist()) & set(Y.ranking(Y.score_keys(row))[:k].tolist())) / k)
    return float(np.mean(hits)), float(np.min(hits))


def test_recall_condition_on_the_model(model):
    mean10, min10 = _recall(model, 10, 64)
    mean100, min100 = _recall(model, 100, 128)
    print(f"recall@10 beam 64: mean {mean10:.3f} min {min10:.3f}; recall@100 beam 128: mean {mean100:.3f} min {min100:.3f}")
    assert mean10 >= 0.95
    assert mean100 >= 0.90


def test_a_visited_set_that_forgets_changes_nothing_but_the_rows_scored(model):
    """The licence of the kernel's fixed-size table: cutting the visited set down to the beam's rows, at any steps, gives the same ids, scores
    and step count as the exact set -- a forgotten row is scored again and dropped again -- and only `rows scored` can grow."""
    more = 0
    for i in range(64):
        row = model["S"][i]
        ent = Y.best_entries(row, model["entries"], 64)
        exact = Y.beam_search(row, model["graph"], ent, 10, 64, 4)
        for forget_at in (range(0, 100), (1, 5, 6), (exact[2] - 1,)):
            got = Y.beam_search(row, model["graph"], ent, 10, 64, 4, forget_at=tuple(forget_at))
            assert np.array_equal(got[0], exact[0]) and np.array_equal(got[1], exact[1]) and got[2] == exact[2], (i, forget_at)
            assert got[3] >= exact[3]
            more += got[3] - exact[3]
    assert more > 0                                  # the variant did forget something on the way


def test_beam_search_model_edges():
    graph = np.array([[1, 2], [0, 2], [0, 1], [-1, -1]], dtype=np.int32)
    row = np.array([1, 3, 3, 9], dtype=np.float32)
    ids, sc, steps, scored = Y.beam_search(row, graph, [0, -1, 7, 0], 3, 2, 1)         # padding, a row that does not exist, a duplicate
    assert ids.tolist() == [1, 2, -1] and sc[:2].tolist() == [3, 3] and sc[2] == -np.finfo(np.float32).max   # ties to the lower row; row 3 unreachable
    assert (steps, scored) == (3, 3)                 # 0, then 1 and 2: each expanded once
    assert Y.beam_search(row, graph, [0], 3, 2, 1, max_iterations=1)[2] == 1
    assert Y.beam_search(row, graph, [-1, -1], 2, 2, 1)[0].tolist() == [-1, -1]
    assert Y.score_keys(np.array([-1.0, 0.0, 2.0, -3.0], np.float32)).argsort().tolist() == [3, 0, 1, 2]


# ---- searcher: argument mapping, routes, shims ------------------------------------------------------------------------------------------
def test_searcher_argument_mapping_and_refusals():
    from lightretriever_amd.retriever import FaissHNSWIndex, FaissIndex, HNSWFaissSearch
    s = HNSWFaissSearch(None)                        # the reference's defaults: hnsw_store_n 512, efSearch 128, efConstruction 200
    assert (s.hnsw_store_n, s.hnsw_ef_search, s.hnsw_ef_construction, s.batch_size) == (512, 128, 200, 128)
    assert s._degrees() == (64, 200)
    assert HNSWFaissSearch(None, hnsw_store_n=8)._degrees() == (16, 200)
    assert HNSWFaissSearch(None, hnsw_store_n=3)._degrees() == (8, 200)
    assert HNSWFaissSearch(None, hnsw_store_n=16, hnsw_ef_construction=40)._degrees() == (32, 64)
    assert HNSWFaissSearch(None, hnsw_ef_construction=1000)._degrees() == (64, 256)
    assert s._degrees(1000) == (64, 200) and s._degrees(100) == (64, 100) and s._degrees(20) == (16, 20) and s._degrees(5) == (8, 8)   # a chunk's rows
    assert s.index_ext == "hnsw" and s.get_index_name() == "hnsw_faiss_index" and s.serves_rpc_shards is False
    assert s.faiss_index_cls is FaissHNSWIndex and issubclass(FaissHNSWIndex, FaissIndex) and s.index_cls is G.GraphFlatIndex
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        HNSWFaissSearch(None, similarity_metric=1)
    for bad in (dict(hnsw_store_n=0), dict(hnsw_ef_search=0), dict(hnsw_ef_search=4096), dict(hnsw_ef_construction=0)):
        with pytest.raises(ValueError, match="hnsw_"):
            HNSWFaissSearch(None, **bad)


def test_shims_and_hybrid_route():
    from lightretriever.retriever.faiss_index import FaissHNSWIndex
    from lightretriever.retriever.faiss_search import HNSWFaissSearch
    import lightretriever_amd
    from lightretriever_amd import retriever
    assert HNSWFaissSearch is retriever.HNSWFaissSearch and FaissHNSWIndex is retriever.FaissHNSWIndex
    assert lightretriever_amd.GraphFlatIndex is G.GraphFlatIndex
    h = retriever.HybridSearch(model=None, faiss_search_map="graph", hnsw_store_n=8, hnsw_ef_search=77, hnsw_ef_construction=90, nlist=4)
    assert type(h.dense_search) is HNSWFaissSearch
    assert (h.dense_search.hnsw_store_n, h.dense_search.hnsw_ef_search, h.dense_search.hnsw_ef_construction) == (8, 77, 90)
    with pytest.raises(NotImplementedError):
        retriever.HybridSearch(model=None, faiss_search_map="graph", similarity_metric=1)
    with pytest.raises((ValueError, NotImplementedError)):                              # not a base of the exact re-ranking: its scores are exact already
        retriever.RefineFaissSearch(None, refine_base="graph")


def test_index_argument_refusals_need_no_gpu():
    for kw, msg in ((dict(d=48), "d=48"), (dict(d=16384), "d=16384"), (dict(degree=12), "degree=12"), (dict(degree=136), "degree=136"),
                    (dict(degree=0), "degree=0"), (dict(intermediate_degree=16), "intermediate_degree=16"), (dict(intermediate_degree=257), "intermediate_degree=257"),
                    (dict(ef_search=0), "ef_search=0"), (dict(ef_search=2049), "ef_search=2049"), (dict(search_width=0), "search_width=0"),
                    (dict(search_width=9), "search_width=9"), (dict(n_entry=0), "n_entry=0")):
        args = dict(d=64, degree=32, intermediate_degree=64, ef_search=128, search_width=4)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            G.GraphFlatIndex(**args)


# ---- ABI and argument checks ------------------------------------------------------------------------------------------------------------------
NAMES = ("lrx_graph_ip_workspace_bytes", "lrx_graph_ip_search", "lrx_graph_detour_counts")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "lrx.h")).read()
    l = ctypes.CDLL(build.build(verbose=False))
    for name in NAMES:
        assert name + "(" in hdr and hasattr(l, name) and name in _lib.SIGNATURES, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [5, 23, 5]
    assert "#define LRX_ABI_VERSION 9" in hdr and _lib.lib().lrx_abi_version() == _lib.ABI_VERSION == 9
    assert '#include "lrx_search_graph.h"' in open(os.path.join(ROOT, "lightretriever_amd", "csrc", "lrx_search.hip")).read()
    from lightretriever_amd import ops
    assert callable(ops.graph_ip_topk) and callable(ops.graph_detour_counts)


FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work


def _search(l, *, X=FAKE, n_rows=1000, ldx=64, dim=64, graph=FAKE, degree=32, q=FAKE, nq=3, entry=FAKE, n_entry=64, ld_entry=64, k=10, beam=64,
            width=4, max_it=0, out=FAKE, ws=None, ws_bytes=0):
    return l.lrx_graph_ip_search(X, n_rows, ldx, dim, graph, degree, q, nq, entry, n_entry, ld_entry, k, beam, width, max_it, 0, out, out, None, None, ws,
                                 ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(dim=48, ldx=48), b"dim=48"), (dict(dim=0), b"dim=0"), (dict(dim=8224, ldx=8224), b"dim=8224"), (dict(ldx=60), b"ldx=60"), (dict(ldx=66), b"ldx=66"),
    (dict(X=ctypes.c_void_p(264)), b"16-byte"), (dict(q=ctypes.c_void_p(260)), b"16-byte"),
    (dict(degree=0), b"degree=0"), (dict(degree=12), b"degree=12"), (dict(degree=136), b"degree=136"),
    (dict(k=0), b"k=0"), (dict(k=65), b"k=65"), (dict(beam=2049, k=10), b"beam=2049"), (dict(beam=0, k=0), b"beam=0"),
    (dict(width=0), b"width=0"), (dict(width=9), b"width=9"),
    (dict(n_rows=-1), b"n_rows=-1"), (dict(n_rows=1 << 31), b"n_rows=2147483648"),
    (dict(n_entry=0, ld_entry=0), b"n_entry=0"), (dict(n_entry=2049, ld_entry=2049), b"n_entry=2049"), (dict(ld_entry=63), b"ld_entry=63"),
    (dict(max_it=-1), b"max_iterations=-1"), (dict(max_it=65537), b"max_iterations=65537"), (dict(nq=-1), b"n_queries=-1"),
    (dict(q=None), b"null"), (dict(entry=None), b"null"), (dict(out=None), b"null"), (dict(X=None), b"null"), (dict(graph=None), b"null")])
def test_graph_search_argument_errors_need_no_gpu(kw, msg):
    l = _lib.lib()
    assert _search(l, **kw) == -1, kw               # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())


def test_graph_search_launches_nothing_for_zero_queries():
    l = _lib.lib()
    assert _search(l, nq=0, q=None, entry=None, out=None) == 0
    assert _search(l, nq=0, X=None, graph=None, n_rows=0) == 0
    # every traversal lives in LDS: no global scratch for any arguments, so a NULL workspace is accepted (and LRX_ERR_WORKSPACE cannot arise today)
    assert [l.lrx_graph_ip_workspace_bytes(*a) for a in ((1, 1, 8, 1, 1), (1000, 2048, 128, 2048, 8), (0, 0, 0, 0, 0))] == [0, 0, 0]


@pytest.mark.parametrize("kw,msg", [(dict(K=0), b"K=0"), (dict(K=257), b"K=257"), (dict(n=-1), b"n_rows=-1"), (dict(n=1 << 31), b"n_rows=2147483648"),
                                    (dict(knn=None), b"null"), (dict(counts=None), b"null")])
def test_detour_count_argument_errors_need_no_gpu(kw, msg):
    l = _lib.lib()
    a = dict(knn=FAKE, n=100, K=32, counts=FAKE)
    a.update(kw)
    assert l.lrx_graph_detour_counts(a["knn"], a["n"], a["K"], a["counts"], None) == -1, kw
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert l.lrx_graph_detour_counts(None, 0, 32, None, None) == 0


# ---- the side file -----------------------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    p = dict(d=64, ntotal=5, degree=8, intermediate_degree=16, ef_search=32, search_width=2, n_entry=-1)
    p.update(kw)
    return p


def test_side_file_round_trip_and_refusals(tmp_path):
    rng = np.random.default_rng(0)
    graph = rng.integers(-1, 5, (5, 8)).astype(np.int32)
    entries = np.array([0, 2, 4], dtype=np.int64)
    f = str(tmp_path / "a.hnsw.faiss")
    G.write_graph_file(f, graph, entries, _params())
    st = G.read_graph_file(f)
    assert np.array_equal(st["graph"], graph) and np.array_equal(st["entry_rows"], entries) and st["graph"].dtype == np.int32
    assert {p: st[p] for p in G.PARAMS} == _params()
    for bad, msg in (((graph[:4], entries, _params()), r"int32 \[5, 8\]"),                       # a table of another row count
                     ((graph[:, :4], entries, _params()), r"int32 \[5, 8\]"),                    # ... of another degree
                     ((graph.astype(np.int64), entries, _params()), "int32"),
                     ((np.where(graph == 4, 5, graph), entries, _params()), r"\[-1, 5\)"),       # an edge to a row that does not exist
                     ((np.where(graph == -1, -2, graph), entries, _params()), r"\[-1, 5\)"),
                     ((graph, np.array([0, 5]), _params()), "entry_rows"),
                     ((graph, np.array([-1]), _params()), "entry_rows"),
                     ((graph, np.zeros(0, np.int64), _params()), "entry_rows"),
                     ((graph, entries, _params(degree=12)), "degree=12"),
                     ((graph, entries, _params(d=50)), "d=50"),
                     ((graph, entries, _params(ef_search=0)), "ef_search=0")):
        g = str(tmp_path / "bad.faiss")
        G.write_graph_file(g, *bad)
        with pytest.raises(ValueError, match=msg):
            G.read_graph_file(g)
    # the table against the store it is installed over: ntotal disagrees, or the rows have another d
    with pytest.raises(ValueError, match="built for 5 rows, but the store holds 6"):
        G.check_table(np.zeros((6, 8), np.int32), entries, 6, 8, built_for=5)
    with pytest.raises(ValueError, match="d=32"):
        G.check_table(graph, entries, 5, 8, store_d=32)
    np.savez(str(tmp_path / "c.faiss") + ".graph.npz", graph=graph, entry_rows=entries)
    with pytest.raises(ValueError, match="no params"):
        G.read_graph_file(str(tmp_path / "c.faiss"))
    np.savez(str(tmp_path / "d.faiss") + ".graph.npz", graph=graph, entry_rows=entries, params=np.arange(3))
    with pytest.raises(ValueError, match="params holds 3"):
        G.read_graph_file(str(tmp_path / "d.faiss"))
