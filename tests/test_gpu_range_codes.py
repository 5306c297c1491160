"""GPU: range search over the fp16 scalar-quantised, product-quantised and impact indexes (SQFp16Index / PQIndex / ImpactIndex.range_search,
ImpactSearch.retrieve_all_with_emb, torch.ops.lrx.{sq_fp16_ip,pq_ip,impact}_range_search) against the numpy yardstick of the contract
(tests/range_codes_yardstick.py).  Every comparison is exact: lims and ids equal, the scores bit for bit.

Shapes are the smallest at which each path can go wrong.  fp16-SQ: 20 000 rows take the candidate-list path (more than 4096 rows), 130
queries cross the 128-query group inside a chunk, 3 000 rows take the score-matrix path, 70 000 rows under radius = -inf overflow the 64 Ki
list.  PQ / impact: 5 000 / 3 000 rows span two 4096-row segments at the default row chunk and many row chunks at 1024 / 256 / 128."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import impact_yardstick as IY  # noqa: E402
import range_codes_yardstick as RY  # noqa: E402

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    lims, D, I = (t.cpu() for t in got)
    wl, wD, wI = (torch.from_numpy(np.ascontiguousarray(a)) for a in want)
    assert lims.dtype == torch.int64 and D.dtype == torch.float32 and I.dtype == torch.int64
    assert torch.equal(lims, wl), (lims[:8].tolist(), wl[:8].tolist())
    assert torch.equal(I, wI)
    assert torch.equal(D.view(torch.int32), wD.view(torch.int32))


def same_tensors(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])) and torch.equal(a[2], b[2]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def radius_for(S, per_query):
    """A radius drawn from the yardstick's own scores: about `per_query` rows per query pass (0: the largest score itself -- strictly
    greater keeps nothing, and the radius equals a stored score)."""
    flat = np.sort(np.asarray(S, np.float32).ravel())[::-1]
    return float(flat[min(per_query * S.shape[0], flat.size - 1)])


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------
# fp16 scalar-quantised index
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sq_case(n, d, nq, id_base=0):
    """(index, queries on the device, yardstick scores fp32 [nq, n]): computed once per shape, shared by the tests and left unchanged."""
    from lightretriever_amd import SQFp16Index
    rng = np.random.default_rng(n + d)
    x, q = unit(rng, n, d), unit(rng, nq, d)
    q[0] = x[n // 3] + 0.05 * q[0]                                   # one query next to a stored row
    idx = SQFp16Index(d, capacity=n, id_base=id_base)
    idx.add(torch.from_numpy(x))
    codes = x.astype(np.float16)                                     # round-to-nearest-even, the index's rule (no value near fp16's limits)
    assert torch.equal(idx.codes().cpu(), torch.from_numpy(codes))
    return idx, torch.from_numpy(q).cuda(), RY.sq_fp16_scores(q, codes)


@pytest.mark.parametrize("Q", [1, 5, 130])
def test_sq_list_path(Q):
    idx, q, S = sq_case(20_000, 128, 130)
    for per_query in (0, 50, 2000):
        radius = radius_for(S[:Q], per_query)
        want = RY.range_dense(S[:Q], radius)
        assert abs(int(want[0][-1]) - per_query * Q) <= Q
        assert_same(idx.range_search(q[:Q], radius), want)


def test_sq_small_shard_takes_the_matrix_path():
    idx, q, S = sq_case(3_000, 128, 9)
    for per_query in (0, 50, 2000):
        radius = radius_for(S, per_query)
        assert_same(idx.range_search(q, radius), RY.range_dense(S, radius))


def test_sq_width_not_a_multiple_of_64_cannot_be_stored():
    """20 000 x 96: the tiled code layout exists only for d % 64 == 0, so no fp16-SQ index of that width can be built and the library's entry
    point refuses the width before any launch -- there is no `dim % 64 != 0` state for the range search to fall back from."""
    from lightretriever_amd import SQFp16Index, _lib
    with pytest.raises(ValueError, match="multiple of 64"):
        SQFp16Index(96, capacity=20_000)
    q = torch.zeros(1, 96, device="cuda")
    lims = torch.zeros(2, dtype=torch.int64, device="cuda")
    rc = _lib.lib().lrx_sq_fp16_ip_range_search(_lib.ptr(q), 20_000, 96, _lib.ptr(q), _lib.ptr(q), 1, 0.0, 0, _lib.ptr(lims), None, None, 0, _lib.ptr(q), 0, None)
    assert rc == -1 and b"dim=96" in _lib.lib().lrx_last_error()


def test_sq_list_overflow_falls_back_to_the_matrix_and_counts():
    """radius = -inf returns every row: 70 000 > the 64 Ki entries of a candidate list, so both queries take the score-matrix path and
    lrx_search_fallback_count grows by 2 per LIBRARY call.  The statistic is the flat range search's: it counts inside the library, and
    140 000 hits are more than the 2 x 1024 first guess, so SQFp16Index.range_search calls the library twice (4); one library call whose
    outputs fit counts exactly the 2 queries."""
    from lightretriever_amd import _lib
    idx, q, S = sq_case(70_000, 64, 2)
    lib = _lib.lib()
    want = RY.range_dense(S, -np.inf)
    torch.cuda.synchronize()
    before = int(lib.lrx_search_fallback_count(0))
    got = idx.range_search(q, -np.inf)
    assert int(lib.lrx_search_fallback_count(0)) - before == 2 * 2     # 2 queries x (first guess too short + the resized call)
    assert got[0].tolist() == [0, 70_000, 140_000]
    assert_same(got, want)
    lims = torch.empty(3, dtype=torch.int64, device="cuda")
    D = torch.empty(140_000, dtype=torch.float32, device="cuda")
    I = torch.empty(140_000, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.lrx_sq_fp16_ip_range_workspace_bytes(idx.ntotal, idx.d, 2)), dtype=torch.uint8, device="cuda")
    before = int(lib.lrx_search_fallback_count(0))
    _lib.check(lib.lrx_sq_fp16_ip_range_search(_lib.ptr(idx._xb), idx.ntotal, idx.d, _lib.ptr(idx._bounds), _lib.ptr(q), 2, -np.inf, 0, _lib.ptr(lims),
                                               _lib.ptr(D), _lib.ptr(I), 140_000, _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    assert int(lib.lrx_search_fallback_count(0)) - before == 2
    assert_same((lims, D, I), want)
    # a radius few rows pass keeps both queries on the list path: no fallback
    before = int(lib.lrx_search_fallback_count(0))
    assert_same(idx.range_search(q, radius_for(S, 50)), RY.range_dense(S, radius_for(S, 50)))
    assert int(lib.lrx_search_fallback_count(0)) == before


def test_sq_radius_equal_to_a_stored_score_excludes_that_row():
    idx, q, S = sq_case(20_000, 128, 130)
    order = np.argsort(-S[0], kind="stable")
    r = int(order[30])                                               # the 31st best row of query 0: its score is the radius
    radius = float(S[0, r])
    lims, D, I = idx.range_search(q[:1], radius)
    assert r not in I.tolist() and int(lims[1]) == int((S[0] > np.float32(radius)).sum()) >= 30
    assert_same((lims, D, I), RY.range_dense(S[:1], radius))
    below = float(np.nextafter(np.float32(radius), np.float32(-np.inf)))
    assert r in idx.range_search(q[:1], below)[2].tolist()


def test_sq_id_base_empty_and_extremes():
    from lightretriever_amd import SQFp16Index
    idx, q, S = sq_case(20_000, 128, 6, 1000)
    radius = radius_for(S, 50)
    want = RY.range_dense(S, radius, id_base=1000)
    assert int(want[2].min()) >= 1000
    assert_same(idx.range_search(q, radius), want)
    assert_same(idx.range_search(q, np.inf), RY.range_dense(S, np.inf))
    with pytest.raises(ValueError, match="NaN"):
        idx.range_search(q, float("nan"))
    lims, D, I = idx.range_search(q[:0], 0.0)
    assert lims.tolist() == [0] and D.numel() == I.numel() == 0
    empty = SQFp16Index(128)
    lims, D, I = empty.range_search(q, 0.0)
    assert lims.tolist() == [0] * 7 and D.numel() == I.numel() == 0


def test_sq_result_longer_than_the_first_guess_is_resized():
    idx, q, S = sq_case(20_000, 128, 130)
    radius = radius_for(S[:2], 3000)                                 # ~6000 hits for 2 queries: more than the 2 x 1024 first guess
    want = RY.range_dense(S[:2], radius)
    assert int(want[0][-1]) > 2 * 1024
    assert_same(idx.range_search(q[:2], radius), want)


def test_sq_result_does_not_depend_on_batching_or_the_workspace_cap():
    idx, q, S = sq_case(20_000, 128, 130)
    radius = radius_for(S, 50)
    whole = idx.range_search(q, radius)
    assert_same(whole, RY.range_dense(S, radius))
    one_by_one = [idx.range_search(q[i:i + 1], radius) for i in (0, 64, 129)]
    for i, (lims, D, I) in zip((0, 64, 129), one_by_one):
        a, b = int(whole[0][i]), int(whole[0][i + 1])
        assert int(lims[1]) == b - a and torch.equal(I, whole[2][a:b]) and torch.equal(D.view(torch.int32), whole[1][a:b].view(torch.int32))
    cap = idx.max_workspace_bytes
    try:
        idx.max_workspace_bytes = 24 << 20                           # forces host chunks of fewer than 130 queries: the results are stitched
        assert int(idx.lib.lrx_sq_fp16_ip_range_workspace_bytes(idx.ntotal, idx.d, 130)) > (24 << 20)
        assert same_tensors(idx.range_search(q, radius), whole)
    finally:
        idx.max_workspace_bytes = cap


def test_sq_equals_the_flat_index_over_the_decoded_codes():
    """Both are bit-exact under the same score on the same fp32 rows (the decoded codes are exactly fp16-representable)."""
    from lightretriever_amd import FlatIPIndex
    from lightretriever_amd.retriever import FaissIndex
    idx, q, S = sq_case(20_000, 128, 130)
    flat = FlatIPIndex(128, capacity=idx.ntotal)
    flat.add(idx.vectors)
    for per_query in (50, 2000):
        radius = radius_for(S[:5], per_query)
        assert same_tensors(idx.range_search(q[:5], radius), flat.range_search(q[:5], radius))
    # FaissIndex.range_search works unchanged over the quantised index
    pids = np.arange(idx.ntotal, dtype=np.int64) * 3 + 7
    lims, D, I = FaissIndex(idx, pids).range_search(q[:5], radius)
    want = RY.range_dense(S[:5], radius)
    assert_same((lims, D, I), (want[0], want[1], pids[want[2]]))


def test_sq_op_equals_method():
    from lightretriever_amd import torch_ops  # noqa: F401
    for shape, nq in (((20_000, 128), 130), ((3_000, 128), 9)):
        idx, q, S = sq_case(*shape, nq)
        radius = radius_for(S[:7], 50)
        got = torch.ops.lrx.sq_fp16_ip_range_search(q[:7], idx._xb, idx.ntotal, idx._bounds, radius, idx.id_base)
        assert same_tensors(got, idx.range_search(q[:7], radius))
        assert_same(got, RY.range_dense(S[:7], radius))


# ---------------------------------------------------------------------------------------------------------------
# product-quantised index
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pq_case(id_base=0):
    """d = 32, M = 8, trained on 4 096 rows, 5 000 rows added; 40 queries; the yardstick's scores from the index's own centroids and codes."""
    from lightretriever_amd import PQIndex
    rng = np.random.default_rng(5)
    x, q = unit(rng, 5_000, 32), unit(rng, 40, 32)
    idx = PQIndex(32, 8, id_base=id_base)
    idx.train(torch.from_numpy(x[:4096]))
    idx.add(torch.from_numpy(x))
    S = RY.pq_scores(q, idx.centroids.cpu().numpy(), idx.codes().cpu().numpy())
    return idx, torch.from_numpy(q).cuda(), S


@pytest.mark.parametrize("Q", [1, 3, 40])
def test_pq_default_chunk(Q):
    idx, q, S = pq_case()
    for per_query in (0, 50, 2000):
        radius = radius_for(S[:Q], per_query)
        assert_same(idx.range_search(q[:Q], radius), RY.range_dense(S[:Q], radius))


@pytest.mark.parametrize("row_chunk", [1024, 128])
def test_pq_many_row_chunks_give_the_same_result(row_chunk):
    idx, q, S = pq_case()
    try:
        idx.range_row_chunk = row_chunk
        for Q, per_query in ((40, 50), (3, 2000), (1, 0)):
            radius = radius_for(S[:Q], per_query)
            assert_same(idx.range_search(q[:Q], radius), RY.range_dense(S[:Q], radius))
        assert_same(idx.range_search(q[:3], -np.inf), RY.range_dense(S[:3], -np.inf))
    finally:
        idx.range_row_chunk = 0


def test_pq_extremes_id_base_and_resize():
    from lightretriever_amd import PQIndex
    idx, q, S = pq_case(1000)
    everything = idx.range_search(q[:3], -np.inf)                    # 15 000 hits: more than the 3 x 1024 first guess -> one resize
    assert everything[0].tolist() == [0, 5000, 10000, 15000]
    assert int(everything[2].min()) == 1000 and int(everything[2].max()) == 5999
    assert_same(everything, RY.range_dense(S[:3], -np.inf, id_base=1000))
    assert_same(idx.range_search(q, np.inf), RY.range_dense(S, np.inf))
    radius = radius_for(S, 50)
    assert_same(idx.range_search(q, radius), RY.range_dense(S, radius, id_base=1000))
    with pytest.raises(ValueError, match="NaN"):
        idx.range_search(q, float("nan"))
    lims, D, I = idx.range_search(q[:0], 0.0)
    assert lims.tolist() == [0] and D.numel() == I.numel() == 0
    lims, D, I = PQIndex(32, 8).range_search(q[:2], 0.0)
    assert lims.tolist() == [0, 0, 0] and D.numel() == I.numel() == 0


def test_pq_scores_are_the_ones_search_reports():
    idx, q, S = pq_case()
    Dk, Ik = idx.search(q[:3], 100)
    radius = float(Dk.min().item())
    lims, D, I = idx.range_search(q[:3], float(np.nextafter(np.float32(radius), np.float32(-np.inf))))
    for i in range(3):
        a, b = int(lims[i]), int(lims[i + 1])
        pos = torch.searchsorted(I[a:b], Ik[i])                      # rows ascend inside a query
        assert torch.equal(I[a:b][pos], Ik[i]) and torch.equal(D[a:b][pos].view(torch.int32), Dk[i].view(torch.int32))


def test_pq_op_equals_method():
    from lightretriever_amd import torch_ops  # noqa: F401
    idx, q, S = pq_case()
    radius = radius_for(S, 50)
    want = idx.range_search(q, radius)
    for row_chunk in (0, 1024):
        got = torch.ops.lrx.pq_ip_range_search(q, idx._codes, idx.centroids, idx.ntotal, radius, idx.id_base, row_chunk)
        assert same_tensors(got, want)
    assert_same(want, RY.range_dense(S, radius))


# ---------------------------------------------------------------------------------------------------------------
# impact index
# ---------------------------------------------------------------------------------------------------------------
VOCAB = 500


@functools.lru_cache(maxsize=None)
def impact_case():
    """3 000 documents x 8 .. 40 terms over a 500-term vocabulary, weights 1 .. 200; queries of 2 .. 12 terms (at most 2048 hits each),
    two of 60 terms (more than 2048 hits), one whose only term no document holds; the yardstick's integer scores."""
    rng = np.random.default_rng(17)
    docs = []
    for _ in range(3000):
        nnz = int(rng.integers(8, 41))
        docs.append((rng.choice(VOCAB, nnz, replace=False), rng.integers(1, 201, nnz)))
    queries = []
    for nt in (2, 3, 5, 8, 12, 12, 60, 60):
        queries.append((rng.choice(VOCAB, nt, replace=False), rng.integers(1, 4, nt)))
    queries.insert(4, ([VOCAB + 400], [2]))
    yard = IY.Yardstick(*IY.csr_of(docs))
    return docs, queries, RY.impact_scores(yard, [(np.asarray(t)[np.asarray(t) < VOCAB], np.asarray(c)[np.asarray(t) < VOCAB]) for t, c in queries])


def impact_index(docs, window_rows=0, row_chunk=0, id_base=0):
    from lightretriever_amd import ImpactIndex
    idx = ImpactIndex(id_base=id_base)
    idx.window_rows, idx.range_row_chunk = window_rows, row_chunk
    idx.add(*IY.csr_of(docs))
    return idx


def impact_range(idx, queries, radius):
    from lightretriever_amd.impact_index import query_csr
    return idx.range_search(*query_csr(queries), radius)


def test_impact_every_hit():
    docs, queries, S = impact_case()
    idx = impact_index(docs)
    got = impact_range(idx, queries, -1)
    want = RY.range_impact(S, -1)
    assert_same(got, want)
    lims, D, I = (t.cpu() for t in got)
    nhits = (S >= 1).sum(axis=1)
    assert torch.equal(lims[1:] - lims[:-1], torch.from_numpy(nhits)) and float(D.min()) >= 1.0
    assert nhits[4] == 0 and int(lims[4]) == int(lims[5])             # the query with no known term: an empty slice
    assert (nhits > 2048).sum() == 2 and (nhits[nhits > 0] <= 2048).sum() == 6
    # where the top-k search can hold every hit, it returns the same set
    from lightretriever_amd.impact_index import query_csr
    Dk, Ik = (t.cpu() for t in idx.search(*query_csr(queries), 2048))
    for i in np.flatnonzero(nhits <= 2048):
        a, b = int(lims[i]), int(lims[i + 1])
        top = {int(r): float(s) for s, r in zip(Dk[i].tolist(), Ik[i].tolist()) if r >= 0}
        assert top == dict(zip(I[a:b].tolist(), D[a:b].tolist()))
    # radius 0 and -inf keep the same rows: only hits are ever returned
    assert same_tensors(impact_range(idx, queries, 0.0), got) and same_tensors(impact_range(idx, queries, -np.inf), got)


def test_impact_radius_at_a_score_quantile_and_extremes():
    docs, queries, S = impact_case()
    idx = impact_index(docs, id_base=500)
    hits = S[S >= 1].astype(np.float32)
    for quantile in (0.5, 0.9, 0.999):
        radius = float(np.quantile(hits, quantile, method="lower"))   # a score some row holds: strictly greater excludes it
        want = RY.range_impact(S, radius, id_base=500)
        assert 0 < int(want[0][-1]) < hits.size
        assert_same(impact_range(idx, queries, radius), want)
    assert_same(impact_range(idx, queries, float(hits.max())), RY.range_impact(S, float(hits.max()), id_base=500))
    assert_same(impact_range(idx, queries, np.inf), RY.range_impact(S, np.inf))
    with pytest.raises(ValueError, match="NaN"):
        impact_range(idx, queries, float("nan"))
    lims, D, I = impact_range(idx, [], 0.0)
    assert lims.tolist() == [0] and D.numel() == I.numel() == 0
    with pytest.raises(ValueError, match="2\\^31"):                    # the overflow refusal stays check_queries'
        impact_range(idx, [([int(queries[0][0][0])], [1 << 30])], 0.0)


@pytest.mark.parametrize("window_rows", [128, 2048])
def test_impact_row_chunks_and_windows_give_the_same_result(window_rows):
    docs, queries, S = impact_case()
    idx = impact_index(docs, window_rows=window_rows, row_chunk=256)
    assert_same(impact_range(idx, queries, -1), RY.range_impact(S, -1))
    radius = float(np.quantile(S[S >= 1].astype(np.float32), 0.9, method="lower"))
    assert_same(impact_range(idx, queries, radius), RY.range_impact(S, radius))


def test_impact_op_equals_method():
    from lightretriever_amd import torch_ops  # noqa: F401
    docs, queries, S = impact_case()
    idx = impact_index(docs)
    want = impact_range(idx, queries, 100.0)
    from lightretriever_amd.impact_index import query_csr
    off, term, cnt = (torch.from_numpy(a).cuda() for a in idx.check_queries(*query_csr(queries)))
    for window_rows, row_chunk in ((0, 0), (128, 256)):
        got = torch.ops.lrx.impact_range_search(idx._postings, idx._term_off, idx.ntotal, off, term, cnt, 100.0, idx.id_base, window_rows, row_chunk)
        assert same_tensors(got, want)
    assert_same(want, RY.range_impact(S, 100.0))


def test_impact_search_retrieve_all_with_emb_serves_every_query_form():
    from lightretriever_amd.retriever import ImpactSearch
    from lightretriever_amd.sparse_rows import SparseRows
    docs, queries, S = impact_case()
    queries = [queries[i] for i in (0, 3, 4, 7)]                      # small, empty and > 2048 hits
    S = S[[0, 3, 4, 7]]
    eng = ImpactSearch()
    pids = [f"d{i}" for i in range(len(docs))]
    eng.index([{str(int(t)): int(w) for t, w in zip(ts, ws)} for ts, ws in docs], pids)
    qids = [f"q{i}" for i in range(len(queries))]
    as_dicts = [{str(int(t)): int(c) for t, c in zip(ts, cs)} for ts, cs in queries]
    as_text = [" ".join(" ".join([str(int(t))] * int(c)) for t, c in zip(ts, cs)) for ts, cs in queries]
    known = [[(int(t), int(c)) for t, c in sorted(zip(ts, cs)) if t < VOCAB] for ts, cs in queries]      # (SparseRows: token ids below vocab_size)
    off = np.cumsum([0] + [len(k) for k in known])
    rows = SparseRows(torch.tensor(off, dtype=torch.int64), torch.tensor([t for k in known for t, _ in k], dtype=torch.int32),
                      torch.tensor([c for k in known for _, c in k], dtype=torch.int32), VOCAB).to("cuda")
    want = {qid: {pids[r]: float(np.float32(S[i, r])) for r in np.flatnonzero(S[i] >= 1)} for i, qid in enumerate(qids)}
    assert len(want["q3"]) > 2048 and want["q2"] == {}
    for form in (as_dicts, as_text, rows):
        assert eng.retrieve_all_with_emb(form, qids) == want
    cut = float(np.quantile(S[S >= 1].astype(np.float32), 0.9, method="lower"))
    want_cut = {qid: {p: s for p, s in hits.items() if s > cut} for qid, hits in want.items()}
    assert eng.retrieve_all_with_emb(as_dicts, qids, min_score=cut) == want_cut
    top = eng.retrieve_with_emb(as_dicts, qids, 10)                    # the top-k engine call is a subset with the same scores
    assert all(want[qid][p] == s for qid in qids for p, s in top[qid].items())


# ---------------------------------------------------------------------------------------------------------------
# graph capture: the result length is read back once per library call, so every range_search refuses before anything is launched
# ---------------------------------------------------------------------------------------------------------------
def test_range_search_is_refused_under_graph_capture():
    from lightretriever_amd import _lib
    from lightretriever_amd.impact_index import query_csr
    sq, q_sq, S_sq = sq_case(3_000, 128, 9)
    pq, q_pq, S_pq = pq_case()
    docs, queries, S_im = impact_case()
    imp = impact_index(docs)
    eager = [sq.range_search(q_sq, 0.1), pq.range_search(q_pq, 0.5), impact_range(imp, queries, 100.0)]   # (workspaces exist, postings finalised)
    torch.cuda.synchronize()
    csr = query_csr(queries)
    for call in (lambda: sq.range_search(q_sq, 0.1), lambda: pq.range_search(q_pq, 0.5), lambda: imp.range_search(*csr, 100.0)):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.LrxError, match="graph capture"):
            with torch.cuda.graph(g):
                call()
        del g
    torch.cuda.synchronize()
    # the stream is usable afterwards and the results are what they were
    again = [sq.range_search(q_sq, 0.1), pq.range_search(q_pq, 0.5), impact_range(imp, queries, 100.0)]
    assert all(same_tensors(a, b) for a, b in zip(again, eager))
