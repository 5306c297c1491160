"""GPU: every branch of the shared top-k selection (lrx_search_select.h: select_topk_sorted, rescore_band) on crafted score rows, against
the host model of tests/select_reference.py.  Three harnesses make an existing index report an intended integer score row exactly (PQIndex ->
k_topk_select, FlatIPIndex with two_pass = False -> k_topk_select_rescore<ROWS_F32>, SQ8Index -> k_sq8_select_rescore), so the selection is
the only step left to go wrong; test_select_reference_host.py proves on the CPU that each case sits on the branch it names.  Ids are compared
with torch.equal and scores by their bits: there is no tolerance in this file.  The one branch that shows from outside, the streaming form of
the band under the SQ8 select, is read off lrx_search_fallback_count."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import impact_yardstick as IY  # noqa: E402
import select_reference as R  # noqa: E402
import sq8_yardstick as SY  # noqa: E402

pytestmark = pytest.mark.gpu

_LEVELS = {}


def levels_of(case):
    if case["name"] not in _LEVELS:
        _LEVELS[case["name"]] = case["make"]()
    return _LEVELS[case["name"]]


def assert_same(got, want):
    D, I = (torch.from_numpy(np.ascontiguousarray(a)) for a in want)
    assert torch.equal(got[1].cpu(), I)
    assert torch.equal(got[0].cpu().view(torch.int32), D.view(torch.int32))


def mapped(I, row_map):
    return np.where(I >= 0, row_map[np.maximum(I, 0)], -1)


def pq_index(v, special=False, id_base=0):
    from lightretriever_amd import PQIndex
    idx = PQIndex(R.PQ_D, R.PQ_M, id_base=id_base)
    idx.set_contents(torch.from_numpy(R.pq_tables(special)), torch.from_numpy(R.pq_codes(v, special)))
    return idx


def flat_index(lv, id_base=0):
    from lightretriever_amd import FlatIPIndex
    idx = FlatIPIndex(R.FLAT_D, capacity=len(lv), id_base=id_base)
    idx.two_pass = False
    idx.add(torch.from_numpy(R.flat_rows(lv)))
    return idx


def sq8_index(lv, id_base=0):
    from lightretriever_amd import SQ8Index
    idx = SQ8Index(R.SQ8_D, "QT_8bit_uniform", id_base=id_base)
    idx.set_contents(torch.from_numpy(R.SQ8_TRAINED), torch.from_numpy(R.sq8_codes(lv)))
    return idx


# ---- A: every PQ case, all of its queries in one call (the workgroups of one launch take different branches) ----------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["name"])
def test_pq_case_with_id_base_and_row_map(case):
    v, S = R.case_rows(case)
    n = len(v)
    idx = pq_index(v, case["special"], case["id_base"])
    q = torch.from_numpy(R.pq_queries(case["queries"])).cuda()
    row_map = np.arange(n, dtype=np.int64) * 3 + 7
    row_map_gpu = torch.from_numpy(row_map).cuda()
    for k in case["ks"]:
        D, I = R.topk_rows(S, k)
        print(f"{case['name']} k={k}: " + ", ".join(R.select_path(s, k)[0] for s in S))
        assert_same(idx.search(q, k), (D, np.where(I >= 0, I + case["id_base"], -1)))
        assert_same(idx.search(q, k, row_map=row_map_gpu), (D, mapped(I, row_map)))


# ---- B: every band case through the two rescoring selects -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", R.FLAT_BATCHES)
@pytest.mark.parametrize("case", R.BAND_CASES, ids=lambda c: c["name"])
def test_flat_band_case(case, nq):
    lv, k = levels_of(case), case["k"]
    D2, I2 = R.topk_rows(R.flat_intended(lv, 2), k)
    pick = np.arange(nq) % 2
    got = flat_index(lv).search(torch.from_numpy(R.e0_queries(nq, R.FLAT_D)).cuda(), k)
    assert_same(got, (D2[pick], I2[pick]))


@pytest.mark.parametrize("case", R.BAND_CASES, ids=lambda c: c["name"])
def test_sq8_band_case_and_its_fallback_count(case):
    from lightretriever_amd import _lib
    lib = _lib.lib()
    lv, k, nq = levels_of(case), case["k"], R.SQ8_BATCH
    idx = sq8_index(lv)
    q = torch.from_numpy(R.e0_queries(nq, R.SQ8_D)).cuda()
    torch.cuda.synchronize()
    lib.lrx_search_fallback_count(1)
    got = idx.search(q, k)
    torch.cuda.synchronize()
    streamed = lib.lrx_search_fallback_count(1)
    forms = R.band_forms(lv, k, nq)
    print(f"{case['name']}: {streamed} queries streamed, model: {forms}")
    assert_same(got, SY.topk(R.sq8_expected_scores(lv, nq), k))
    assert streamed == sum(f.startswith("stream/") for f in forms)       # also: the band is no wider than one level (band_gap_ok, measured)


# ---- C: impact queries with fewer hits than k over more than 4096 rows ------------------------------------------------------------------------
def impact_case(hit_rows, n=20000):
    from lightretriever_amd import ImpactIndex
    weights = np.random.default_rng(len(hit_rows)).permutation(len(hit_rows)) + 1          # distinct
    docs = [([1], [1]) for _ in range(n)]                                                  # term 1 everywhere, term 0 in the hit rows only
    for r, w in zip(hit_rows, weights):
        docs[r] = ([1, 0], [1, int(w)])
    csr = IY.csr_of(docs)
    idx = ImpactIndex()
    idx.add(*csr)
    return idx, IY.Yardstick(*csr)


def impact_search(idx, queries, k):
    from lightretriever_amd.impact_index import query_csr
    return idx.search(*query_csr(queries), k)


def impact_assert(got, want):
    assert torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
    assert torch.equal(got[0].cpu().view(torch.int32), torch.from_numpy(want[0]).view(torch.int32))


def test_impact_fewer_hits_than_k_spread_over_blocks():
    rng = np.random.default_rng(3)
    rows = np.sort(rng.permutation(156)[:50] * 128 + rng.integers(0, 128, 50))             # 50 different blocks
    idx, y = impact_case(rows)
    queries = [([0], [1]), ([1], [1]), ([0, 1], [2, 1])]                                   # the hits; every row on one score; both
    dense = y.scores(*queries[0]).astype(np.float32)
    assert R.select_path(dense, 100)[0] == "fast>cand>exact/scan" and R.select_path(dense, 10)[0] == "fast"
    got = impact_search(idx, queries, 100)
    impact_assert(got, y.search(queries, 100))
    assert (got[1][0, :50] >= 0).all() and (got[1][0, 50:] == -1).all()                    # 50 hits, then padding
    impact_assert(impact_search(idx, queries, 10), y.search(queries, 10))


def test_impact_hits_packed_into_three_blocks():
    rows = np.concatenate([5 * 128 + np.arange(17) * 7, 77 * 128 + np.arange(17) * 5 + 3, 150 * 128 + np.arange(16) * 8])
    idx, y = impact_case(rows)
    queries = [([0], [1]), ([0, 1], [3, 1])]
    dense = y.scores(*queries[0]).astype(np.float32)
    label, counts = R.select_path(dense, 10)
    assert label == "fast>cand>exact/sorted" and counts["nb"] == 157 and counts["neq"] == 1     # the 10th block maximum is 0: every row is a candidate
    impact_assert(impact_search(idx, queries, 10), y.search(queries, 10))


# ---- D: a non-finite query in the batch ------------------------------------------------------------------------------------------------------
def check_batch_with_a_non_finite_query(search, q, bad, k, id_base, n):
    """Every other query: bit-identical to searching it alone.  The non-finite one: ids -1 or inside [id_base, id_base + n), no id twice;
    the contract does not define its order and nothing more is asserted.  (Regression: over a row of NaN scores with the sign bit set --
    an infinite query through the six-product or the 8-bit filter -- the block maxima, taken with fmaxf, stayed above every key, the fast
    path gathered no row and one id came back k times, until select_topk_sorted required at least k gathered rows of its fast path.)"""
    D, I = search(q)
    alone = {}
    for i in range(q.shape[0]):
        if i == bad:
            continue
        sig = q[i].cpu().numpy().tobytes()
        if sig not in alone:
            alone[sig] = search(q[i:i + 1])
        assert torch.equal(I[i], alone[sig][1][0]) and torch.equal(D[i].view(torch.int32), alone[sig][0][0].view(torch.int32))
    ids = I[bad].cpu().numpy()
    real = ids[ids != -1]
    assert ((real >= id_base) & (real < id_base + n)).all() and len(np.unique(real)) == len(real)


def test_non_finite_query_pq():
    v = R.CASE_BY_NAME["fast-20000"]["make"]()
    idx = pq_index(v, id_base=1000)
    q = torch.from_numpy(R.pq_queries(R.PQ_QUERIES[:2] + ((1, 1),) + R.PQ_QUERIES[2:])).cuda()
    q[2, 0] = float("inf")
    for k in (10, 300):
        check_batch_with_a_non_finite_query(lambda x: idx.search(x, k), q, 2, k, 1000, len(v))


@pytest.mark.parametrize("nq", R.FLAT_BATCHES)
def test_non_finite_query_flat_plain_path(nq):
    lv = levels_of(R.BAND_BY_NAME["band-merge"])
    idx = flat_index(lv, id_base=1000)
    q = torch.from_numpy(R.e0_queries(nq, R.FLAT_D)).cuda()
    q[1, 0] = float("inf")
    check_batch_with_a_non_finite_query(lambda x: idx.search(x, 100), q, 1, 100, 1000, len(lv))


def test_non_finite_query_sq8():
    lv = levels_of(R.BAND_BY_NAME["band-merge"])
    idx = sq8_index(lv, id_base=1000)
    q = torch.from_numpy(R.e0_queries(4, R.SQ8_D)).cuda()
    q[2, 0] = float("inf")
    check_batch_with_a_non_finite_query(lambda x: idx.search(x, 100), q, 2, 100, 1000, len(lv))
