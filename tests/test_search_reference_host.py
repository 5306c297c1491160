"""The fp64 model of the bounded search's filter stages (search_reference.py) against itself, and -- more important -- the preconditions of
every case of test_gpu_search_stages.py on the model alone: what a case claims to exercise (benign / overflow, which threshold branch, which
plan) holds before any GPU sees it.  No GPU."""
import os

import numpy as np
import pytest

import search_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        c = R.case_spec(name)
        X, q = R.case_data(name)
        plan = R.expected_plan(c["N"], c["D"], c["Q"], c["k"], c["has_shadow"], c["flags"])
        _MODELS[name] = (c, plan, R.StageModel(q, X, R.host_bounds(X), c["k"], plan, c["index"] == "sq"))
    return _MODELS[name]


def test_accessor_is_declared_in_header_and_binding():
    from lightretriever_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lrx.h")).read()
    assert "#define LRX_ABI_VERSION 9" in hdr and _lib.ABI_VERSION == 9
    assert "int lrx_flat_ip_bounded_chunk_state(const void* workspace, int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int32_t flags," in hdr
    assert "#define LRX_CHUNK_STATE_PLAN_INTS 12" in hdr
    assert len(_lib.SIGNATURES["lrx_flat_ip_bounded_chunk_state"][1]) == 15
    assert hasattr(_lib.lib(), "lrx_flat_ip_bounded_chunk_state") and _lib.lib().lrx_abi_version() == 9


def test_fp16_rounding_saturates_and_rounds_to_even():
    a = np.array([1e5, -1e5, 65519.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -26, 0.0], np.float32)
    assert R.f16_sat(a).tolist() == [65504.0, -65504.0, 65504.0, 1.0, 1 + 2.0 ** -9, 0.0, 0.0]


def test_eps_upper_factor_is_the_written_safety_factors():
    for D in (64, 1024):
        f = R.eps_upper_factor(D)
        assert 1.01 * 1.0001 < f < 1.01 * 1.0001 * (1 + 1e-4)              # the fp32 summation adds less than the 1.0001 allows
        assert R.eps_upper_factor(D, True) == pytest.approx(f * 1.0001, rel=1e-12)


def test_expected_plan_of_the_documented_shapes():
    """plan_chunk's rules at shapes whose plan DESIGN 5.4 / lrx_search.hip state in words."""
    p = R.expected_plan(1_000_000, 2048, 100, 100, True, 0)
    assert p["emit"] and not p["gemm"] and not p["fused"] and p["ss"] == 32 and p["cap"] == 65536 and p["nsplit"] == 2     # 30 blocks per CU: fill rule 32, hits rule 35
    assert R.expected_plan(1_000_000, 2048, 200, 100, True, 0)["gemm"] and R.expected_plan(1_000_000, 2048, 200, 100, True, 0)["rb"] == 256
    assert R.expected_plan(125_000, 2048, 16, 100, True, 0)["fused"] and not R.expected_plan(125_000, 2048, 32, 100, True, 0)["fused"]
    assert not R.expected_plan(10_000, 256, 10, 10, True, 0)["emit"] and R.expected_plan(10_000, 256, 10, 10, True, 2)["emit"]   # below 16 Ki rows: forced only
    assert R.expected_plan(100_000, 256, 10, 2048, True, 0)["cap"] == 131072
    assert not R.expected_plan(100_000, 256, 20, 10, False, 2)["emit"] and R.expected_plan(100_000, 256, 48, 10, False, 2)["group_rows"] == 128


def test_eps_ref_bounds_the_adversarial_midpoint_rows():
    """Elements just below / above fp16 rounding midpoints push |s64 - st64| towards its bound: eps_ref (no safety factor, no accumulation
    error in st64) must still hold for every (query, row) -- and how close it comes is reported."""
    X, q = R.adversarial_midpoint_case()
    plan = R.expected_plan(X.shape[0], X.shape[1], q.shape[0], 10, True, 2)
    m = R.StageModel(q, X, R.host_bounds(X), 10, plan)
    err = np.abs(m.s64 - m.st64)
    ratio = err / m.eps_ref[:, None]
    print(f"\nadversarial midpoints: max |s64 - st64| / eps_ref = {ratio.max():.4f} (crafted rows {ratio[:, :48 * 40].max():.4f}, "
          f"Gaussian rows {ratio[:, 48 * 40:].max():.4f}); sqrt(D) 2^-11 = {np.sqrt(128) * 2.0 ** -11:.4f}")
    assert (err <= m.eps_ref[:, None]).all()
    assert ratio.max() > 0.25                      # the crafted rows do come within a small factor of the bound (Gaussian rows: ~1e-2)


@pytest.mark.parametrize("name", list(R.CASES))
def test_eps_ref_bounds_the_rounding_error_of_every_case(name):
    _, _, m = _model(name)
    assert (np.abs(m.s64 - m.st64) <= m.eps_ref[:, None]).all()
    assert np.isfinite(m.s64).all() and np.isfinite(m.st64).all() and np.isfinite(m.eps_hi).all()
    lo, hi = m.threshold_bounds()
    assert (lo <= hi).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_preconditions(name):
    """Benign cases: every query's upper band count <= 1024 and upper list count <= cap / 2.  Overflow cases: the named queries have a lower
    band count > 4096 or a lower list count > cap, the others are benign.  No query is undecided inside the +- acc slack.
    ONE exception, stated: top-1000 of wave_lists_flushed cannot have a band of <= 1024 rows (the band holds the top-k itself: lower count
    1017..1049) -- there the bound is the band capacity of one part for the nsplit of the case's own plan (256 queries: one part of 4096 on any
    device of fewer than 512 compute units), which test_gpu_search_stages.py asserts the library reports."""
    c, plan, m = _model(name)
    assert plan["emit"], "the case does not reach the score-free filter"
    band_safe = 1024
    if name == "wave_lists_flushed":
        assert plan["nsplit"] == 1
        band_safe = R.REF_CAND // plan["nsplit"]
    p = m.predictions(band_safe)
    print(f"\n{name}: list [{p['list_lo'].min()}, {p['list_hi'].max()}] of {plan['cap']}, band [{p['band_lo'].min()}, {p['band_hi'].max()}], "
          f"verdicts {dict(zip(*np.unique(p['verdict'], return_counts=True)))}")
    assert (p["list_lo"] <= p["list_hi"]).all() and (p["band_lo"] <= p["band_hi"]).all() and (p["band_lo"] >= c["k"]).all()
    want = np.array(["overflow" if i in c["overflow"] else "benign" for i in range(c["Q"])])
    assert (p["verdict"] == want).all(), (p["verdict"], p["band_hi"], p["list_hi"])


def test_cases_reach_the_paths_they_name():
    g = lambda n: (_model(n)[1], _model(n)[2])
    for n in ("gemm_one_n_tile", "gemm_wide_ragged_n_tile"):
        assert g(n)[0]["gemm"] and g(n)[0]["rb"] == 256 and not g(n)[0]["fused"]
    for n in ("fused_1_tile", "fused_7_tiles"):
        assert g(n)[0]["fused"]
    for n in R.CASES:
        if not n.startswith("fused"):
            assert not g(n)[0]["fused"], n
    assert g("q_resident_block_max_thr")[1].threshold_grouping() == 128 and g("list_overflow_near_copies")[1].threshold_grouping() == 128
    assert g("sorted_scores_thr")[1].threshold_grouping() == 1 and g("wave_lists_flushed")[1].threshold_grouping() == 1
    assert g("no_shadow_dim_96")[0]["group_rows"] == 128 and g("no_shadow_switched_off")[0]["group_rows"] == 128
    assert g("no_shadow_dim_96")[1].threshold_grouping() == 1
    assert g("clustered_row_exact_thr")[1].threshold_grouping() == 16
    assert R.CASES["wg_per_block_3_slices_ragged"]["N"] % 128 != 0 and R.CASES["persistent_7_tiles_odd_blocks"]["N"] % 128 != 0
    # the clustered case is one where the group threshold alone would be far too low: the k-th group maximum lies well below the k-th sample score
    m = g("clustered_row_exact_thr")[1]
    lo, hi = m.threshold_bounds()
    half = m.Q // 2
    assert ((hi - lo)[:half] > 20 * m.eps_hi[:half]).all()
    # ... and more than 2 k sample rows reach the group threshold there: the condition of the row-exact branch, with the whole slack against it
    # (lo = the k-th group maximum of st64 minus the slack: the library's group T' is at most lo + 2 slack, its eps at least eps_ref)
    sr = m.sample_rows
    reach = (m.st64[:, sr] - m.acc[:, sr] >= (lo + 2 * m.acc[:, sr].max(1) - 2 * m.eps_ref)[:, None]).sum(1)
    assert (reach[:half] > 2 * m.k).all()


@pytest.mark.parametrize("name", ["wg_per_block_3_slices_ragged", "sorted_scores_thr", "clustered_row_exact_thr", "band_overflow_copies"])
def test_an_ideal_filter_satisfies_the_model(name):
    """A filter without any accumulation error (s~ = fp32(st64)), the library's eps formula evaluated in fp64 with its safety factors and the
    selection rules of sample_threshold_query, simulated in numpy, passes every check the GPU test makes: the model does not contradict the design."""
    c, plan, m = _model(name)
    k = c["k"]
    st = m.st64.astype(np.float32).astype(np.float64)
    assert (np.abs(st - m.st64) <= m.acc).all()
    eps = m.eps_hi / (1 + m.D * 2.0 ** -25 + 9 * 2.0 ** -24)                     # every written safety factor, exact arithmetic
    assert (m.eps_ref <= eps).all() and (eps <= m.eps_hi).all()
    sr = m.sample_rows
    g = m.threshold_grouping()
    ss = st[:, sr]
    if g == 1:
        kth = np.sort(ss, axis=1)[:, -k]
    else:
        gid = sr // g
        starts = np.flatnonzero(np.r_[True, gid[1:] != gid[:-1]])
        kth = np.sort(np.maximum.reduceat(ss, starts, axis=1), axis=1)[:, -k]
    thr = kth - 2 * eps
    if plan["group_rows"] == 16:                                                # the row-exact branch
        for qi in range(m.Q):
            hits = ss[qi][ss[qi] >= thr[qi]]
            if hits.size > 2 * k:
                thr[qi] = max(thr[qi], np.sort(hits)[-k] - 2 * eps[qi])
    lo, hi = m.threshold_bounds()
    T = thr + 2 * eps
    assert (lo <= T).all() and (T <= hi).all()
    must, must_not = m.list_must(thr)
    listed = st >= thr[:, None]
    assert (listed | ~must).all() and not (listed & must_not).any()
    kth_all = np.sort(st, axis=1)[:, -k]
    band = (st >= (kth_all - 2 * eps)[:, None]).sum(1)
    blo, bhi = m.band_count_bounds(eps, eps)
    assert (blo <= band).all() and (band <= bhi).all()
    llo, lhi = m.list_count_bounds(thr, thr)
    assert (llo <= listed.sum(1)).all() and (listed.sum(1) <= lhi).all()
    top = np.argsort(-m.s64, axis=1, kind="stable")[:, :k]
    assert np.take_along_axis(listed, top, axis=1).all()                        # the exact top-k survives the filter
