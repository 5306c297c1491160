"""The fp64 model of the 8-bit index's filter stages (sq8_stage_reference.py) against itself and the yardstick, the preconditions of every
case of test_gpu_sq8_stages.py on the model alone -- what a case claims to exercise holds before any GPU sees it -- and the host-only
layout entry lrx_sq8_ip_workspace_layout.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import sq8_stage_reference as R
import sq8_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _good(name):
    m = R.case_model(name)
    g = R.good_queries(name)
    return m, g


def test_layout_entry_is_declared_and_agrees_with_the_sizes():
    from lightretriever_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lrx.h")).read()
    assert "#define LRX_ABI_VERSION 9" in hdr and _lib.ABI_VERSION == 9
    assert "#define LRX_SQ8_LAYOUT_INTS 12" in hdr
    assert "int lrx_sq8_ip_workspace_layout(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int64_t out[LRX_SQ8_LAYOUT_INTS]);" in hdr
    assert len(_lib.SIGNATURES["lrx_sq8_ip_workspace_layout"][1]) == 5
    lib = _lib.lib()
    assert lib.lrx_abi_version() == 9
    out = (C.c_int64 * 12)()
    for n, d, Q, k in [(300, 64, 17, 10), (1, 64, 1, 10), (500, 256, 129, 10), (2 * 2048 * 128 + 77, 64, 17, 10), (1000, 1024, 128, 100),
                       (10_000_000, 256, 100, 100), (5_000_000, 2048, 1000, 1000), (129, 192, 33, 2048)]:
        assert lib.lrx_sq8_ip_workspace_layout(n, d, Q, k, out) == 0
        qc, rc, ld, nblk_ld, qpad, dig, sc, bi, ep, mat, bm, total = list(out)
        assert qc == lib.lrx_sq8_ip_chunk_queries(n, d, Q, k) and 1 <= qc <= min(Q, 128) and total == lib.lrx_sq8_ip_workspace_bytes(n, d, Q, k)
        assert qc == min(Q, 128) or n > (1 << 21)                     # (fewer only where the 1 GiB matrix budget decides)
        assert rc == min(n, 1 << 22) and ld == -(-rc // 128) * 128 and nblk_ld >= ld // 128 and nblk_ld % 4 == 0
        tiles = -(-qc // 16)
        assert qpad == 16 * (1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 8) and qpad >= qc
        # the regions lie in this order, 256-byte aligned, and none overlaps the next
        assert dig == 0 and dig + qpad * d * 2 <= sc and sc + qc * 8 <= bi and bi + qc * 8 <= ep and ep + qc * 4 <= mat
        assert mat + qc * ld * 4 <= bm and bm + qc * nblk_ld * 4 <= total
        assert all(o % 256 == 0 for o in (sc, bi, ep, mat, bm))
    for bad in [(300, 65, 17, 10), (300, 64, 0, 10), (300, 64, 17, 0), (-1, 64, 17, 10)]:
        assert lib.lrx_sq8_ip_workspace_layout(*bad, out) != 0
    assert lib.lrx_sq8_ip_workspace_layout(300, 64, 17, 10, None) != 0


def test_model_decode_and_scores_equal_the_yardstick():
    for name in ("d64", "d576_uniform", "subnormal", "offset", "const_cols"):
        trained, codes, q = R.case_data(name)
        m = R.case_model(name)
        dec = Y.decode(codes, trained)
        assert np.array_equal(m.s64, q.astype(np.float64) @ dec.astype(np.float64).T)
        assert np.array_equal(m.s.view(np.int32), Y.scores(q, codes, trained).view(np.int32))
        vmin, vdiff = R.split(trained, codes.shape[1])
        assert np.array_equal(dec, vmin + ((codes.astype(np.float32) + np.float32(0.5)) / np.float32(255)) * vdiff)


@pytest.mark.parametrize("name", list(R.CASES))
def test_digits_and_bound_of_every_case(name):
    """hi / lo are int8 digits of n, n is within a half of w / scale, and |v - s64| <= eps_ref for every pair."""
    m, g = _good(name)
    c = R.case_spec(name)
    assert (np.abs(m.hi[g]) <= 127).all() and (m.lo[g] >= -64).all() and (m.lo[g] <= 63).all() and (128 * m.hi[g] + m.lo[g] == m.n[g]).all()
    assert (np.abs(m.rho[g]) <= 0.5 * m.scale[g][:, None] * (1 + 2.0 ** -40)).all()
    assert (np.abs(m.w[g]).max(1) <= m.scale[g] * R.NMAX).all() and (m.scale[g] * R.NMAX <= np.abs(m.w[g]).max(1) * (1 + 2.0 ** -21)).all()
    r = m.ratio()[g]
    print(f"\n{name}: worst |v - s64| / eps_ref = {r.max():.4f}; terms of eps (worst query share): quantisation "
          f"{(m.terms[0][g] / np.maximum(sum(m.terms)[g], 1e-300)).max():.3f}, decode {(m.terms[1][g] / np.maximum(sum(m.terms)[g], 1e-300)).max():.3f}, "
          f"subnormal {(m.terms[2][g] / np.maximum(sum(m.terms)[g], 1e-300)).max():.2e}")
    assert np.isfinite(m.v[g]).all() and np.isfinite(m.s64[g]).all()
    assert (np.abs(m.v[g] - m.s64[g]) <= m.eps_ref[g].astype(np.float64)[:, None]).all()
    for z in c["zero"]:
        assert m.scale[z] == 0 and not m.n[z].any() and m.eps_ref[z] == 0 and m.bias[z] == 0 and not m.v[z].any() and not m.s64[z].any()
    # the scores are normal fp32 numbers or zero: the assumption the bound is written under
    a = np.abs(m.s64[g])
    assert ((a == 0) | ((a > 2.0 ** -126) & (a < 2.0 ** 127))).all()


@pytest.mark.parametrize("name", R.ALIGNED)
def test_aligned_rows_come_within_a_tenth_of_the_bound(name):
    m = R.case_model(name)
    r = m.ratio()
    ab = np.stack([r[np.arange(m.Q), 2 * np.arange(m.Q)], r[np.arange(m.Q), 2 * np.arange(m.Q) + 1]])
    print(f"\n{name}: |v - s64| / eps_ref of rows A {np.round(ab[0], 4)}, rows B {np.round(ab[1], 4)}; random rows {r[:, 2 * m.Q:].max():.4f}")
    assert (ab >= 0.9).all() and (ab <= 1).all()


@pytest.mark.parametrize("name", R.BAND_EDGE)
def test_band_edge_preconditions(name):
    c = R.case_spec(name)
    m = R.case_model(name)
    k = c["k"]
    U, others = R.band_edge_rows(c)
    qi = np.arange(m.Q)
    eps = m.eps_ref.astype(np.float64)
    kth = m.kth_filter(k)
    gap = (kth - m.v[qi, U]) / eps
    order = np.argsort(-m.s64, axis=1, kind="stable")
    top = order[:, :k]
    ftop = np.argsort(-m.v, axis=1, kind="stable")[:, :k]
    print(f"\n{name}: (k-th filter score - filter score of U) / eps_ref = {np.round(gap, 4)}")
    assert (gap > 1.25).all() and (gap <= 2).all()
    assert (top[:, 0] == U).all()                                             # U is the exact top-1 ...
    assert not (ftop == U[:, None]).any()                                     # ... and not among the filter's top-k,
    assert (np.sort(ftop, axis=1) == others).all()                            # which are the k other crafted rows, in filter order above U
    assert (m.s64[qi[:, None], others] < m.s64[qi, U][:, None]).all()         # and all of them exactly below U, in fp32 as well
    assert (m.s[qi[:, None], others] < m.s[qi, U][:, None]).all()
    assert (np.take_along_axis(m.v, top, axis=1) >= (kth - 2 * eps)[:, None]).all()
    far = np.delete(m.s64, np.concatenate([U, others.ravel()]), axis=1).max(1)   # the fillers and the rows crafted for the other queries
    assert (far < m.s64[qi[:, None], others].min(1) - 100 * eps).all()


def test_cases_exercise_what_they_name():
    S = R.case_spec
    # Q spans every k_sq8_scan<QT> at a full and a ragged tile count; the last chunk of two_chunks is a single query
    assert sorted({S(n)["Q"] for n in R.CASES} & {1, 16, 17, 33, 65, 128, 129}) == [1, 16, 17, 33, 65, 128, 129]
    assert {S(n)["n"] for n in ("rows_127", "rows_128", "rows_129")} == {127, 128, 129} and S("one_row")["n"] == 1 < S("one_row")["k"]
    assert S("d192")["d"] % 256 and S("d576_uniform")["d"] % 512 == 64 and S("grid_stride")["n"] > 2 * 2048 * 128
    assert all(S(n)["n"] <= 1000 or n in ("grid_stride", "zero_query") for n in R.CASES)
    # offset: the 2^-21 term is most of eps; subnormal: the 3 2^-149 term is several per cent of it, and most ranges are subnormal
    m = R.case_model("offset")
    assert (m.terms[1] > 0.9 * sum(m.terms)).all()
    m = R.case_model("subnormal")
    assert (m.terms[2] > 0.02 * sum(m.terms)).all()
    _, vdiff = R.split(R.case_data("subnormal")[0], 128)
    assert (vdiff < 2.0 ** -126).sum() == 96 and (vdiff >= 2.0 ** -126).sum() == 32 and (vdiff > 0).all()
    _, vdiff = R.split(R.case_data("const_cols")[0], 192)
    assert (vdiff == 0).sum() == 64
    # zero_query: every row ties, more than the 4096-entry list
    assert S("zero_query")["n"] > 4096
    q = R.case_data("nonfinite_query")[2]
    assert np.isnan(q[1]).sum() == 1 and np.isposinf(q[4]).sum() == 1 and np.isfinite(np.delete(q, [1, 4], axis=0)).all()
    # padding: the pattern does beat every stored row of every query
    trained, codes, q = R.case_data("padding")
    m = R.case_model("padding")
    pat = R.padding_pattern(q, trained, 84)
    vp, _ = R.filter_scores(m.scale, m.n, m.bias, R.centred(pat))
    assert (vp.max(1) > m.v.max(1)).all()
