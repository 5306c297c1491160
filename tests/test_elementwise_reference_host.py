"""tests/elementwise_reference.py pinned on the CPU before it judges a kernel: it agrees with the oracle (oracle/lrx_oracle.py) and, through it,
with the reference's own pooling outputs (tests/golden/pooling.npz); and the condition the GPU comparison rule relies on holds for every
input the GPU tests run -- few elements lie within the fp32 error budget of a bf16 rounding boundary."""
import os

import numpy as np
import pytest

import elementwise_reference as ER
from helpers import GOLDEN
from oracle import lrx_oracle as O

U_F32 = 2.0 ** -24


def test_bf16_rounding_is_the_oracles_and_the_neighbours_bracket():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 6, 20000), [1.0, -1.0, 255.0, 1.00390625, 1.01171875, 1.001953125]])
    v32 = v.astype(np.float32)
    np.testing.assert_array_equal(ER.bf16_round(v32), O.round_bf16(v32).astype(np.float64))          # RNE, ties to even included
    lo, hi, rel = ER.bf16_neighbours(v)
    assert (lo <= v).all() and (v <= hi).all() and (ER.bf16_round(lo) == lo).all() and (ER.bf16_round(hi) == hi).all()
    r = ER.bf16_round(v)
    assert ((r == lo) | (r == hi)).all()
    mid = (lo + hi) / 2
    fin = np.isfinite(rel)
    np.testing.assert_allclose(rel[fin], np.abs(v - mid)[fin] / np.abs(v)[fin], rtol=1e-9)
    assert ER.bf16_neighbours(1.00390625)[2] == 0.0 and ER.bf16_round(1.00390625) == 1.0 and ER.bf16_round(1.01171875) == 1.015625   # ties go to even
    np.testing.assert_array_equal(ER.fp16_round([70000.0, -1e9, 0.1]), [65504.0, -65504.0, float(np.float16(0.1))])
    # the store rule of the fp16-operand kernels: the same on every number, a NaN as -65504, subnormals rounded once (RNE at 2^-24)
    np.testing.assert_array_equal(ER.fp16_sat([70000.0, -1e9, 0.1, np.nan, np.inf, -np.inf, 65519.9, 65520.0, 3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -26]),
                                  [65504.0, -65504.0, float(np.float16(0.1)), -65504.0, 65504.0, -65504.0, 65504.0, 65504.0, 2 * 2.0 ** -24, 2 * 2.0 ** -24, 0.0])
    np.testing.assert_array_equal(ER.fp16_sat(v), ER.fp16_round(v))
    assert np.isinf(ER.fp16_ieee(65520.0)) and np.isnan(ER.fp16_ieee(np.nan)) and ER.fp16_ieee(65519.9) == 65504.0


@pytest.mark.parametrize("rows,H", [(1, 64), (37, 256), (300, 2048), (9, 4096)])
def test_rmsnorm_agrees_with_the_oracle_on_the_existing_seeds(rows, H):
    """O.rmsnorm computes rstd in fp32: its bf16 result may differ from the fp64 one only where the inner value is within the oracle's own
    fp32 error (4 u: the mean, the addition of eps, the root and reciprocal, the product) of a rounding boundary."""
    rng = np.random.default_rng(rows)
    x = O.round_bf16(rng.standard_normal((rows, H)).astype(np.float32) * 3.0)
    w = O.round_bf16(1 + 0.1 * rng.standard_normal(H).astype(np.float32))
    y, inner, outer = ER.rmsnorm_bf16(x, w, 1e-5)
    want, alt, near = ER.hf_candidates(inner, w, 8 * U_F32)
    np.testing.assert_array_equal(y, want)
    ER.assert_bf16_rule(O.rmsnorm(x, w, 1e-5, bf16=True), want, alt, near, "oracle bf16")
    np.testing.assert_allclose(O.rmsnorm(x, w, 1e-5, bf16=False), w.astype(np.float64) * inner, rtol=8 * U_F32)
    np.testing.assert_array_equal(outer, w.astype(np.float64) * ER.bf16_round(inner))
    y1, pre = ER.rmsnorm_f32(x, w, 1e-5)
    np.testing.assert_allclose(pre, w.astype(np.float64) * inner, rtol=1e-12)
    np.testing.assert_array_equal(y1, ER.bf16_round(pre))
    np.testing.assert_allclose(ER.row_rscale(x, 1e-5)[:, None] * x.astype(np.float64), inner, rtol=1e-12)
    parts = np.stack([(x[:, :H // 2].astype(np.float64) ** 2).sum(1), (x[:, H // 2:].astype(np.float64) ** 2).sum(1)])
    np.testing.assert_allclose(ER.finalize_rscale(parts, H, 1e-5), ER.row_rscale(x, 1e-5), rtol=1e-12)


@pytest.mark.parametrize("pooling", ER.POOLINGS)
def test_pool_norm_agrees_with_the_oracle_and_the_reference_pooling(pooling):
    # (1) the bare pooling against the reference's own outputs, as tests/test_gpu_kernels.py does: unit-RMS rows, identity weight, eps = 0
    g = np.load(os.path.join(GOLDEN, "pooling.npz"))
    for name in ("ragged", "allfull"):
        h, m = g[f"fn_{name}_hidden"].astype(np.float64), g[f"fn_{name}_mask"]
        np.testing.assert_allclose(O.pool_padded(g[f"fn_{name}_hidden"], m, pooling), g[f"fn_{name}_{pooling}"], atol=1e-6)
        hn = h / np.sqrt((h * h).mean(-1, keepdims=True))
        packed, cu = hn[m.astype(bool)], np.concatenate([[0], np.cumsum(m.sum(1))])
        got, _ = ER.pool_norm(packed, np.ones(hn.shape[-1]), cu, 0.0, pooling, hn.shape[-1], False, f32=True)
        # both in float64; the oracle rounds its float64 'mean' to fp32 once at the end: that one rounding
        np.testing.assert_allclose(got, O.pool_padded(hn, m, pooling).astype(np.float64), rtol=1.001 * U_F32 if pooling == "mean" else 1e-12, atol=1e-15)
    # (2) with a real norm, on the existing seeds: the fp32 oracle within its own fp32 rounding, the bf16 oracle by the rounding rule
    lens = [3, 40, 17, 129, 5]
    x, w, cu = ER.legacy_strategy_inputs(lens)
    for out_dim, normalize in ((256, True), (64, True), (256, False)):
        got, info = ER.pool_norm(x, w, cu, 1e-5, pooling, out_dim, normalize, f32=True)
        pooled = O.pool_packed(O.rmsnorm(x, w, 1e-5, bf16=False), cu, pooling)[:, :out_dim]
        o32 = O.l2_normalize(pooled) if normalize else pooled
        # the oracle's fp32 steps: the norm (8 u), for 'mean' a sum of up to 129 fp32 terms and a division, the fp32 L2 norm of <= 256 terms
        scale = np.abs(info["normed"][:, :out_dim]).max() if not normalize else 1.0
        np.testing.assert_allclose(o32, got, rtol=0, atol=(8 + 131 + 260) * U_F32 * scale)
        got16, info16 = ER.pool_norm(x, w, cu, 1e-5, pooling, out_dim, False, f32=False)
        want16 = O.pool_packed(O.rmsnorm(x, w, 1e-5, bf16=True), cu, pooling)[:, :out_dim]
        lo, hi, share = ER.pool_allowed(info16, w, 256, out_dim, f32=False)
        assert share <= ER.NEAR_CAP
        if pooling == "mean":
            assert ((want16 >= lo - 131 * U_F32 * np.abs(lo)) & (want16 <= hi + 131 * U_F32 * np.abs(hi))).all()
        else:
            assert ((want16 == lo) | (want16 == hi)).all()
            np.testing.assert_array_equal(np.where(lo == hi, got16, want16), want16)
        if normalize:
            np.testing.assert_allclose(ER.pool_norm(x, w, cu, 1e-5, pooling, out_dim, True, f32=False)[0], O.l2_normalize(got16).astype(np.float64),
                                       rtol=0, atol=300 * U_F32)
    if pooling == "lasttoken":
        np.testing.assert_array_equal(ER.pool_norm(x, w, cu, 1e-5, pooling, 256, False, f32=False)[0],
                                      O.lasttoken_pool_packed(ER.rmsnorm_bf16(x, w, 1e-5)[0], cu))


def test_impossible_sequences_and_the_shard_form():
    x, w, _ = ER.pool_inputs(64, False, (3, 4))
    for pooling in ER.POOLINGS:
        out, info = ER.pool_norm(x, w, [0, 3, 3, 7], 1e-5, pooling, 64, True, f32=False)
        ref, _ = ER.pool_norm(x, w, [0, 3, 7], 1e-5, pooling, 64, True, f32=False)
        assert info["tokens"][1] is None and (out[1] == 0).all()
        np.testing.assert_array_equal(out[[0, 2]], ref)
    assert ER.pooled_tokens([0, 1, 3, 6], "third_to_last") == [None, None, [3]] and ER.pooled_tokens([0, 1, 3], "second_to_last") == [None, [1]]
    rows = np.array([[3.0, 4.0], [70000.0, 0.1]])
    r, e, sh = ER.shard_bounds(rows)
    assert r == np.sqrt(70000.0 ** 2 + 0.01) and sh[1, 0] == 65504.0
    np.testing.assert_allclose(e, np.sqrt((70000.0 - 65504.0) ** 2 + (0.1 - float(np.float16(0.1))) ** 2), rtol=1e-12)
    src, cu = ER.gather_inputs(8, 4)
    g, empty = ER.gather_last_rows(src, cu)
    np.testing.assert_array_equal(g, src[cu[1:] - 1])
    assert not any(empty) and ER.gather_last_rows(src, [0, 0, 2])[1] == [True, False] and (ER.gather_last_rows(src, [0, 0, 2])[0][0] == 0).all()
    dst = np.full((int(cu[-1]), 16), -7.0, np.float32)
    d2, _ = ER.scatter_last_rows(g, cu, dst)
    assert (d2[cu[1:] - 1, :8] == g).all() and (d2[:, 8:] == -7.0).all() and (d2 != -7.0).sum() == g.size
    x3, a16, rs = ER.embed_stream32(*ER.embed_inputs(8), 1e-5)
    assert (x3[2:4] == 0).all() and (a16[2:4] == 0).all() and np.allclose(rs[2:4], 1e-5 ** -0.5)
    # the fp16 operand of the same inputs: x32 and rs unchanged; a16 is NOT the bf16 operand converted, on most elements, at every GPU shape
    for H in ER.EMBED_H:
        table, ids, gamma = ER.embed_inputs(H)
        xb, ab, rb = ER.embed_stream32(table, ids, gamma, 1e-5)
        xh, ah, rh = ER.embed_stream32(table, ids, gamma, 1e-5, f16=True)
        np.testing.assert_array_equal(xb, xh), np.testing.assert_array_equal(rb, rh)
        assert (ah != ER.fp16_round(ab)).mean() > 0.5 and np.abs(ah).max() < 65504 and (ah[2:4] == 0).all()
        np.testing.assert_array_equal(ah, (xh * gamma.astype(np.float64)).astype(np.float16).astype(np.float64))


def test_exact_probes_are_exact_in_the_reference_too():
    x, w = ER.probe_inputs(9, 896)
    y, inner, _ = ER.rmsnorm_bf16(x, w, 0.0)
    np.testing.assert_array_equal(y, w.astype(np.float64) * x)
    np.testing.assert_array_equal(ER.bf16_round(w), w)                                    # the weights are bf16 numbers
    assert len({tuple(r) for r in x}) == 9 and len(set(w.tolist())) == 896          # rows and columns are told apart
    cu = np.concatenate([[0], np.cumsum([4, 8, 16, 64, 4])])
    xm, wm = ER.probe_inputs(int(cu[-1]), 64, seed=1)
    out, _ = ER.pool_norm(xm, wm, cu, 0.0, "mean", 64, False, f32=False)
    np.testing.assert_array_equal(out, np.stack([(wm.astype(np.float64) * xm[a:b]).mean(0) for a, b in zip(cu[:-1], cu[1:])]))
    np.testing.assert_array_equal(out.astype(np.float32), out)                            # ... and fp32 numbers: nothing for a kernel to round


def test_few_elements_of_the_gpu_inputs_are_near_a_rounding_boundary():
    """The GPU rule lets a near-boundary element be either neighbour: that is only a strict test while such elements are rare.  Every input
    of the GPU files, with the budget the GPU files use (ER.rstd_budget), stays under ER.NEAR_CAP -- in fact near what the budget predicts
    (2 budget / 2^-8 .. 2^-7 spacing: 0.1 % at H = 64, 0.3 % at H = 8192)."""
    n = 0
    for name, near in ER.near_share_cases():
        share = float(near.mean())
        assert share <= ER.NEAR_CAP, (name, share)
        assert share <= 0.005, (name, share)
        n += 1
    assert n == len(ER.RMSNORM_H) + len(ER.RMSNORM_F32_H) + len(ER.POOL_H) + 1 + 4 + 2 + 1
