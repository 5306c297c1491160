"""Host-side checks of tests/gemm_reference.py: the reference agrees with what is already pinned (the oracle, the expectations the existing GEMM
tests compute inline), the accumulator of every GPU case is exact in fp32 in two summation orders, the comparison rule exempts at most 2 %
of any case (nothing where the budget is zero), and the rule has teeth: a float32 stand-in of each epilogue passes it, every listed mutant of
the stand-in fails it.  The fp16-operand / fp16-output cases (GR.gpu_cases_f16) on top of that: their operands are fp16-exact without
subnormals, and for every fp16 output the rule rejects the two likeliest wrong kernels computed from the reference itself -- the value
rounded through bf16 first, and (on the saturation inputs) the store without the clamp."""
import functools

import numpy as np
import pytest

import gemm_reference as GR
from oracle import lrx_oracle as O

CASES = GR.gpu_cases()
IDS = [c["name"] for c in CASES]
CASES_F16 = GR.gpu_cases_f16()
IDS_F16 = [c["name"] for c in CASES_F16]


@functools.lru_cache(maxsize=None)
def _case(name):
    case = CASES[IDS.index(name)] if name in IDS else CASES_F16[IDS_F16.index(name)]
    inp = GR.case_inputs(case)
    return case, inp, GR.case_reference(case, inp)


# ---------------------------------------------------------------------------------------------------------------
# the reference against what is already pinned
# ---------------------------------------------------------------------------------------------------------------
def test_store_resid_and_max_aggregate_equal_the_oracle_on_exact_operands():
    rng = np.random.default_rng(0)
    A, B = GR.exact_operands(rng, 37, 24, 128)
    bias, R = rng.integers(-8, 9, 24).astype(np.float32), rng.integers(-8, 9, (37, 24)).astype(np.float32)
    np.testing.assert_array_equal(GR.store(A, B)[0], O._mm(A, B, bf16=True))
    np.testing.assert_array_equal(GR.store(A, B, bias)[0], O.round_bf16(A @ B.T + bias))
    np.testing.assert_array_equal(GR.resid(A, B, R)[0], O.round_bf16(O.round_bf16(A @ B.T) + R))          # tests/test_gpu_kernels.py::test_gemm_residual_inplace
    cu, mask = np.array([0, 5, 5, 30, 37]), (rng.random(37) < 0.7).astype(np.uint8)
    out, _, _ = GR.max_aggregate(A, B, bias, GR.row_segments(cu, mask), 4)
    np.testing.assert_array_equal(out, O.max_aggregate_packed(A, cu, mask, B, bias, bf16=True))
    assert (out[1] == GR.BF16_MIN).all()
    x0, gamma = rng.standard_normal((37, 24)).astype(np.float32), O.round_bf16(rng.standard_normal(24).astype(np.float32))
    x, a16, _, _, _, ss = GR.resid32(A, B, x0, gamma)
    np.testing.assert_array_equal(x, (x0.astype(np.float64) + A.astype(np.float64) @ B.astype(np.float64).T).astype(np.float32))
    np.testing.assert_array_equal(a16, O.round_bf16(x.astype(np.float32) * gamma))                       # ::test_precise_stream_residual_gemm
    np.testing.assert_allclose(ss.sum(0), (x ** 2).sum(1), rtol=1e-14)


def test_swiglu_equals_the_inline_expectation_and_the_interleave_of_the_encoder():
    import torch
    from lightretriever_amd.encoder import interleave_gate_up
    rng = np.random.default_rng(1)
    A, Wg = GR.exact_operands(rng, 20, 32, 64, b_scale=GR.swiglu_b_scale(64))
    _, Wu = GR.exact_operands(rng, 1, 32, 64, b_scale=GR.swiglu_b_scale(64))
    Bi = GR.interleave_gate_up(Wg, Wu)
    np.testing.assert_array_equal(Bi, interleave_gate_up(torch.from_numpy(Wg), torch.from_numpy(Wu)).numpy())
    g, u = A.astype(np.float64) @ Wg.T, A.astype(np.float64) @ Wu.T
    np.testing.assert_allclose(GR.swiglu(A, Bi)[1], g / (1 + np.exp(-g)) * u, rtol=1e-13)                # ::test_gemm_swiglu
    np.testing.assert_allclose(GR.swiglu(A, Bi)[1], O._silu(g.astype(np.float32)) * u, rtol=1e-5, atol=1e-6)
    rs = rng.uniform(0.2, 3.0, 20)
    np.testing.assert_allclose(GR.swiglu(A, Bi, rs)[1], (g * rs[:, None]) / (1 + np.exp(-g * rs[:, None])) * (u * rs[:, None]), rtol=1e-13)
    assert 0.5 < np.abs(g).std() < 8 and (np.abs(g) < 8).mean() > 0.8 and np.abs(g).max() > 8


@pytest.mark.parametrize("d,nq,nkv", [(64, 2, 1), (128, 2, 2)])
def test_qkv_rope_equals_hf_rotary_in_logical_order(d, nq, nkv):
    import torch
    from lightretriever_amd import ops
    perm = GR.rotary_pair_order(nq, nkv, d)
    np.testing.assert_array_equal(perm, ops.rotary_pair_order(nq, nkv, d).numpy())
    rng = np.random.default_rng(d)
    T, K, N = 9, 64, (nq + 2 * nkv) * d
    A, Wl = GR.exact_operands(rng, T, N, K)
    bl, rs = GR.bf16_values(rng, N), rng.uniform(0.2, 3.0, T)
    cos, sin = GR.rope_table(d, 32)
    pos = rng.integers(0, 32, T)
    t = (A.astype(np.float64) @ Wl.T.astype(np.float64)) * rs[:, None] + bl                             # ::test_gemm_qkv_rope_fused_equals_fp32_projection_then_rope
    qk = t[:, :(nq + nkv) * d].reshape(T, nq + nkv, d)
    c, s = cos[pos].astype(np.float64)[:, None, :], sin[pos].astype(np.float64)[:, None, :]
    x1, x2 = qk[..., :d // 2], qk[..., d // 2:]
    want = np.concatenate([np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(T, -1), t[:, (nq + nkv) * d:]], 1)
    got, pre, _ = GR.qkv_rope(A, Wl[perm], pos, cos, sin, nq, nkv, d, bl[perm], rs)
    logical = np.empty_like(pre)
    logical[:, perm] = pre
    np.testing.assert_allclose(logical, want, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(logical[:, :(nq + nkv) * d].reshape(T, nq + nkv, d), O.apply_rope(qk.astype(np.float32), cos[pos], sin[pos]), rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(got, pre.astype(np.float16).astype(np.float64))
    # a head slice is the columns of the full call; saturation
    np.testing.assert_array_equal(GR.qkv_rope(A, Wl[perm], pos, cos, sin, nq, nkv, d, bl[perm], rs, nq, 2 * nkv)[1], pre[:, nq * d:])
    np.testing.assert_array_equal(GR.qkv_rope(A * 2.0 ** 14, Wl[perm], pos * 0, cos, sin, nq, nkv, d)[0].max(), 65504.0)


# ---------------------------------------------------------------------------------------------------------------
# every GPU case: exact accumulator, exemption cap
# ---------------------------------------------------------------------------------------------------------------
def _two_orders(A, B):
    A, B = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)
    fwd = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k in range(A.shape[1]):                                      # forward, one k at a time: every partial sum rounded to fp32
        fwd += A[:, k, None] * B[None, :, k]
    parts = [A[:, t:t + GR.GBK] @ B[:, t:t + GR.GBK].T for t in range(0, A.shape[1], GR.GBK)]   # per 64-wide K-tile (float32), then pairwise
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return fwd, parts[0]


@pytest.mark.parametrize("name", IDS + IDS_F16)
def test_accumulator_is_exact_and_the_rule_exempts_little(name):
    case, inp, ref = _case(name)
    if name in IDS_F16:
        # what the bf16 cases cannot require: the operands survive the conversion to fp16 unchanged, none of them subnormal (the subnormal
        # probe is a test of its own), and the same arrays serve the bf16 case of the same shape
        assert GR.is_fp16_exact(inp["A"]) and GR.is_fp16_exact(inp["B"]), name
        assert not GR.has_fp16_subnormals(inp["A"]) and not GR.has_fp16_subnormals(inp["B"]), name
        if "base" in case:
            base = _case(case["base"])[1]
            assert all(np.array_equal(inp[k], base[k]) if inp[k] is not None else base[k] is None for k in inp), name
        if case.get("wide"):
            assert not (O.round_bf16(inp["A"]) == inp["A"]).all() and np.abs(inp["A"]).max() * 2 ** 10 > 1000, "the wide family must not be bf16-exact"
    units, _ = GR.sum_units(inp["A"], inp["B"])
    assert units < 2 ** 24
    fwd, pair = _two_orders(inp["A"], inp["B"])
    acc = GR.acc64(inp["A"], inp["B"])
    assert (fwd.astype(np.float64) == acc).all() and (pair.astype(np.float64) == acc).all()
    for key, val in ref.items():
        if key == "ss":
            continue
        _, pre, budget, fmt = val
        share = GR.exempt_share(pre, budget, fmt, f"{name} {key}")
        print(f"{name} {key}: exempt share {share:.5f}, largest budget {float(np.max(budget)):.3e}")
        if case["family"] == "exact":
            assert share == 0.0 and not np.any(budget), name
    if case["epi"] == "swiglu":
        g = acc[:, GR.gate_up_columns(case["N"])[0]] * (1.0 if inp["rscale"] is None else inp["rscale"].astype(np.float64)[:, None])
        assert (np.abs(g) < 8).mean() > 0.6 and np.abs(g).max() < 80, ((np.abs(g) < 8).mean(), np.abs(g).max())


@pytest.mark.parametrize("name", IDS_F16)
def test_fp16_outputs_tell_a_rounding_through_bf16_from_the_right_answer(name):
    """the likeliest wrong kernel of an fp16 store: fp16(bf16(x)), a conversion that went through the bf16 path first"""
    case, inp, ref = _case(name)
    n = 0
    for key, val in ref.items():
        if key != "ss" and val[3] == "fp16":
            want, pre, budget, fmt = val
            GR.check(want, pre, budget, fmt, f"{name} {key}")
            with pytest.raises(AssertionError):
                GR.check(GR.fp16_round(GR.bf16_round(pre)), pre, budget, fmt, f"{name} {key}")
            # ... and not by a hair: the mutant differs in far more elements than the rule exempts
            assert (GR.fp16_round(GR.bf16_round(pre)) != want).mean() > 0.25, name
            n += 1
    assert n == (0 if case.get("no_a16") else 1)


def test_fp16_swiglu_outputs_reach_into_the_subnormals():
    """0.1 % to 0.8 % of the SwiGLU outputs at K >= 192 are fp16 subnormals: the conversion's subnormal rounding is exercised"""
    shares = {}
    for name in IDS_F16:
        case, inp, ref = _case(name)
        if case["epi"] == "swiglu":
            want = np.abs(ref["C"][0])
            shares[name] = float(((want > 0) & (want < 2.0 ** -14)).mean())
    print(shares)
    assert sum(v >= 1e-3 for v in shares.values()) >= 4 and max(shares.values()) < 1e-2


@pytest.mark.parametrize("which", GR.SATURATION)
def test_saturation_inputs_tell_a_store_without_the_clamp_from_the_right_answer(which):
    case, inp, ref = GR.saturation_inputs(which)
    key = "C" if case["epi"] == "swiglu" else "a16"
    want, pre, budget, fmt = ref[key]
    with np.errstate(all="ignore"):
        out = ~(np.abs(pre) <= 65504)
        assert fmt == "fp16" and np.isfinite(want).all() and out.sum() >= 100 and np.isnan(pre).any()
        assert (want[out & (pre > 0)] == 65504).all() and (want[out & ~(pre > 0)] == -65504).all()         # by sign; NaN as -65504
        assert (want == 65504).any() and (want[~np.isnan(pre)] == -65504).any() and (np.abs(want[~out]) < 65504).all() and (~out).mean() > 0.9
        GR.check(want, pre, budget, fmt, which)
        with pytest.raises(AssertionError):
            GR.check(GR.fp16_ieee(pre), pre, budget, fmt, which)
        with pytest.raises(AssertionError):                              # a clamp that lets the NaN through
            GR.check(np.where(np.isnan(pre), np.nan, want), pre, budget, fmt, which)


def test_wide_and_subnormal_probes_are_what_their_docstrings_say():
    A, B = GR.one_hot_rows_wide(300, 264, 192)
    assert GR.is_fp16_exact(B) and (O.round_bf16(B) != B).mean() > 0.8 and np.abs(B).min() >= 1024 and np.abs(B).max() <= 2046
    np.testing.assert_array_equal(GR.acc64(A, B), B[:, (37 * np.arange(300) + 11) % 192].T)
    A, B = GR.subnormal_probe(300, 128)
    j = np.abs(B.astype(np.float64)) * 2.0 ** 24
    assert GR.is_fp16_exact(B) and sorted(set(j.ravel().tolist())) == list(range(1, 1024)) and (np.abs(B) < 2.0 ** -14).all()
    np.testing.assert_array_equal(GR.acc64(A, B), B[:, (37 * np.arange(300) + 11) % 128].T.astype(np.float64))


@pytest.mark.parametrize("M,N", GR.TILE_MAP)
def test_probe_operands_are_exact_and_decode(M, N):
    A, B = GR.coded_operands(M, N)
    fwd, pair = _two_orders(A, B)
    acc = GR.acc64(A, B)
    assert (fwd == acc).all() and (pair == acc).all() and (GR.store(A, B)[0] == acc).all()              # a bf16 number: stored as it is
    m, n = M - 1, N - 1
    assert f"row = {m % 199} mod 199 and a column = {n % 127} mod 127" in GR.decode_coded((m, n), acc[m, n])
    A, B = GR.one_hot_rows(300, 264, 192)
    np.testing.assert_array_equal(GR.acc64(A, B), B[:, (37 * np.arange(300) + 11) % 192].T)
    A, B = GR.identity_operands(320, 264)
    np.testing.assert_array_equal(GR.store(A, B)[0], B.T)


# ---------------------------------------------------------------------------------------------------------------
# the rule has teeth: a float32 stand-in of each epilogue passes, its mutants do not
# ---------------------------------------------------------------------------------------------------------------
def _acc32(A, B, drop_last=False, twice=None):
    tiles = list(range(0, A.shape[1], GR.GBK))
    if drop_last:
        tiles = tiles[:-1]
    if twice is not None:
        tiles.append(tiles[twice])
    acc = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for t in tiles:
        acc += A[:, t:t + GR.GBK].astype(np.float32) @ B[:, t:t + GR.GBK].astype(np.float32).T
    return acc


def _bf(x):
    return O.round_bf16(np.asarray(x, np.float32))


def _h(x):
    return np.clip(np.asarray(x, np.float32), np.float32(-65504), np.float32(65504)).astype(np.float16)


def standin(case, inp, mutant=None):
    """the epilogue in numpy float32, step by step as the kernel does it -> {output: array}"""
    epi = case["epi"]
    acc = _acc32(inp["A"], inp["B"], drop_last=mutant == "drop_last_k_tile", twice=1 if mutant == "k_tile_twice" else None)
    if epi == "store":
        rs, bias = inp["rscale"][:, None], inp["bias"][None, :]
        if mutant == "bias_after_rounding":
            C = _bf(_bf(acc * rs) + bias)
        elif mutant == "rscale_after_bias":
            C = _bf((acc + bias) * rs)
        else:
            C = _bf(acc * rs + bias)
        if mutant == "tile_transposed":
            C[:64, :64] = C[:64, :64].T.copy()
        return {"C": C}
    if epi == "resid":
        C = _bf(acc + inp["R"]) if mutant == "resid_before_inner_rounding" else _bf(_bf(acc) + inp["R"])
        sq = (_bf(acc) if mutant == "ss_before_resid" else C).astype(np.float64) ** 2
        return {"C": C, "ss": GR.tile_sums(sq, case["N"])}
    if epi == "swiglu":
        gc, uc = GR.gate_up_columns(case["N"])
        if mutant == "gate_up_swapped":
            gc, uc = uc, gc
        rs = np.float32(1) if inp["rscale"] is None else inp["rscale"][:, None]
        g, u = acc[:, gc] * rs, acc[:, uc] * rs
        sg = np.float32(1) / (np.float32(1) + np.exp2(g * np.float32(-1.4426950408889634)))
        t = g * sg * u
        if mutant == "through_bf16":
            t = _bf(t)
        return {"C": _h(t) if case.get("f16") else _bf(t)}
    if epi == "resid32":
        x = inp["x32"] + acc
        t = x * inp["gamma"][None, :]
        if mutant == "through_bf16":
            t = _bf(t)
        out = {"x32": x, "a16": _h(t) if case.get("out_f16") else _bf(t), "ss": GR.tile_sums(x.astype(np.float64) ** 2, case["N"])}
        if case.get("no_a16"):
            del out["a16"]
        return out
    if epi == "rope":
        d, nq, nkv = case["d"], case["nq"], case["nkv"]
        x = acc
        if inp["rscale"] is not None:
            x = x * inp["rscale"][:, None]
        if inp["bias"] is not None:
            x = x + inp["bias"][None, :]
        out = x.copy()
        cos, sin = inp["cos"][inp["positions"]], inp["sin"][inp["positions"]]
        sign = np.float32(-1 if mutant == "rotation_sign_flipped" else 1)
        for h in range(nq + nkv):                                    # physical order: columns 32 g + t and 32 g + 16 + t are the pair j = 16 g + t
            for g in range(d // 32):
                c0 = h * d + 32 * g
                if mutant == "partner_j_plus_16":                    # logical j pairs with j + 16: physical block g' = g ^ 1's first half for odd ...
                    pair0 = h * d + 32 * (g ^ 1)                     # (for d = 128: the partner column comes from the neighbouring 32-block)
                    a, b = x[:, c0:c0 + 16], x[:, pair0:pair0 + 16]
                else:
                    a, b = x[:, c0:c0 + 16], x[:, c0 + 16:c0 + 32]
                c, s = cos[:, 16 * g:16 * g + 16], sin[:, 16 * g:16 * g + 16]
                out[:, c0:c0 + 16] = a * c - sign * b * s
                out[:, c0 + 16:c0 + 32] = b * c + sign * a * s
        return {"C": np.clip(out, -65504, 65504).astype(np.float16)}
    raise KeyError(epi)


def _judge(case, inp, ref, got):
    for key, val in ref.items():
        if key == "ss":
            GR.check_ss(got["ss"], val[0], val[1], f"{case['name']} ss")
        else:
            GR.check(got[key], val[1], val[2], val[3], f"{case['name']} {key}")


STANDIN_CASES = ["store-exact-129x504x192", "store-general-129x504x192", "resid-exact-129x504x192", "resid-general-255x520x256", "swiglu-129x544x192",
                 "resid32-general-128x264x64", "rope-d128-q2kv1-b1r1-127x192", "rope-d64-q4kv2-b0r0-257x64", "rope-d64-q4kv2-b0r0-257x64-pos0",
                 "f16-swiglu-129x544x192", "resid32-f1h1-general-128x264x64", "resid32-f0h1-exact-129x504x192", "resid32-f1h1-wide-300x264x512",
                 "resid32-f1h1-noa16-exact-129x504x192", "kloop-resid32-f1h1-nk5", "f16-rope-d128-q2kv1-b1r1-127x192"]
MUTANTS = [("store-exact-129x504x192", "drop_last_k_tile"), ("store-exact-129x504x192", "k_tile_twice"), ("store-exact-129x504x192", "bias_after_rounding"),
           ("store-general-129x504x192", "bias_after_rounding"), ("store-exact-129x504x192", "rscale_after_bias"), ("store-general-129x504x192", "rscale_after_bias"),
           ("resid-exact-129x504x192", "resid_before_inner_rounding"), ("swiglu-129x544x192", "gate_up_swapped"),
           ("rope-d128-q2kv1-b1r1-127x192", "rotation_sign_flipped"), ("rope-d128-q2kv1-b1r1-127x192", "partner_j_plus_16"),
           ("store-exact-129x504x192", "tile_transposed"), ("resid-exact-129x504x192", "ss_before_resid"),
           ("f16-swiglu-129x544x192", "through_bf16"), ("f16-swiglu-129x544x192", "gate_up_swapped"), ("resid32-f1h1-general-128x264x64", "through_bf16"),
           ("resid32-f0h1-exact-129x504x192", "through_bf16"), ("resid32-f1h1-wide-300x264x512", "drop_last_k_tile"),
           ("kloop-resid32-f1h1-nk5", "k_tile_twice"), ("f16-rope-d128-q2kv1-b1r1-127x192", "rotation_sign_flipped")]


@pytest.mark.parametrize("name", STANDIN_CASES)
def test_float32_standin_passes(name):
    case, inp, ref = _case(name)
    _judge(case, inp, ref, standin(case, inp))


@pytest.mark.parametrize("name,mutant", MUTANTS)
def test_mutant_of_the_standin_fails(name, mutant):
    case, inp, ref = _case(name)
    with pytest.raises(AssertionError):
        _judge(case, inp, ref, standin(case, inp, mutant))
