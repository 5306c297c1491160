"""k_gemm_bf16_nt (lrx_gemm.hip) and its six exported epilogues against tests/gemm_reference.py: operands whose accumulator is exact in fp32
(small integers times a power of two), so that everything behind the accumulator is required BIT FOR BIT at any K -- the K-loop tails
(nk = 1, 2, 3, 4, 5, 7, 128), the workgroup -> tile map (coded probes that name the tile a value came from), every M % 256 / N % 256 edge of
every epilogue, head slices, guards around every output, the refusals, saturation.  Only where an fp32 epilogue step is inexact (arbitrary
rscale / bias, SwiGLU, RoPE away from position 0) may an element within its derived budget of a rounding boundary be the other neighbour;
tests/test_gemm_reference_host.py proves that this exempts at most 2 % of a case (measured: at most 0.16 %) and nothing of the exact family.

Every output lives inside a larger allocation filled with a sentinel; nothing outside its logical block may change.

The fp16-operand and fp16-output instantiations (lrx_gemm_nt_fused_ex, lrx_gemm_qkv_rope_slice_ex, lrx_gemm_nt_resid32_ex: what the encoder
launches under precise_stream = 2 and 3) are pinned here too, by the same rule with "fp16" as the output format (GR.gpu_cases_f16, the wide-mantissa
and subnormal probes, saturation, refusals).  The search instantiations are pinned by tests/test_gpu_search_stages.py.

Set LRX_GEMM_REFERENCE_PROFILE=<file> to have one JSON line per case written there (exempt share, mismatches against round(pre), the
largest distance of such an element from its boundary in budgets)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import gemm_reference as GR

pytestmark = pytest.mark.gpu

GUARD = 4096
S = GR.SENTINEL
_FIGURES = []
CASES = GR.gpu_cases()
IDS = [c["name"] for c in CASES]
CASES_F16 = GR.gpu_cases_f16()
IDS_F16 = [c["name"] for c in CASES_F16]


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("LRX_GEMM_REFERENCE_PROFILE")
    if path:
        with open(path, "w") as f:
            for r in _FIGURES:
                f.write(json.dumps(r) + "\n")


def _record(case, key, fig):
    _FIGURES.append(dict(case=case, output=key, exempt_share=fig["exempt"], mismatches=fig["mismatches"], max_dist_in_budgets=fig["dist"]))


def L():
    from lightretriever_amd import _lib
    return _lib


def bf(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(torch.bfloat16).contiguous()


def h16(a):
    """fp16 device tensor of fp16-exact values (the host file proves that they are)"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(torch.float16).contiguous()


def f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


class Guarded:
    """a [rows, cols] output in the middle of a sentinel-filled allocation"""

    def __init__(self, rows, cols, dtype, init=None):
        self.n = rows * cols
        self.flat = torch.full((GUARD + self.n + GUARD,), S, dtype=dtype, device="cuda")
        self.t = self.flat[GUARD:GUARD + self.n].view(rows, cols)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.flat[:GUARD] == S).all()) and bool((self.flat[GUARD + self.n:] == S).all())


def fused(A, B, C, bias, resid, M, N, K, epi, rscale=None, ss=None):
    lib = L()
    return lib.lib().lrx_gemm_bf16_nt_fused(lib.ptr(A), lib.ptr(B), lib.ptr(C), lib.ptr(bias), lib.ptr(resid), M, N, K, epi, lib.ptr(rscale), lib.ptr(ss), lib.current_stream())


def resid32_call(A, B, x32, a16, gamma, M, N, K, ss):
    lib = L()
    return lib.lib().lrx_gemm_bf16_nt_resid32(lib.ptr(A), lib.ptr(B), lib.ptr(x32), lib.ptr(a16), lib.ptr(gamma), M, N, K, lib.ptr(ss), lib.current_stream())


def fused_ex(A, B, C, bias, resid, M, N, K, epi, rscale=None, ss=None, f16=0):
    lib = L()
    return lib.lib().lrx_gemm_nt_fused_ex(lib.ptr(A), lib.ptr(B), lib.ptr(C), lib.ptr(bias), lib.ptr(resid), M, N, K, epi, lib.ptr(rscale), lib.ptr(ss), f16,
                                          lib.current_stream())


def resid32_ex_call(A, B, x32, a16, gamma, M, N, K, ss, f16, out_f16):
    lib = L()
    return lib.lib().lrx_gemm_nt_resid32_ex(lib.ptr(A), lib.ptr(B), lib.ptr(x32), lib.ptr(a16), lib.ptr(gamma), M, N, K, lib.ptr(ss), f16, out_f16,
                                            lib.current_stream())


def saturations():
    return int(L().lib().lrx_device_saturation_count(1))


@functools.lru_cache(maxsize=None)
def _ref(name):
    case = CASES[IDS.index(name)] if name in IDS else CASES_F16[IDS_F16.index(name)]
    inp = GR.case_inputs(case)
    return case, inp, GR.case_reference(case, inp)


def run_case(case, inp):
    """one launch of the case into fresh guarded outputs -> ({name: tensor}, [Guarded])"""
    from lightretriever_amd import ops
    M, N, K, epi = case["M"], case["N"], case["K"], case["epi"]
    f16, out_f16 = case.get("f16", 0), case.get("out_f16", 0)
    A, B = (h16 if f16 else bf)(inp["A"]), (h16 if f16 else bf)(inp["B"])
    nt = GR.n_tiles(N)
    if epi == "swiglu" and f16:
        C = Guarded(M, N // 2, torch.float16)
        assert fused_ex(A, B, C.t, None, None, M, N, K, 2, f32(inp["rscale"]), None, 1) == 0
        return {"C": C.t}, [C]
    if epi == "resid32" and (f16 or out_f16):
        x, ss = Guarded(M, N, torch.float32, f32(inp["x32"])), Guarded(nt, M, torch.float32)
        a = None if case.get("no_a16") else Guarded(M, N, torch.float16 if out_f16 else torch.bfloat16)
        assert resid32_ex_call(A, B, x.t, None if a is None else a.t, None if a is None else bf(inp["gamma"]), M, N, K, ss.t, f16, out_f16) == 0
        return dict({"x32": x.t, "ss": ss.t}, **({} if a is None else {"a16": a.t})), [x, ss] + ([] if a is None else [a])
    if epi == "store":
        C = Guarded(M, N, torch.bfloat16)
        assert fused(A, B, C.t, bf(inp["bias"]), None, M, N, K, 0, f32(inp["rscale"])) == 0
        return {"C": C.t}, [C]
    if epi == "resid":
        C, ss = Guarded(M, N, torch.bfloat16, bf(inp["R"])), Guarded(nt, M, torch.float32)
        assert fused(A, B, C.t, None, C.t, M, N, K, 1, None, ss.t) == 0                                # C aliases resid
        return {"C": C.t, "ss": ss.t}, [C, ss]
    if epi == "swiglu":
        C = Guarded(M, N // 2, torch.bfloat16)
        assert fused(A, B, C.t, None, None, M, N, K, 2, f32(inp["rscale"])) == 0
        return {"C": C.t}, [C]
    if epi == "resid32":
        x, a, ss = Guarded(M, N, torch.float32, f32(inp["x32"])), Guarded(M, N, torch.bfloat16), Guarded(nt, M, torch.float32)
        assert resid32_call(A, B, x.t, a.t, bf(inp["gamma"]), M, N, K, ss.t) == 0
        return {"x32": x.t, "a16": a.t, "ss": ss.t}, [x, a, ss]
    if epi == "maxagg":
        nb = len(inp["cu"]) - 1
        out = Guarded(nb, N + 24, torch.float32)
        ops.sparse_max_aggregate(A, B, i32(inp["cu"]), torch.from_numpy(inp["mask"]).cuda(), bf(inp["bias"]), out=out.t)
        assert bool((out.t[:, N:] == S).all()), "columns past the vocabulary were written"
        return {"out": out.t[:, :N]}, [out]
    if epi == "rope":
        C = Guarded(M, N, torch.float16)
        ops.gemm_qkv_rope_slice(A, B, i32(inp["positions"]), f32(inp["cos"]), f32(inp["sin"]), case["nq"], case["nkv"], case["d"], 0,
                                case["nq"] + 2 * case["nkv"], C.t, bias=bf(inp["bias"]), rscale=f32(inp["rscale"]), operands="fp16" if f16 else "bf16")
        return {"C": C.t}, [C]
    raise KeyError(epi)


@pytest.mark.parametrize("name", IDS + IDS_F16)
def test_case(name):
    case, inp, ref = _ref(name)
    counted = case["epi"] == "rope" or name in IDS_F16                # every fp16 store counts what leaves the range: nothing here does
    if counted:
        saturations()
    got, guards = run_case(case, inp)
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), f"{name}: memory outside the logical block of an output changed"
    for key, val in ref.items():
        if key == "ss":
            worst = GR.check_ss(host(got["ss"]), val[0], val[1], f"{name} ss_part")
            _FIGURES.append(dict(case=name, output="ss_part", worst_in_u=worst, bound_in_u=val[1]))
            continue
        _, pre, budget, fmt = val
        fig = GR.check(host(got[key]), pre, budget, fmt, f"{name} {key}")
        print(f"{name} {key}: exempt {fig['exempt']:.5f}, {fig['mismatches']} differ from round(pre), largest distance {fig['dist']:.3f} budgets")
        if case["family"] == "exact":
            assert fig["mismatches"] == 0
        _record(name, key, fig)
    if case["epi"] == "maxagg":                                     # bit patterns, the sign of zero included
        want = ref["out"][0].astype(np.float32)
        np.testing.assert_array_equal(got["out"].cpu().numpy().view(np.uint32), want.view(np.uint32))
        if not case.get("negative"):
            assert (want == 0).any() and (want == np.float32(GR.BF16_MIN)).any() and (want < 0).any()
        else:
            assert (want[want != np.float32(GR.BF16_MIN)] < 0).all()
    if counted:
        assert saturations() == 0
    # a second launch: the same bits (max aggregation: integer atomics of a maximum, order-free as well)
    again, guards2 = run_case(case, inp)
    for key in got:
        assert torch.equal(got[key], again[key]), f"{name} {key}: two runs differ"
    if case["epi"] == "resid":                                      # and the residual read from another buffer than C: what the aliased call gave
        M, N, K = case["M"], case["N"], case["K"]
        C = Guarded(M, N, torch.bfloat16)
        assert fused(bf(inp["A"]), bf(inp["B"]), C.t, None, bf(inp["R"]), M, N, K, 1) == 0
        assert torch.equal(C.t, got["C"]) and C.intact()


# ---------------------------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 7])
def test_k_loop_one_hot_rows_name_the_k_element_read(nk):
    """A[m, pi(m)] = 1: C[m, n] = B[n, pi(m)], bit for bit; and A = I against an asymmetric B at the same K"""
    from lightretriever_amd import ops
    M, N, K = 300, 264, 64 * nk
    A, B = GR.one_hot_rows(M, N, K)
    np.testing.assert_array_equal(host(ops.gemm_bf16_nt(bf(A), bf(B))), B[:, (37 * np.arange(M) + 11) % K].T, err_msg=f"nk={nk}")
    A, B = GR.identity_operands(K, N)
    np.testing.assert_array_equal(host(ops.gemm_bf16_nt(bf(A), bf(B))), B.T, err_msg=f"identity nk={nk}")


def _resid32_f16_from_zero(A, B, M, N, K):
    """x32 = 0 + A . B^T through <EPI_RESID32, true> (fp16 operands, fp16 a16), guarded -> the fp32 x32 as float64"""
    x, a = Guarded(M, N, torch.float32, torch.zeros(M, N, device="cuda")), Guarded(M, N, torch.float16)
    assert resid32_ex_call(h16(A), h16(B), x.t, a.t, None, M, N, K, None, 1, 1) == 0
    torch.cuda.synchronize()
    assert x.intact() and a.intact()
    return host(x.t), host(a.t)


@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 7])
def test_k_loop_one_hot_rows_with_11_bit_values_through_the_f16_mfma(nk):
    """The one-hot probe with values that need all 11 bits of fp16 (1024 .. 2046, odd ones included: bf16 holds none of the odd ones):
    x32[m, n] = B[n, pi(m)] bit for bit names the K element read AND shows that no operand bit was dropped on the way through LDS and the
    f16 MFMA; a16 (gamma = NULL) is the same number, an fp16 number already"""
    M, N, K = 300, 264, 64 * nk
    A, B = GR.one_hot_rows_wide(M, N, K)
    want = B[:, (37 * np.arange(M) + 11) % K].T.astype(np.float64)
    x, a = _resid32_f16_from_zero(A, B, M, N, K)
    np.testing.assert_array_equal(x, want, err_msg=f"nk={nk}")
    np.testing.assert_array_equal(a, want, err_msg=f"a16 nk={nk}")


def test_fp16_subnormal_operands_pass_the_f16_mfma_unchanged():
    """One-hot A against B = j 2^-24, j = 1 .. 1023 (every fp16 subnormal), x32 = 0: IEEE arithmetic gives x32 == B exactly -- 1 x a
    subnormal, added to zeros, is that subnormal, a normal fp32 number.  A matrix core that flushed subnormal f16 inputs would give 0.
    The ISA notes at hand state the MFMA's subnormal behaviour for f32 inputs and for C / D only, so it was measured here.  OUTCOME on gfx950
    (MI355X): v_mfma_f32_16x16x32_f16 KEEPS subnormal inputs -- none of the 4800 outputs is flushed, all equal B bit for bit.
    So the encoder's survival check of the fp16 weight conversion counts subnormal weights as kept, and rightly.  a16 = fp16(x32) is the
    subnormal again (the conversion's subnormal path)."""
    M, N, K = 300, 16, 128
    A, B = GR.subnormal_probe(M, K)
    want = B[:, (37 * np.arange(M) + 11) % K].T.astype(np.float64)
    x, a = _resid32_f16_from_zero(A, B, M, N, K)
    flushed = float((x == 0).mean())
    print(f"fp16-subnormal operands: {flushed:.4f} of the outputs are zero (1.0 = the f16 MFMA flushes subnormal inputs, 0.0 = it keeps them)")
    np.testing.assert_array_equal(x, want)
    np.testing.assert_array_equal(a, want)


@pytest.mark.parametrize("M,N", GR.TILE_MAP)
def test_tile_map_with_coded_probe(M, N):
    """C[m, n] encodes (m, n): a tile computed twice, never, or written to another tile's place shows as the wrong code.  Store epilogue
    (group_m 8) and residual epilogue with a zero residual (group_m 6; bf16(bf16(acc) + 0) = acc)"""
    A, B = GR.coded_operands(M, N)
    want = GR.acc64(A, B)
    Ad, Bd = bf(A), bf(B)
    for epi in (0, 1):
        C = Guarded(M, N, torch.bfloat16)
        if epi == 1:
            C.t.zero_()
        assert fused(Ad, Bd, C.t, None, C.t if epi else None, M, N, GR.GBK, epi) == 0
        got = host(C.t)
        bad = got != want
        if bad.any():
            i = tuple(np.argwhere(bad)[0].tolist())
            raise AssertionError(f"{M}x{N} epilogue {epi}: {int(bad.sum())} wrong elements in tiles {sorted({(int(r) // 256, int(c) // 256) for r, c in np.argwhere(bad)})[:8]}; "
                                 f"first at {list(i)}: {GR.decode_coded(i, got[i])}")
        assert C.intact()


# ---------------------------------------------------------------------------------------------------------------
# head slices, saturation, refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rope-d64-q4kv2-b0r0-257x64", "rope-d128-q2kv1-b1r1-127x192"])
def test_head_slices_write_their_columns_only(name):
    from lightretriever_amd import ops
    case, inp, _ = _ref(name)
    nq, nkv, d, M, N = case["nq"], case["nkv"], case["d"], case["M"], case["N"]
    full, _ = run_case(case, inp)
    args = (bf(inp["A"]), bf(inp["B"]), i32(inp["positions"]), f32(inp["cos"]), f32(inp["sin"]), nq, nkv, d)
    for head0, n_heads in ((nq, 2 * nkv), (0, nq), (nq + nkv - 1, 2)):          # k|v, q, and the last k head with the first v head
        C = Guarded(M, N, torch.float16)
        ops.gemm_qkv_rope_slice(*args, head0, n_heads, C.t, bias=bf(inp["bias"]), rscale=f32(inp["rscale"]))
        lo, hi = head0 * d, (head0 + n_heads) * d
        assert torch.equal(C.t[:, lo:hi], full["C"][:, lo:hi]), (name, head0, n_heads)
        assert bool((C.t[:, :lo] == S).all()) and bool((C.t[:, hi:] == S).all()) and C.intact(), (name, head0, n_heads)


def test_saturation_stores_65504_by_sign_and_nan_as_minus_65504():
    """accumulators beyond fp16's range: +-65504 by sign; a NaN (a zero accumulator times an infinite row scale) is stored as -65504 --
    fmaxf(NaN, -65504) = -65504 in f2h_bits -- and both are counted"""
    from lightretriever_amd import ops
    case, inp, _ = _ref("rope-d64-q4kv2-b0r0-257x64-pos0")
    nq, nkv, d, M, N = case["nq"], case["nkv"], case["d"], case["M"], case["N"]
    A = inp["A"].copy()
    A[7] = 0.0
    rs = np.ones(M, np.float32)
    rs[[3, 200, 256]] = 2.0 ** 16
    want, pre, _ = GR.qkv_rope(A, inp["B"], inp["positions"], inp["cos"], inp["sin"], nq, nkv, d, None, rs)
    assert (np.abs(pre[[3, 200, 256]]) > 65504).mean() > 0.5 and (np.abs(np.delete(pre, [3, 200, 256], 0)) < 65504).all()
    rs[7] = np.inf
    want[7] = -65504.0
    saturations()
    C = Guarded(M, N, torch.float16)
    ops.gemm_qkv_rope_slice(bf(A), bf(inp["B"]), i32(inp["positions"]), f32(inp["cos"]), f32(inp["sin"]), nq, nkv, d, 0, nq + 2 * nkv, C.t, rscale=f32(rs))
    np.testing.assert_array_equal(host(C.t), want)
    assert saturations() > 0 and C.intact()
    assert saturations() == 0                                        # (the read above reset it)


@pytest.mark.parametrize("which", GR.SATURATION)
def test_fp16_operand_stores_saturate_by_sign_and_store_nan_as_minus_65504(which):
    """The SwiGLU store under fp16 operands and the a16 store under out_f16 (both operand formats) on GR.saturation_inputs: +-65504 by sign,
    a NaN as -65504, every other element held to the rule (bit-exact outside its budget), counted, and the counter reads 0 after the reset"""
    case, inp, ref = GR.saturation_inputs(which)
    saturations()
    got, guards = run_case(case, inp)
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards)
    key = "C" if case["epi"] == "swiglu" else "a16"
    _, pre, budget, fmt = ref[key]
    out = host(got[key])
    assert np.isfinite(out).all(), "an inf or a NaN was stored"
    with np.errstate(all="ignore"):
        fig = GR.check(out, pre, budget, fmt, which)
    if case["epi"] == "resid32":
        assert fig["mismatches"] == 0
        np.testing.assert_array_equal(got["x32"].cpu().numpy(), ref["x32"][0].astype(np.float32))       # (NaN and inf kept in the fp32 stream)
    assert saturations() > 0
    assert saturations() == 0                                        # (the read above reset it)


def test_fp16_refusals_leave_the_output_alone():
    """fp16 operands are served for the SwiGLU epilogue only; fp16 operands never write a bf16 operand"""
    A, B = h16(np.ones((8, 128))), h16(np.ones((64, 128)))
    C = Guarded(8, 64, torch.float32)
    refused = [
        fused_ex(A, B, C.t, None, None, 8, 64, 128, 0, None, None, 1),                       # f16 with the store epilogue
        fused_ex(A, B, C.t, None, C.t, 8, 64, 128, 1, None, None, 1),                        # f16 with the residual epilogue
        fused_ex(A, B, C.t, None, None, 8, 40, 128, 2, None, None, 1),                       # f16 SwiGLU with N % 32 != 0
        resid32_ex_call(A, B, C.t, C.t, None, 8, 64, 128, None, 1, 0),                       # f16 && !out_f16 && a16 != NULL
        resid32_ex_call(A, B, C.t, None, None, 8, 64, 96, None, 1, 1),
        resid32_ex_call(A, B, None, None, None, 8, 64, 128, None, 0, 1),                     # no residual stream
    ]
    assert all(rc != 0 for rc in refused), refused
    assert L().lib().lrx_last_error()
    assert fused_ex(A, B, C.t, None, None, 0, 64, 128, 2, None, None, 1) == 0 and resid32_ex_call(A, B, C.t, C.t, None, 0, 64, 128, C.t, 1, 1) == 0
    torch.cuda.synchronize()
    assert bool((C.t == S).all()) and C.intact()
    # f16 && !out_f16 with a16 == NULL is served: x32 alone
    x = Guarded(8, 64, torch.float32, torch.zeros(8, 64, device="cuda"))
    assert resid32_ex_call(A, B, x.t, None, None, 8, 64, 128, None, 1, 0) == 0
    torch.cuda.synchronize()
    assert bool((x.t == 128.0).all()) and x.intact()


def test_refusals_leave_the_output_alone():
    lib = L()
    l = lib.lib()
    A, B = bf(np.ones((8, 128))), bf(np.ones((64, 128)))
    C = Guarded(8, 64, torch.float32)                                # wide enough for every output type below
    one = f32(np.ones(64))
    s = lib.current_stream()
    p = lib.ptr
    pos, tab = i32(np.zeros(8)), f32(np.ones((4, 64)))
    refused = [
        fused(A, B, C.t, None, None, 8, 64, 96, 0),                                          # K % 64 != 0
        fused(A, B, C.t, None, None, 8, 60, 128, 0),                                         # N % 8 != 0
        fused(A, B, C.t, None, None, 8, 40, 128, 2),                                         # SwiGLU with N % 32 != 0
        fused(A, B, C.t, None, None, 8, 64, 128, 1),                                         # residual epilogue without resid
        fused(A, B, C.t, None, None, 8, 64, 128, 0, None, C.t),                              # ss_part with a non-residual epilogue
        fused(A, B, C.t, None, C.t, 8, 64, 128, 1, one),                                     # rscale with the residual epilogue
        resid32_call(A, B, C.t, None, None, 8, 64, 96, None),
        resid32_call(A, B, C.t, None, None, 8, 60, 128, None),
        l.lrx_gemm_qkv_rope_slice(p(A), p(B), p(C.t), None, p(pos), p(tab), p(tab), 8, 128, 1, 1, 96, None, 0, 3, s),     # head_dim 96
        l.lrx_gemm_qkv_rope_slice(p(A), p(B), p(C.t), None, p(pos), p(tab), p(tab), 8, 128, 1, 1, 64, None, 2, 2, s),     # heads [2, 4) of 3
        l.lrx_gemm_qkv_rope_slice(p(A), p(B), p(C.t), None, p(pos), p(tab), p(tab), 8, 128, 1, 1, 64, None, -1, 2, s),
        l.lrx_gemm_qkv_rope_slice(p(A), p(B), p(C.t), None, p(pos), p(tab), p(tab), 8, 128, 1, 1, 64, None, 0, 0, s),
    ]
    assert all(rc != 0 for rc in refused), refused
    assert l.lrx_last_error()
    # M = 0: fine, and nothing is written
    assert fused(A, B, C.t, None, None, 0, 64, 128, 0) == 0 and fused(A, B, C.t, None, C.t, 0, 64, 128, 1) == 0
    assert fused(A, B, C.t, None, None, 0, 64, 128, 2) == 0 and resid32_call(A, B, C.t, C.t, None, 0, 64, 128, C.t) == 0
    assert l.lrx_gemm_qkv_rope_slice(p(A), p(B), p(C.t), None, p(pos), p(tab), p(tab), 0, 128, 1, 1, 64, None, 0, 3, s) == 0
    torch.cuda.synchronize()
    assert bool((C.t == S).all()) and C.intact()
