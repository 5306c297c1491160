"""The issue order of k_gemm_bf16_nt's MFMA clusters (lrx_gemm.hip, G_PHASE), pinned with operands that name the accumulator a product landed in.

A reordered cluster can go wrong in two ways only: a fragment is paired with the wrong accumulator, or a ks step of a K-tile is dropped or
issued twice.  The operands make both visible exactly:

  A[m, k] = alpha(m) w(k)          alpha(m) = 1 + (m / 16) % 16: one value per 16-row group (h, wave row, mi) of a 256-row tile
  w(k)    = (1 + k / 64) (1 | 2)   the K-tile's factor, times 1 in the first 32 elements of the K-tile (ks 0) and 2 in the second 32 (ks 1)
  B[n, k] = beta(n) 2^-s           beta(n) = the ((n / 16) % 16)-th prime from 17: one value per 16-column group (hp, wave column, ni)

All of them are integers of at most 8 bits times a power of two (bf16- and fp16-exact), every partial sum is an integer below 2^24 units, so
the fp32 accumulator is alpha beta S 2^-s exactly, S = 96 nk (nk + 1) / 2.  A prime above 16 divides no alpha: the 256 products alpha beta of a
tile are all different, and an accumulator fed from another row group, another column group, or with a ks half missing or doubled holds
another number.  test_operands_name_every_slot_and_both_ks_halves proves all of that on the host, per entry, on what the entry STORES (a bf16
or fp16 rounding, or the SwiGLU of two accumulators): no such mistake leaves a stored value where it was.

The entries are those tests/gemm_reference.py drives, compared under its rule with a zero budget (bit for bit) wherever the epilogue is exact:
store (the entry refuses fp16 operands: bf16 only), SwiGLU, the fp32 residual (x32 shows the accumulator itself; a16 and ss_part as well) and
the QKV projection with RoPE at position 0 (the identity), each with bf16 and fp16 operands.  Shapes: one full 256 x 256 tile and the ragged
300 x 264 (SwiGLU takes N % 32 == 0: 288; the QKV projection whole heads of 64: 320), at K = 64 (the prologue alone), 128 (both ring
buffers, the last-tile branches) and 256 (steady state)."""
import functools

import numpy as np
import pytest

import gemm_reference as GR
from oracle import lrx_oracle as O

PRIMES = np.array([17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79], np.float64)
ALPHAS = np.arange(1, 17, dtype=np.float64)
B_SCALE = 2.0 ** -6                      # the linear entries: accumulators of 25.5 .. 18960, inside fp16
GATE_SCALE, UP_SCALE = 2.0 ** -14, 2.0 ** -11     # SwiGLU: gate 0.1 .. 74, up 0.8 .. 593, silu(g) u below 43 900
KS = (64, 128, 256)
ROPE_HEADS = {256: (2, 1), 320: (3, 1)}  # N -> (nq, nkv) at d = 64
SHAPES = {"store": ((256, 256), (300, 264)), "resid32": ((256, 256), (300, 264)), "swiglu": ((256, 256), (300, 288)), "rope": ((256, 256), (300, 320))}
FORMATS = {"store": ("bf16",), "resid32": ("bf16", "fp16"), "swiglu": ("bf16", "fp16"), "rope": ("bf16", "fp16")}
CASES = [(e, f, M, N, K) for e in SHAPES for f in FORMATS[e] for M, N in SHAPES[e] for K in KS]
IDS = [f"{e}-{f}-{M}x{N}x{K}" for e, f, M, N, K in CASES]


def k_weights(K):
    k = np.arange(K)
    return (1 + k // GR.GBK) * np.where(k % GR.GBK < 32, 1.0, 2.0)


def half_sums(K):
    """what each (K-tile, ks) step adds to an accumulator, in units of alpha beta"""
    return k_weights(K).reshape(-1, 32).sum(1)


def column_scale(entry, N):
    if entry != "swiglu":
        return np.full(N, B_SCALE)
    return np.where(np.arange(N) % 32 < 16, GATE_SCALE, UP_SCALE)        # interleaved weight: 16 gate rows, 16 up rows, ...


@functools.lru_cache(maxsize=None)
def operands(entry, M, N, K):
    A = (ALPHAS[(np.arange(M) // 16) % 16][:, None] * k_weights(K)[None, :]).astype(np.float32)
    B = np.repeat((PRIMES[(np.arange(N) // 16) % 16] * column_scale(entry, N))[:, None], K, 1).astype(np.float32)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def accumulator(entry, M, N, K):
    """the integer reference: alpha(m) beta(n) S, scaled"""
    S = half_sums(K).sum()
    return ALPHAS[(np.arange(M) // 16) % 16][:, None] * (PRIMES[(np.arange(N) // 16) % 16] * column_scale(entry, N))[None, :] * S


def silu_mul(g, u):
    return g / (1.0 + np.exp(-g)) * u


def stored(entry, fmt, acc, gate=None):
    """what the entry stores for accumulator values `acc` (SwiGLU: `gate` is the gate accumulator, `acc` the up one), rounding included"""
    if entry == "store":
        return GR.bf16_round(acc)
    if entry == "resid32":
        return np.asarray(acc, np.float64).astype(np.float32).astype(np.float64)
    if entry == "rope":
        return GR.fp16_round(acc)
    return (GR.fp16_sat if fmt == "fp16" else GR.bf16_round)(silu_mul(gate, acc))


@functools.lru_cache(maxsize=None)
def reference(entry, fmt, M, N, K):
    A, B = operands(entry, M, N, K)
    if entry == "store":
        return {"C": GR.store(A, B) + ("bf16",)}
    if entry == "swiglu":
        return {"C": GR.swiglu(A, B, None, fmt) + (fmt,)}
    if entry == "resid32":
        x, a, px, pa, b, ss = GR.resid32(A, B, np.zeros((M, N), np.float32), np.ones(N, np.float32), fmt)
        return {"x32": (x, px, b, "fp32"), "a16": (a, pa, b, fmt), "ss": (ss, GR.SS_ROUNDINGS_RESID32)}
    nq, nkv = ROPE_HEADS[N]
    cos, sin = GR.rope_table(64, GR.N_POS)
    return {"C": GR.qkv_rope(A, B, np.zeros(M, np.int32), cos, sin, nq, nkv, 64) + ("fp16",)}


# ---------------------------------------------------------------------------------------------------------------
# host: the operands do what the module docstring says
# ---------------------------------------------------------------------------------------------------------------
def wrong_accumulators(a, b, K):
    """[n_mistakes, 16, 16]: what the accumulator of slot (alpha a, beta b) would hold, in units of the scale, after each mistake a reordered
    cluster can make: the A fragment of another row group, the B fragment of another column group, a (K-tile, ks) step dropped, issued
    twice, or replaced by another step"""
    hs = half_sums(K)
    S = hs.sum()
    out = []
    for d in range(1, 16):
        out.append(np.roll(a, d, 0) * b * S)                         # a[mi'] / the other h
        out.append(a * np.roll(b, d, 1) * S)                         # b[ni'] / b2 for b
    for i, h in enumerate(hs):
        out.append(a * b * (S - h))
        out.append(a * b * (S + h))
        out += [a * b * (S - h + h2) for j, h2 in enumerate(hs) if h2 != h]
    return np.stack(out)


def test_operands_name_every_slot_and_both_ks_halves():
    a, b = ALPHAS[:, None] * np.ones((1, 16)), np.ones((16, 1)) * PRIMES[None, :]
    assert len(np.unique(a * b)) == 256                              # one number per (row group, column group) of a tile
    for entry, fmt, M, N, K in CASES:
        what = f"{entry}-{fmt}-{M}x{N}x{K}"
        A, B = operands(entry, M, N, K)
        # bf16- and fp16-exact operands, nothing subnormal in either format
        assert (O.round_bf16(A) == A).all() and (O.round_bf16(B) == B).all() and GR.is_fp16_exact(A) and GR.is_fp16_exact(B), what
        assert not GR.has_fp16_subnormals(A) and not GR.has_fp16_subnormals(B), what
        # every partial sum is an integer below 2^24 units: the fp32 accumulator is exact, in any order
        units, _ = GR.sum_units(A, B)
        assert units < 2 ** 24, (what, units)
        acc = accumulator(entry, M, N, K)
        np.testing.assert_array_equal(GR.acc64(A, B), acc, err_msg=what)
        assert (acc.astype(np.float32).astype(np.float64) == acc).all(), what
        # the two ks halves of every K-tile weigh differently
        hs = half_sums(K).reshape(-1, 2)
        assert (hs[:, 1] == 2 * hs[:, 0]).all() and (hs[:, 0] == 32 * (1 + np.arange(K // GR.GBK))).all(), what
        # within a tile every slot holds another number, and a 16 x 16 block one number
        t = acc[:min(M, 256), :min(N, 256)]
        blocks = [t[i:i + 16, j:j + 16] for i in range(0, t.shape[0], 16) for j in range(0, t.shape[1], 16)]
        assert all((blk == blk.flat[0]).all() for blk in blocks), what
        if entry != "swiglu":
            assert len({float(blk.flat[0]) for blk in blocks}) == len(blocks), what
        # no mistake leaves a STORED value where it was
        wrong = wrong_accumulators(a, b, K)
        S = half_sums(K).sum()
        if entry != "swiglu":
            good = stored(entry, fmt, a * b * S * B_SCALE)
            assert np.isfinite(good).all() and (np.abs(good) < 65504).all(), what
            assert (stored(entry, fmt, wrong * B_SCALE) != good[None]).all(), what
            continue
        # SwiGLU: output column group j takes gate = column group 2 j and up = column group 2 j + 1 of the interleaved weight; a mistake hits
        # one of the two accumulators.  The stored value must leave everything the reference's rule would accept for the right one.
        ref = reference(entry, fmt, M, N, K)["C"]
        _, lo, hi, _ = GR.allowed(ref[1], ref[2], fmt)
        GR.exempt_share(ref[1], ref[2], fmt, what)
        assert np.isfinite(hi).all() and (hi < 65504).all() and (lo > 0).all(), what
        g, u = a[:, 0::2] * b[:, 0::2] * S * GATE_SCALE, a[:, 1::2] * b[:, 1::2] * S * UP_SCALE
        lo_s, hi_s = lo[:256:16, :128:16][:16, :8], hi[:256:16, :128:16][:16, :8]
        rows = lo_s.shape[0]
        np.testing.assert_array_equal(stored(entry, fmt, u, g)[:rows], ref[0][:256:16, :128:16][:16, :8], err_msg=what)
        for wg, wu in ((wrong[:, :, 0::2] * GATE_SCALE, u[None]), (g[None], wrong[:, :, 1::2] * UP_SCALE)):
            s = stored(entry, fmt, np.broadcast_to(wu, wrong[:, :, 0::2].shape), np.broadcast_to(wg, wrong[:, :, 0::2].shape))[:, :rows]
            assert ((s < lo_s[None]) | (s > hi_s[None])).all(), what


# ---------------------------------------------------------------------------------------------------------------
# GPU: every entry stores exactly that
# ---------------------------------------------------------------------------------------------------------------
def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(dtype).contiguous()          # (a copy: the cached operands are read-only)


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def launch(entry, fmt, M, N, K):
    """one launch of the entry -> {output name: device tensor}"""
    import torch
    from lightretriever_amd import _lib as lib, ops
    A, B = operands(entry, M, N, K)
    f16 = int(fmt == "fp16")
    op = torch.float16 if f16 else torch.bfloat16
    A, B = _dev(A, op), _dev(B, op)
    stream = lib.current_stream()
    if entry == "store":
        C = torch.full((M, N), GR.SENTINEL, dtype=torch.bfloat16, device="cuda")
        assert lib.lib().lrx_gemm_bf16_nt_fused(lib.ptr(A), lib.ptr(B), lib.ptr(C), None, None, M, N, K, 0, None, None, stream) == 0
        return {"C": C}
    if entry == "swiglu":
        C = torch.full((M, N // 2), GR.SENTINEL, dtype=op, device="cuda")
        if f16:
            assert lib.lib().lrx_gemm_nt_fused_ex(lib.ptr(A), lib.ptr(B), lib.ptr(C), None, None, M, N, K, 2, None, None, 1, stream) == 0
        else:
            assert lib.lib().lrx_gemm_bf16_nt_fused(lib.ptr(A), lib.ptr(B), lib.ptr(C), None, None, M, N, K, 2, None, None, stream) == 0
        return {"C": C}
    if entry == "resid32":
        x = torch.zeros((M, N), dtype=torch.float32, device="cuda")
        a = torch.full((M, N), GR.SENTINEL, dtype=op, device="cuda")
        ss = torch.full((GR.n_tiles(N), M), GR.SENTINEL, dtype=torch.float32, device="cuda")
        gamma = torch.ones(N, dtype=torch.bfloat16, device="cuda")
        if f16:
            assert lib.lib().lrx_gemm_nt_resid32_ex(lib.ptr(A), lib.ptr(B), lib.ptr(x), lib.ptr(a), lib.ptr(gamma), M, N, K, lib.ptr(ss), 1, 1, stream) == 0
        else:
            assert lib.lib().lrx_gemm_bf16_nt_resid32(lib.ptr(A), lib.ptr(B), lib.ptr(x), lib.ptr(a), lib.ptr(gamma), M, N, K, lib.ptr(ss), stream) == 0
        return {"x32": x, "a16": a, "ss": ss}
    nq, nkv = ROPE_HEADS[N]
    cos, sin = GR.rope_table(64, GR.N_POS)
    C = torch.full((M, N), GR.SENTINEL, dtype=torch.float16, device="cuda")
    ops.gemm_qkv_rope_slice(A, B, torch.zeros(M, dtype=torch.int32, device="cuda"), torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda(),
                            nq, nkv, 64, 0, nq + 2 * nkv, C, operands=fmt)
    return {"C": C}


@pytest.mark.gpu
@pytest.mark.parametrize("entry,fmt,M,N,K", CASES, ids=IDS)
def test_entry_stores_the_integer_reference(entry, fmt, M, N, K):
    import torch
    what = f"{entry}-{fmt}-{M}x{N}x{K}"
    ref = reference(entry, fmt, M, N, K)
    got = launch(entry, fmt, M, N, K)
    torch.cuda.synchronize()
    acc = accumulator(entry, M, N, K)
    if entry != "swiglu":                                            # bit for bit: the integer reference under the output's one rounding
        key = "x32" if entry == "resid32" else "C"
        np.testing.assert_array_equal(host(got[key]), stored(entry, fmt, acc), err_msg=f"{what} {key}")
    for key, val in ref.items():
        if key == "ss":
            worst = GR.check_ss(host(got["ss"]), val[0], val[1], f"{what} ss_part")
            print(f"{what} ss_part: worst {worst:.2f} u of {val[1]} u")
            continue
        _, pre, budget, f = val
        fig = GR.check(host(got[key]), pre, budget, f, f"{what} {key}")
        print(f"{what} {key}: exempt {fig['exempt']:.5f}, {fig['mismatches']} differ from round(pre)")
        if entry != "swiglu":
            assert fig["exempt"] == 0 and fig["mismatches"] == 0
