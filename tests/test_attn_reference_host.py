"""Host checks of tests/attn_reference.py: the float64 reference against the numpy loop the kernel tests have used so far, and the CPU
restatement of the kernels' arithmetic against the error bound it calibrates (its worst ratio is printed; run with -s to see it)."""
import functools

import numpy as np
import pytest
import torch

import attn_reference as R
from test_gpu_kernels import PREFIX_SUFFIX_CASES, VARLEN_CASES, attn_oracle, rnd


def _f16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.float16)


@pytest.mark.parametrize("d,nq,nkv,lens", VARLEN_CASES)
def test_fp64_reference_agrees_with_the_numpy_oracle(d, nq, nkv, lens):
    rng = np.random.default_rng(sum(lens) + d)
    qkv = rnd(rng, sum(lens), (nq + 2 * nkv) * d)
    qkv[:, :nq * d] *= 2.0
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = _f16(qkv)
    O, A = R.causal_gqa_fp64(x, cu, nq, nkv, d)
    np.testing.assert_allclose(O.numpy(), attn_oracle(x.float().numpy(), cu, nq, nkv, d), atol=1e-5, rtol=0)
    assert (A >= O.abs() - 1e-12).all()


@pytest.mark.parametrize("d,nq,nkv,P1,S2,n", PREFIX_SUFFIX_CASES)
def test_prefix_suffix_reference_is_the_suffix_rows_of_full_causal(d, nq, nkv, P1, S2, n):
    g = torch.Generator().manual_seed(d + nq + P1 + n)
    W = (nq + 2 * nkv) * d
    pre = torch.randn(P1, W, generator=g).to(torch.float16)
    suf = torch.randn(n * S2, W, generator=g).to(torch.float16)
    O, A = R.prefix_suffix_fp64(suf, pre[:, nq * d:].contiguous(), n, S2, nq, nkv, d)
    L = P1 + S2
    full = torch.cat([torch.cat([pre, suf[i * S2:(i + 1) * S2]]) for i in range(n)])
    Of, Af = R.causal_gqa_fp64(full, [i * L for i in range(n + 1)], nq, nkv, d)
    pick = lambda t: t.view(n, L, nq * d)[:, P1:].reshape(n * S2, nq * d)
    assert (O - pick(Of)).abs().max() < 1e-12 and (A - pick(Af)).abs().max() < 1e-12


def test_chunked_reference_equals_the_unchunked_one(monkeypatch):
    g = torch.Generator().manual_seed(3)
    nq, nkv, d, lens = 4, 2, 64, [70, 5, 70, 33, 5]
    qkv = torch.randn(sum(lens), (nq + 2 * nkv) * d, generator=g).to(torch.float16)
    cu = np.concatenate([[0], np.cumsum(lens)])
    O, A = R.causal_gqa_fp64(qkv, cu, nq, nkv, d)
    monkeypatch.setattr(R, "_BUDGET", 4 * 70 * 9)          # 9 query rows per chunk, one sequence at a time
    O2, A2 = R.causal_gqa_fp64(qkv, cu, nq, nkv, d)
    assert (O - O2).abs().max() < 1e-13 and (A - A2).abs().max() < 1e-13


# the regimes of tests/test_gpu_attn_reference.py at sizes a CPU does in seconds: (q scale, k scale, v offset)
REGIMES = {"flat": (1.0, 1.0, 0.0), "peaky": (4.0, 1.0, 0.0), "peaky8": (8.0, 1.0, 0.0), "offset": (1.0, 1.0, 30.0), "peaky_offset": (4.0, 1.0, 30.0),
           "large_scores": (8.0, 8.0, 0.0)}


@functools.lru_cache(maxsize=None)
def _restatement_case(d, regime):
    qs, ks, voff = REGIMES[regime]
    nq, nkv, lens = 2, 1, [129, 700, 2000, 33]
    g = torch.Generator().manual_seed(d + len(regime))
    x = torch.randn(sum(lens), (nq + 2 * nkv) * d, generator=g)
    x[:, :nq * d] *= qs
    x[:, nq * d:(nq + nkv) * d] *= ks
    x[:, (nq + nkv) * d:] += voff
    x = x.to(torch.float16)
    cu = np.concatenate([[0], np.cumsum(lens)])
    return (x, cu, nq, nkv) + R.causal_gqa_fp64(x, cu, nq, nkv, d)


def _restatement_inside_the_bound(d, regime, fmt):
    x, cu, nq, nkv, O, A = _restatement_case(d, regime)
    got = R.restated(x, cu, nq, nkv, d, fmt=fmt)
    assert got.dtype == {"bf16": torch.bfloat16, "fp16": torch.float16}[fmt]
    ratio = R.worst_ratio(got, O, A, fmt=fmt)
    print(f"restated d={d} {regime} {fmt} output: worst |err| / bound = {ratio:.3f}, norm ratio - 1 = {R.norm_ratio(got, O) - 1:+.2e}")
    assert ratio <= 1.0
    assert abs(R.norm_ratio(got, O) - 1) < 3e-3


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("d", [64, 128])
def test_restatement_stays_inside_the_bound(d, regime):
    _restatement_inside_the_bound(d, regime, "bf16")


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("d", [64, 128])
def test_restatement_with_fp16_output_stays_inside_the_fp16_bound(d, regime):
    """the output term of the bound is 2^-11 |O| instead of 2^-8 |O|, c = 2 unchanged (attn_reference.py)"""
    _restatement_inside_the_bound(d, regime, "fp16")


def test_two_roundings_of_one_number():
    """bf16(v) = bf16(fp16(v)) unless fp16(v) is a bf16 midpoint, where either neighbour is allowed: on fp32 values, exhaustively enough"""
    g = torch.Generator().manual_seed(5)
    v = (torch.randn(1 << 20, generator=g) * 10.0 ** torch.randint(-3, 4, (1 << 20,), generator=g)).float()
    v = torch.cat([v, torch.tensor([1.00390625, 1.0039062, 1.0039063, -3.0234375, 2.0 ** -15, 1.0, 0.0])])
    lo, hi, checked = R.bf16_of_fp16_allowed(v.to(torch.float16))
    b = v.to(torch.bfloat16).double()
    assert (((b == lo) | (b == hi)) | ~checked).all() and checked.float().mean() > 0.99
    assert (lo.float().to(torch.bfloat16).double() == lo).all() and (hi.float().to(torch.bfloat16).double() == hi).all()     # bf16 numbers both
    tie = lo != hi
    assert 5e-2 < tie.float().mean() < 0.2 and (hi[tie].abs() > lo[tie].abs()).all()          # one fp16 number in eight is a bf16 midpoint
    away = ~tie
    assert (lo[away] == v.to(torch.float16).to(torch.bfloat16).double()[away]).all()           # elsewhere: the RNE rounding of the fp16 number
    assert (lo[-2] == 1.0) and (hi[-2] == 1.0) and lo[-7] == 1.0 and hi[-7] == 1.0078125       # 1.00390625 = 1 + 2^-8: the midpoint of 1 and 1 + 2^-7
    assert lo[-4] == -3.015625 and hi[-4] == -3.03125                                          # a negative midpoint: towards zero | away from it
    # a launch that rounded another value is caught: bf16 of a value about one fp16 ulp away leaves [lo, hi] on a measurable share
    off =(v.to(torch.float16).float() * (1 + 2.0 ** -10)).to(torch.bfloat16).double()
    assert ((off != lo) & (off != hi) & checked).float().mean() > 0.05
