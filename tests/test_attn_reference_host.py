"""Host checks of tests/attn_reference.py: the float64 reference against the numpy loop the kernel tests have used so far, and the CPU
restatement of the kernels' arithmetic against the error bound it calibrates (its worst ratio is printed; run with -s to see it)."""
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


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("d", [64, 128])
def test_restatement_stays_inside_the_bound(d, regime):
    qs, ks, voff = REGIMES[regime]
    nq, nkv, lens = 2, 1, [129, 700, 2000, 33]
    g = torch.Generator().manual_seed(d + len(regime))
    x = torch.randn(sum(lens), (nq + 2 * nkv) * d, generator=g)
    x[:, :nq * d] *= qs
    x[:, nq * d:(nq + nkv) * d] *= ks
    x[:, (nq + nkv) * d:] += voff
    x = x.to(torch.float16)
    cu = np.concatenate([[0], np.cumsum(lens)])
    O, A = R.causal_gqa_fp64(x, cu, nq, nkv, d)
    got = R.restated(x, cu, nq, nkv, d)
    ratio = R.worst_ratio(got, O, A)
    print(f"restated d={d} {regime}: worst |err| / bound = {ratio:.3f}, norm ratio - 1 = {R.norm_ratio(got, O) - 1:+.2e}")
    assert ratio <= 1.0
    assert abs(R.norm_ratio(got, O) - 1) < 3e-3
