"""The attention kernels (lightretriever_amd/csrc/lrx_attn.hip) against the float64 reference of tests/attn_reference.py, at the shapes of
tests/test_gpu_attn_work_list.py and under the bound derived there, plus probes whose answer needs no floating-point judgement.

  parity      every CASES entry of test_gpu_attn_work_list.py (list launch; the bitwise test there ties the walking launch to it), then a
              subset under three more input regimes, then the two suffix-over-prefix kernels on both sides of their dispatch limits
  first row   row 0 of a sequence sees one key: its output is v_0 of its kv head, bit for bit
  constant    v = c per (sequence, kv head): every output is c to one bf16 rounding; a neighbour's or another head's c is far away
  one-hot     v = unit vectors over a window of d keys: the output columns ARE the probabilities; exactly 0 behind the causal mask
  extremes    +-65504 in every k / v row a compared row must not see: neighbours, its own future tokens, the rows past the buffer's end

Worst |got - O| / bound per case group (bound: 2^-8 |O| + c 2^-11 A + 1e-6 with c = 2, see attn_reference.py), `restated` = the CPU
restatement of the kernels' arithmetic on inputs of the same regime (tests/test_attn_reference_host.py, L = 33 .. 2000):

                                        flat    peaky   offset  large scores
  kernel    resident d64                0.852   0.875   0.807   0.873
  kernel    tiled d64                   0.827   0.872   0.814   0.885
  kernel    tiled d128                  0.859   0.885   0.822   0.888
  kernel    tiled d64 last tile         0.846   -       -       -
  kernel    tiled d128 last tile        0.856   0.867   0.806   0.879
  restated  d = 64                      0.810   0.817   0.791   0.843      (q x 8: 0.848, q x 4 with v + 30: 0.831)
  restated  d = 128                     0.797   0.839   0.751   0.851      (q x 8: 0.862, q x 4 with v + 30: 0.854)

                                        parity  one-hot window  masked extremes
  kernel    prefix/suffix matrix-core   0.814   0.844           0.790
  kernel    prefix/suffix VALU          0.836   0.820           0.797
  kernel    resident d64                        0.866           0.822
  kernel    tiled d64                           0.876           0.822
  kernel    tiled d128                          0.865           0.867

The same with fp16 OUTPUT (out_f16: all five kernels; bound 2^-11 |O| + c 2^-11 A + 1e-6, c = 2 -- only the output term changes, so the
kernels' internal error is resolved eight times finer than above):

                                        flat    large scores
  kernel    resident d64                0.558   0.641
  kernel    tiled d64                   0.579   0.646
  kernel    tiled d128                  0.594   0.644
  kernel    tiled d128 last tile        0.574   0.638
  restated  d = 64                      0.393   0.616              (peaky 0.573, offset 0.346, q x 8: 0.608, q x 4 with v + 30: 0.560)
  restated  d = 128                     0.469   0.622              (peaky 0.572, offset 0.277, q x 8: 0.582, q x 4 with v + 30: 0.544)

                                        parity  masked extremes
  kernel    prefix/suffix matrix-core   0.430   0.423
  kernel    prefix/suffix VALU          0.421   0.407
  kernel    resident d64                        0.562
  kernel    tiled d64                           0.581
  kernel    tiled d128                          0.574

  fp16 out    the parity cases above also run the bf16-output launch: it must hold bf16(fp16 output) -- either neighbour where that is a bf16
              midpoint -- so the two launches differ in the last conversion only; first row = v_0 to all 11 bits; constant v = c to one fp16
              step; masked rows hold +-65504 (the fp16 store does not saturate: see test_fp16_output_masked_rows_hold_extremes)

c = 2 as derived, never adjusted: the kernels' worst ratio (0.888) sits 0.03 above the restatement's (0.862) over some hundred times as many
elements, and both stay under the 0.9 that one worst-case bf16 rounding plus one worst-case fp16 rounding of a dominant probability reach
((2^-8 + 2^-11) / (2^-8 + 2 2^-11)).

Run with -v: the last test of the module prints the table's kernel lines."""
import pytest
import torch

import attn_reference as R
from test_gpu_attn_work_list import CASES, _inputs, _no_overflow
from test_gpu_kernels import PREFIX_SUFFIX_CASES

pytestmark = pytest.mark.gpu

_WORST = {}


def _note(group, ratio):
    _WORST[group] = max(_WORST.get(group, 0.0), ratio) if ratio == ratio else float("nan")


def _check(group, got, O, A, norm=True, fmt="bf16"):
    ratio = R.worst_ratio(got, O, A, fmt=fmt)
    _note(group, ratio)
    print(f"{group}: worst |err| / bound = {ratio:.3f}" + (f", norm ratio - 1 = {R.norm_ratio(got, O) - 1:+.2e}" if norm else ""))
    assert ratio <= 1.0, f"{group}: worst |err| / bound = {ratio:.3f}"
    if norm:
        assert abs(R.norm_ratio(got, O) - 1) < 3e-3


def _cu(lens):
    return torch.tensor([0] + list(lens), dtype=torch.int64).cumsum(0).to(torch.int32).cuda()


def _path(d, lens, last):
    """which device path the documented dispatch sends a launch to"""
    if d == 64 and max(lens) <= 512 and not last:
        return "resident d64"
    return f"tiled d{d}" + (" last tile" if last else "")


# ---- input regimes: flat is the work-list tests' own input (unscaled randn)
def _regime(qkv, nq, nkv, d, regime):
    x = qkv.float()
    if regime == "peaky":
        x[:, :nq * d] *= 4
    elif regime == "offset":               # a normalisation error becomes a scale error of every element
        x[:, (nq + nkv) * d:] += 30
    elif regime == "large_scores":         # |s| / sqrt(d) of a few hundred: the masked maximum and a rescale by alpha ~ 0 in every tile
        x[:, :(nq + nkv) * d] *= 8
    else:
        assert regime == "flat"
    return x.to(torch.float16)


def _run_case(name, nq, nkv, d, lens, last, regime):
    from lightretriever_amd import ops
    qkv, cu = _inputs(nq, nkv, d, lens)
    qkv = _regime(qkv, nq, nkv, d, regime)
    got = ops.attn_varlen_causal(qkv, cu, max(lens), nq, nkv, d, last_tile_only=last)
    _no_overflow()
    O, A = R.causal_gqa_fp64(qkv, cu, nq, nkv, d)
    if last:      # only the q tile holding each sequence's last token is computed, the rest stays zero (test_attention_last_tile_only_and_gather)
        ln = torch.tensor(lens, device="cuda")
        start = torch.repeat_interleave(cu[:-1].long(), ln)
        keep = torch.arange(sum(lens), device="cuda") - start >= torch.repeat_interleave(((ln - 1) // 64) * 64, ln)
        assert (got[~keep] == 0).all()
        got, O, A = got[keep], O[keep], A[keep]
    _check(f"{_path(d, lens, last)}, {regime}", got, O, A)


@pytest.mark.parametrize("name,nq,nkv,d,lens,last", CASES, ids=[c[0] for c in CASES])
def test_work_list_cases_against_fp64(name, nq, nkv, d, lens, last):
    _run_case(name, nq, nkv, d, lens, last, "flat")


# which case stands for what in the three other regimes
REGIME_CASES = {
    "d64_resident_ignores_the_list": "the K/V-resident kernel (d = 64, S <= 512)",
    "d64_g4_long": "the tiled kernel at d = 64",
    "d128_g2_long": "the tiled kernel at d = 128",
    "d128_g6_two_parts": "a GQA group split into two parts (d = 128, 3 + 3 heads)",
    "d64_g16_two_parts": "... and at d = 64 (8 + 8 heads)",
    "8b_ragged_grouped": "the XCD-grouped lists (more items than workgroup slots)",
    "one_long_sequence": "one sequence of 8192 tokens, 128 q tiles",
    "8b_last_tile": "last-tile mode",
    "tiny": "sequences shorter than a tile",
}
_BY_NAME = {c[0]: c for c in CASES}


@pytest.mark.parametrize("regime", ["peaky", "offset", "large_scores"])
@pytest.mark.parametrize("name", list(REGIME_CASES))
def test_work_list_cases_under_other_input_regimes(name, regime):
    _run_case(*_BY_NAME[name], regime)


# ---- suffix over shared prefix
def _prefix_path(d, nq, nkv, P1, S2):
    """the dispatch rule in lrx_attn_prefix_suffix_ex's comments: matrix cores for 1 <= P1 <= 64, S2 <= 4 and grp S2 <= 16 (d = 64) / 12 (d = 128) waves"""
    return "prefix/suffix matrix-core" if 1 <= P1 <= 64 and S2 <= 4 and (nq // nkv) * S2 <= (16 if d == 64 else 12) else "prefix/suffix VALU"


PREFIX_EDGE_CASES = [
    (64, 8, 2, 64, 2, 40), (64, 8, 2, 65, 2, 40), (128, 4, 2, 64, 2, 35), (128, 4, 2, 65, 2, 35),          # P1 = 64 | 65
    (64, 16, 2, 30, 2, 34), (64, 8, 2, 30, 4, 34), (64, 12, 2, 30, 3, 34), (64, 16, 2, 30, 3, 34),         # d = 64: 8x2 = 4x4 = 16 waves | 6x3 = 18, 8x3 = 24
    (128, 12, 2, 30, 2, 34), (128, 4, 1, 30, 3, 34), (128, 14, 2, 30, 2, 34), (128, 5, 1, 30, 3, 34),      # d = 128: 6x2 = 4x3 = 12 waves | 7x2 = 14, 5x3 = 15
    (64, 8, 2, 30, 2, 32), (64, 8, 2, 30, 2, 33), (64, 8, 2, 30, 2, 1), (128, 8, 2, 50, 2, 32), (128, 8, 2, 50, 2, 33), (128, 8, 2, 50, 2, 1),  # 32-sequence blocks
    (64, 8, 2, 64, 5, 7),                                                                                  # S2 = 5: past the matrix-core kernel's 4 own keys
]


def _prefix_inputs(d, nq, nkv, P1, S2, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = (nq + 2 * nkv) * d
    suf = torch.randn(n * S2, W, generator=g, device="cuda")
    suf[:, :nq * d] *= 2.0
    pre = torch.randn(P1, 2 * nkv * d, generator=g, device="cuda")
    return suf.to(torch.float16), pre.to(torch.float16)


@pytest.mark.parametrize("d,nq,nkv,P1,S2,n", PREFIX_SUFFIX_CASES + PREFIX_EDGE_CASES)
def test_prefix_suffix_against_fp64(d, nq, nkv, P1, S2, n):
    from lightretriever_amd import ops
    suf, pre = _prefix_inputs(d, nq, nkv, P1, S2, n, d + nq + P1 + n)
    got = ops.attn_prefix_suffix(suf, pre, n, S2, nq, nkv, d)
    _check(_prefix_path(d, nq, nkv, P1, S2), got, *R.prefix_suffix_fp64(suf, pre, n, S2, nq, nkv, d))


def test_prefix_edge_cases_sit_on_both_sides_of_the_dispatch_limits():
    paths = [_prefix_path(*c[:5]) for c in PREFIX_EDGE_CASES]
    mc, va = "prefix/suffix matrix-core", "prefix/suffix VALU"
    assert paths == [mc, va, mc, va, mc, mc, va, va, mc, mc, va, va, mc, mc, mc, mc, mc, mc, va]


# ---- structural probes.  Lengths straddle 32, 64 and 512 | 513 and leave non-multiple tails; every sequence but the outer two has neighbours
PROBE_LAYOUTS = [
    ("resident_d64", 8, 2, 64, [100, 33, 64, 1, 512, 65, 31, 32, 511, 97]),
    ("tiled_d64", 8, 2, 64, [100, 33, 513, 64, 1, 900, 65, 200, 31, 577, 32]),
    ("tiled_d64_two_parts", 16, 1, 64, [65, 513, 32, 130, 1, 33]),            # group 16: parts of 8 + 8 heads
    ("tiled_d128", 8, 2, 128, [100, 33, 64, 1, 512, 513, 900, 65, 31, 32, 97]),
    ("tiled_d128_two_parts", 12, 2, 128, [65, 513, 32, 130, 1, 96, 33]),      # group 6: parts of 3 + 3 heads
    ("tiled_d128_parts_4_3", 7, 1, 128, [65, 130, 32, 1, 200]),               # group 7: parts of 4 + 3 heads, one idle wave pair
]
_probe = pytest.mark.parametrize("name,nq,nkv,d,lens", PROBE_LAYOUTS, ids=[p[0] for p in PROBE_LAYOUTS])
# (d, nq, nkv, P1, S2, n): both kernels at both head dims; the last one has no prefix at all
PREFIX_PROBE_LAYOUTS = [(64, 8, 2, 40, 4, 37), (128, 6, 2, 33, 2, 33), (64, 8, 2, 70, 6, 9), (128, 4, 2, 65, 3, 5), (64, 4, 2, 0, 3, 6)]
_prefix_probe = pytest.mark.parametrize("d,nq,nkv,P1,S2,n", PREFIX_PROBE_LAYOUTS)


def _randn16(rows, cols, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(rows, cols, generator=g, device="cuda") * scale).to(torch.float16)


def _attn(qkv, lens, nq, nkv, d):
    from lightretriever_amd import ops
    out = ops.attn_varlen_causal(qkv, _cu(lens), max(lens), nq, nkv, d)
    _no_overflow()
    return out


def _of_kv_head(per_kv, nq, nkv):
    """[..., nkv, d] -> [..., nq d]: what each q head should see of its kv head"""
    grp = nq // nkv
    return per_kv.unsqueeze(-2).expand(*per_kv.shape[:-1], grp, per_kv.shape[-1]).reshape(*per_kv.shape[:-2], nq * per_kv.shape[-1])


@_probe
def test_first_row_is_its_own_value_row(name, nq, nkv, d, lens):
    """One visible key: p = 1, l = 1 to an fp32 rounding, O = v_0.  v is bf16-exact here: 1 / l may be 1 - 2^-24, which cannot move an
    8-bit value across a bf16 rounding boundary but can break an fp16 value's tie."""
    qkv = _randn16(sum(lens), (nq + 2 * nkv) * d, 31)
    qkv[:, (nq + nkv) * d:] = qkv[:, (nq + nkv) * d:].to(torch.bfloat16).to(torch.float16)
    got = _attn(qkv, lens, nq, nkv, d)
    first = _cu(lens)[:-1].long()
    want = _of_kv_head(qkv[first, (nq + nkv) * d:].view(len(lens), nkv, d), nq, nkv).to(torch.bfloat16)
    assert torch.equal(got[first], want)


def _constants(n, device="cuda"):
    """n distinct bf16-exact values +-m 2^e, m in 1, 3, 5, 7 and e from -6 up: neighbours in the list differ in sign and by factors.  (Made
    on the host: a device pow() need not return 2^e exactly.)"""
    i = torch.arange(n)
    return ((1 - 2 * (i % 2)).double() * (1 + 2 * (i % 4)).double() * 2.0 ** (-6 + (i // 4) * 2).double()).to(device)


@_probe
def test_constant_value_per_sequence_and_kv_head(name, nq, nkv, d, lens):
    qkv = _randn16(sum(lens), (nq + 2 * nkv) * d, 32, scale=1.5)
    c = _constants(len(lens) * nkv).view(len(lens), nkv)
    assert c.abs().max() < 6e4 and torch.equal(c.to(torch.bfloat16).double(), c) and c.unique().numel() == c.numel()
    seq = torch.repeat_interleave(torch.arange(len(lens), device="cuda"), torch.tensor(lens, device="cuda"))
    qkv[:, (nq + nkv) * d:] = c[seq][:, :, None].expand(-1, -1, d).reshape(sum(lens), nkv * d).to(torch.float16)
    got = _attn(qkv, lens, nq, nkv, d).double()
    want = _of_kv_head(c[seq][:, :, None].expand(-1, -1, d), nq, nkv)
    assert ((got - want).abs() <= 2.0 ** -8 * want.abs()).all(), ((got - want).abs() / want.abs()).max()     # within the smaller neighbouring bf16 step


def _window_start(placement, n, d):
    """windows of d keys across the boundaries the kernels have: sequence start (with the 32-key sub-tile, the 64-key tile and the 64-row q
    tile inside: 16 .. 16 + d), the sequence end (half the window lies past it), 512 (the resident kernel's last key | the tiled one's ninth tile)"""
    return {"start": 0, "sub_tile_and_tile": min(16, n - 1), "end": max(0, n - d // 2), "k512": max(0, min(512, n) - d // 2)}[placement]


@pytest.mark.parametrize("placement", ["start", "sub_tile_and_tile", "end", "k512"])
@_probe
def test_one_hot_window_reads_out_the_probabilities(name, nq, nkv, d, lens, placement):
    T, vcol = sum(lens), (nq + nkv) * d
    qkv = _randn16(T, (nq + 2 * nkv) * d, 33, scale=1.5)
    qkv[:, vcol:] = 0
    visible = torch.zeros(T, d, dtype=torch.bool, device="cuda")       # [row i, column t]: key w + t exists and is <= i
    s0 = 0
    for n in lens:
        w = _window_start(placement, n, d)
        t = torch.arange(min(d, n - w), device="cuda")
        for hk in range(nkv):
            qkv[s0 + w + t, vcol + hk * d + t] = 1.0
        visible[s0:s0 + n] = (w + torch.arange(d, device="cuda"))[None, :] <= torch.arange(n, device="cuda")[:, None]
        visible[s0:s0 + n, min(d, n - w):] = False
        s0 += n
    got = _attn(qkv, lens, nq, nkv, d)
    hidden = ~visible[:, None, :].expand(T, nq, d).reshape(T, nq * d)
    assert (got[hidden] == 0).all(), f"{int((got[hidden] != 0).sum())} probabilities behind the causal mask or outside the sequence are not 0.0"
    P, A = R.causal_gqa_fp64(qkv, _cu(lens), nq, nkv, d)              # O = A = P for unit-vector values
    assert torch.equal(P, A) and (P[hidden] == 0).all()
    _check(f"one-hot window, {_path(d, lens, False)}", got, P, A, norm=False)


def _extremes(rows, cols, device="cuda"):
    """+-65504, the sign alternating along both axes (finite: the QKV epilogue saturates there and never emits inf or nan)"""
    sign = 1 - 2 * ((torch.arange(rows, device=device)[:, None] + torch.arange(cols, device=device)[None, :]) % 2)
    return (sign * 65504.0).to(torch.float16)


@_probe
def test_masked_rows_hold_extremes(name, nq, nkv, d, lens):
    """Every sequence of the layout sits between two filler sequences whose k and v are +-65504, and its own last rows (inside the tile of the
    rows before them) are filled too; the last sequence ends the buffer uncut, with a partial tile behind it.  The reference sees none of it:
    it runs on the rows that remain."""
    W, kcol = (nq + 2 * nkv) * d, nq * d
    all_lens, keep_rows, ref_lens = [], [], []
    s0 = 0
    for i, n in enumerate(lens):
        all_lens.append(40)                                         # filler
        s0 += 40
        cut = n if i == len(lens) - 1 or n < 4 else n - min(n // 2, 21)   # own future tokens: the rows from `cut` on
        all_lens.append(n)
        keep_rows.append(torch.arange(s0, s0 + cut, device="cuda"))
        ref_lens.append(cut)
        s0 += n
    T = sum(all_lens)
    keep = torch.cat(keep_rows)
    qkv = _randn16(T, W, 34, scale=1.5)
    filled = torch.ones(T, dtype=torch.bool, device="cuda")
    filled[keep] = False
    qkv[filled, kcol:] = _extremes(T, W - kcol)[filled]
    got = _attn(qkv, all_lens, nq, nkv, d)
    assert torch.isfinite(got.float()).all()
    O, A = R.causal_gqa_fp64(qkv[keep].contiguous(), _cu(ref_lens), nq, nkv, d)
    assert A.max() < 20
    _check(f"masked extremes, {_path(d, all_lens, False)}", got[keep], O, A)


# ---- the same probes on the suffix-over-prefix kernels
def _prefix_attn(suf, pre, n, S2, nq, nkv, d):
    from lightretriever_amd import ops
    return ops.attn_prefix_suffix(suf, pre, n, S2, nq, nkv, d)


def test_prefix_suffix_first_row_without_a_prefix():
    d, nq, nkv, P1, S2, n = PREFIX_PROBE_LAYOUTS[-1]
    assert P1 == 0
    suf, pre = _prefix_inputs(d, nq, nkv, P1, S2, n, 41)
    suf[:, (nq + nkv) * d:] = suf[:, (nq + nkv) * d:].to(torch.bfloat16).to(torch.float16)
    got = _prefix_attn(suf, pre, n, S2, nq, nkv, d)
    want = _of_kv_head(suf[::S2, (nq + nkv) * d:].view(n, nkv, d), nq, nkv).to(torch.bfloat16)
    assert torch.equal(got[::S2], want)


@_prefix_probe
def test_prefix_suffix_constant_value_per_kv_head(d, nq, nkv, P1, S2, n):
    """(the prefix is shared by every sequence, so the constant is per kv head; reads of a neighbouring sequence: the extremes probe below)"""
    suf, pre = _prefix_inputs(d, nq, nkv, P1, S2, n, 42)
    c = _constants(4 * nkv)[3::4]                                     # 7 2^e: far apart
    suf[:, (nq + nkv) * d:] = c[:, None].expand(nkv, d).reshape(1, nkv * d).to(torch.float16)
    pre[:, nkv * d:] = c[:, None].expand(nkv, d).reshape(1, nkv * d).to(torch.float16)
    got = _prefix_attn(suf, pre, n, S2, nq, nkv, d).double()
    want = _of_kv_head(c[:, None].expand(nkv, d), nq, nkv)[None, :]
    assert ((got - want).abs() <= 2.0 ** -8 * want.abs()).all(), ((got - want).abs() / want.abs()).max()


@_prefix_probe
def test_prefix_suffix_one_hot_window_over_the_seam(d, nq, nkv, P1, S2, n):
    """the last d keys of [prefix | suffix]: the window covers every own key and the prefix keys next to the seam"""
    suf, pre = _prefix_inputs(d, nq, nkv, P1, S2, n, 43)
    L = P1 + S2
    w = max(0, L - d)
    suf[:, (nq + nkv) * d:] = 0
    pre[:, nkv * d:] = 0
    for hk in range(nkv):
        t = torch.arange(w, P1, device="cuda")
        pre[t, nkv * d + hk * d + t - w] = 1.0
        for j in range(S2):
            suf[j::S2, (nq + nkv) * d + hk * d + P1 + j - w] = 1.0
    got = _prefix_attn(suf, pre, n, S2, nq, nkv, d)
    # column t of suffix row j is key w + t: visible iff w + t <= P1 + j
    vis = (w + torch.arange(d, device="cuda"))[None, :] <= (P1 + torch.arange(S2, device="cuda"))[:, None]
    hidden = ~vis[None, :, None, :].expand(n, S2, nq, d).reshape(n * S2, nq * d)
    assert (got[hidden] == 0).all()
    P, A = R.prefix_suffix_fp64(suf, pre, n, S2, nq, nkv, d)
    assert torch.equal(P, A) and (P[hidden] == 0).all()
    _check(f"one-hot window, {_prefix_path(d, nq, nkv, P1, S2)}", got, P, A, norm=False)


@_prefix_probe
def test_prefix_suffix_masked_rows_hold_extremes(d, nq, nkv, P1, S2, n):
    """odd sequences are fillers (k, v = +-65504), the even ones lose their last suffix token to the fill: rows before it must not notice"""
    suf, pre = _prefix_inputs(d, nq, nkv, P1, S2, n, 44)
    cut = S2 - 1
    row = torch.arange(n * S2, device="cuda")
    keep = ((row // S2) % 2 == 0) & (row % S2 < cut)
    kcol = nq * d
    suf[~keep, kcol:] = _extremes(n * S2, suf.shape[1] - kcol)[~keep]
    got = _prefix_attn(suf, pre, n, S2, nq, nkv, d)
    assert torch.isfinite(got.float()).all()
    O, A = R.prefix_suffix_fp64(suf[keep].contiguous(), pre, (n + 1) // 2, cut, nq, nkv, d)
    assert A.max() < 20
    _check(f"masked extremes, {_prefix_path(d, nq, nkv, P1, S2)}", got[keep], O, A)


# ---- fp16 output (out_f16: the O-projection's operand under precise_stream = 2), all five kernels.  Bound: 2^-11 |O| + c 2^-11 A + 1e-6.
def _two_roundings(what, got16, got_bf):
    """the bf16-output launch of the same inputs holds bf16(fp16 output) wherever that is normal; either neighbour where the fp16 value is a
    bf16 midpoint: the two launches differ in the last conversion only"""
    lo, hi, checked = R.bf16_of_fp16_allowed(got16)
    b = got_bf.double()
    bad = checked & (b != lo) & (b != hi)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} elements of the bf16-output launch are not the bf16 rounding of the fp16-output launch's"
    assert checked.float().mean() > 0.9


F16_PARITY = ["d64_resident_ignores_the_list", "d64_g4_long", "d128_g2_long", "d128_g6_two_parts", "8b_last_tile", "tiny"]


@pytest.mark.parametrize("regime", ["flat", "large_scores"])
@pytest.mark.parametrize("name", F16_PARITY)
def test_fp16_output_against_fp64_and_against_the_bf16_launch(name, regime):
    from lightretriever_amd import ops
    _, nq, nkv, d, lens, last = _BY_NAME[name]
    qkv, cu = _inputs(nq, nkv, d, lens)
    qkv = _regime(qkv, nq, nkv, d, regime)
    got = ops.attn_varlen_causal(qkv, cu, max(lens), nq, nkv, d, last_tile_only=last, out_dtype=torch.float16)
    got_bf = ops.attn_varlen_causal(qkv, cu, max(lens), nq, nkv, d, last_tile_only=last)
    _no_overflow()
    assert got.dtype == torch.float16
    # the launch without a list (the kernel walks its items itself: another instantiation of the same store) writes the same bits
    assert torch.equal(got, ops.attn_varlen_causal(qkv, cu, max(lens), nq, nkv, d, last_tile_only=last, work_list=False, out_dtype=torch.float16))
    O, A = R.causal_gqa_fp64(qkv, cu, nq, nkv, d)
    if last:
        ln = torch.tensor(lens, device="cuda")
        start = torch.repeat_interleave(cu[:-1].long(), ln)
        keep = torch.arange(sum(lens), device="cuda") - start >= torch.repeat_interleave(((ln - 1) // 64) * 64, ln)
        assert (got[~keep] == 0).all()
        got, got_bf, O, A = got[keep], got_bf[keep], O[keep], A[keep]
    _check(f"{_path(d, lens, last)}, {regime}, fp16 out", got, O, A, fmt="fp16")
    _two_roundings(f"{name} {regime}", got, got_bf)


@pytest.mark.parametrize("d,nq,nkv,P1,S2,n", PREFIX_EDGE_CASES)
def test_prefix_suffix_fp16_output_against_fp64_and_against_the_bf16_launch(d, nq, nkv, P1, S2, n):
    from lightretriever_amd import ops
    suf, pre = _prefix_inputs(d, nq, nkv, P1, S2, n, d + nq + P1 + n)
    got = ops.attn_prefix_suffix(suf, pre, n, S2, nq, nkv, d, out_dtype=torch.float16)
    assert got.dtype == torch.float16
    _check(_prefix_path(d, nq, nkv, P1, S2) + ", fp16 out", got, *R.prefix_suffix_fp64(suf, pre, n, S2, nq, nkv, d), fmt="fp16")
    _two_roundings(f"prefix {(d, nq, nkv, P1, S2, n)}", got, ops.attn_prefix_suffix(suf, pre, n, S2, nq, nkv, d))


def _attn16(qkv, lens, nq, nkv, d):
    from lightretriever_amd import ops
    out = ops.attn_varlen_causal(qkv, _cu(lens), max(lens), nq, nkv, d, out_dtype=torch.float16)
    _no_overflow()
    return out


@_probe
def test_fp16_output_first_row_is_its_own_value_row_to_all_11_bits(name, nq, nkv, d, lens):
    """One visible key: p = 1, l = 1 to an fp32 rounding, O = v_0.  v is ANY fp16 number here: v (1 - 2^-24) is no fp16 midpoint, so the
    fp16 rounding returns v itself -- all 11 bits, where the bf16-output probe needs bf16-exact values and sees 8."""
    qkv = _randn16(sum(lens), (nq + 2 * nkv) * d, 31)
    got = _attn16(qkv, lens, nq, nkv, d)
    first = _cu(lens)[:-1].long()
    want = _of_kv_head(qkv[first, (nq + nkv) * d:].view(len(lens), nkv, d), nq, nkv)
    assert (want.to(torch.bfloat16).to(torch.float16) != want).float().mean() > 0.5      # (most values need more than bf16's bits)
    assert torch.equal(got[first], want)


def test_prefix_suffix_fp16_output_first_row_without_a_prefix():
    d, nq, nkv, P1, S2, n = PREFIX_PROBE_LAYOUTS[-1]
    suf, pre = _prefix_inputs(d, nq, nkv, P1, S2, n, 41)
    from lightretriever_amd import ops
    got = ops.attn_prefix_suffix(suf, pre, n, S2, nq, nkv, d, out_dtype=torch.float16)
    assert torch.equal(got[::S2], _of_kv_head(suf[::S2, (nq + nkv) * d:].view(n, nkv, d), nq, nkv))


def _within_one_fp16_step(got, want):
    """got is `want` or one of its two fp16 neighbours: fp16 numbers of one sign are consecutive as bit patterns.  -> (all?, share != want)"""
    g, w = got.to(torch.float16).view(torch.int16).int(), want.to(torch.float16).view(torch.int16).int()
    assert (want.to(torch.float16).double() == want).all() and (want != 0).all()
    return bool(((g - w).abs() <= 1).all()), float((g != w).double().mean())


@_probe
def test_fp16_output_constant_value_per_sequence_and_kv_head(name, nq, nkv, d, lens):
    """v = c: O = c exactly, A = |c|.  Before the output rounding the kernel holds c (sum fp16(p_i)) / (sum p_i): within 2^-11 |c| of c (each
    probability is rounded once, the weights are a convex combination) plus fp32 terms a thousand times smaller -- less than one and a half
    fp16 steps at c, so the one fp16 rounding that follows lands on c or on an fp16 NEIGHBOUR of c, never farther.  (The bf16-output probe
    can require c itself: there the internal error is an eighth of the output step.)  A neighbouring sequence's or head's c is a factor away."""
    qkv = _randn16(sum(lens), (nq + 2 * nkv) * d, 32, scale=1.5)
    c = _constants(len(lens) * nkv).view(len(lens), nkv)
    assert c.abs().max() < 6e4 and torch.equal(c.to(torch.float16).double(), c) and c.unique().numel() == c.numel()
    seq = torch.repeat_interleave(torch.arange(len(lens), device="cuda"), torch.tensor(lens, device="cuda"))
    qkv[:, (nq + nkv) * d:] = c[seq][:, :, None].expand(-1, -1, d).reshape(sum(lens), nkv * d).to(torch.float16)
    got = _attn16(qkv, lens, nq, nkv, d).double()
    want = _of_kv_head(c[seq][:, :, None].expand(-1, -1, d), nq, nkv).contiguous()
    ok, moved = _within_one_fp16_step(got, want)
    print(f"{name}: {moved:.4f} of the outputs are a neighbour of c")
    assert ok, ((got - want).abs() / want.abs()).max()
    first = _cu(lens)[:-1].long()
    assert torch.equal(got[first], want[first])                       # one key: nothing is rounded, c itself


def _masked_extremes_fp16(name, nq, nkv, d, lens, top):
    W, kcol = (nq + 2 * nkv) * d, nq * d
    all_lens, keep_rows, ref_lens = [], [], []
    s0 = 0
    for i, n in enumerate(lens):
        all_lens.append(40)
        s0 += 40
        cut = n if i == len(lens) - 1 or n < 4 else n - min(n // 2, 21)
        all_lens.append(n)
        keep_rows.append(torch.arange(s0, s0 + cut, device="cuda"))
        ref_lens.append(cut)
        s0 += n
    T = sum(all_lens)
    keep = torch.cat(keep_rows)
    qkv = _randn16(T, W, 34, scale=1.5)
    filled = torch.ones(T, dtype=torch.bool, device="cuda")
    filled[keep] = False
    qkv[filled, kcol:] = (_extremes(T, W - kcol)[filled].float() * (top / 65504.0)).to(torch.float16)
    assert float(qkv[filled, kcol:].float().abs().min()) == top
    got = _attn16(qkv, all_lens, nq, nkv, d)
    return got, keep, all_lens, qkv, ref_lens


@_probe
def test_fp16_output_masked_rows_hold_extremes(name, nq, nkv, d, lens):
    """test_masked_rows_hold_extremes with the fp16 store: +-65504 in every k / v row a compared row must not see.
    Finiteness is required of the COMPARED rows only.  The fp16 store does not saturate, and |o| <= max |v| holds up to the rounding of
    the probabilities: the kernel forms (sum fp16(p_i) v_i) / (sum p_i), and a dominant p_i (up to 2^8 under the lazy maximum) may be
    rounded UP by 2^-11 of itself, so a filler row whose visible values are +-65504 -- fp16's largest number -- can reach 65504 (1 + 2^-11) >
    65520 and is stored as inf.  Measured: the filler rows of every layout hold some.  One fp16 step below (the test after this one)
    nothing can overflow.  In the encoder v = +-65504 exists only after the QKV store saturated, which lrx_device_saturation_count reports."""
    got, keep, all_lens, qkv, ref_lens = _masked_extremes_fp16(name, nq, nkv, d, lens, 65504.0)
    assert torch.isfinite(got[keep].float()).all()
    print(f"{name}: {int((~torch.isfinite(got.float())).sum())} non-finite outputs in the filler rows (v = +-65504)")
    O, A = R.causal_gqa_fp64(qkv[keep].contiguous(), _cu(ref_lens), nq, nkv, d)
    assert A.max() < 20
    _check(f"masked extremes, {_path(d, all_lens, False)}, fp16 out", got[keep], O, A, fmt="fp16")


@pytest.mark.parametrize("name,nq,nkv,d,lens", [PROBE_LAYOUTS[0], PROBE_LAYOUTS[3]], ids=[PROBE_LAYOUTS[0][0], PROBE_LAYOUTS[3][0]])
def test_fp16_output_is_finite_for_every_value_below_fp16s_largest(name, nq, nkv, d, lens):
    """|v| <= 65472, the second largest fp16 number: 65472 (1 + 2^-11) (1 + a few 2^-24) < 65520, the smallest value that rounds to inf --
    every output of every row, fillers included, is finite: the unsaturating store needs no clamp below fp16's largest number"""
    got, keep, all_lens, qkv, ref_lens = _masked_extremes_fp16(name, nq, nkv, d, lens, 65472.0)
    assert torch.isfinite(got.float()).all() and float(got.float().abs().max()) >= 65472.0


@_prefix_probe
def test_prefix_suffix_fp16_output_masked_rows_hold_extremes(d, nq, nkv, P1, S2, n):
    from lightretriever_amd import ops
    suf, pre = _prefix_inputs(d, nq, nkv, P1, S2, n, 44)
    cut = S2 - 1
    row = torch.arange(n * S2, device="cuda")
    keep = ((row // S2) % 2 == 0) & (row % S2 < cut)
    kcol = nq * d
    suf[~keep, kcol:] = _extremes(n * S2, suf.shape[1] - kcol)[~keep]
    got = ops.attn_prefix_suffix(suf, pre, n, S2, nq, nkv, d, out_dtype=torch.float16)
    assert torch.isfinite(got[keep].float()).all()                   # (the filler rows: see test_fp16_output_masked_rows_hold_extremes)
    O, A = R.prefix_suffix_fp64(suf[keep].contiguous(), pre, (n + 1) // 2, cut, nq, nkv, d)
    assert A.max() < 20
    _check(f"masked extremes, {_prefix_path(d, nq, nkv, P1, S2)}, fp16 out", got[keep], O, A, fmt="fp16")


def test_zz_worst_ratio_per_case_group(request, capsys):
    """The last test of the module: with -v it prints what the tests before it measured, one line per case group."""
    if request.config.getoption("verbose") > 0:
        with capsys.disabled():
            print()
            for group in sorted(_WORST):
                print(f"attention worst |err| / bound (c = {R.C_BOUND:g})  {group:44s} {_WORST[group]:.3f}")
    assert all(r <= 1.0 for r in _WORST.values())
