"""The reference of the norm, pooling and row-statistic kernels (lightretriever_amd/csrc/lrx_elementwise.hip), written once: each operation
restated in numpy float64, the error budget an fp32 kernel may spend before a bf16 rounding, the comparison rule built on it, and the inputs
the GPU tests run -- generated here so that the host test that proves the rule's precondition sees the same arrays.  Plain numpy; nothing
from lightretriever_amd and no torch.

Comparison rule for bf16 results.  A kernel computes the value it rounds in fp32; the reference computes it in fp64 ("pre-rounding value").
Where the fp64 value lies farther from a bf16 rounding boundary (the midpoint of two neighbouring bf16 numbers) than the kernel's fp32 error
budget, both must round the same way: the element is required BIT-EQUAL.  Only an element inside the budget of a boundary may be either
neighbour.  HF's LlamaRMSNorm rounds twice, y = bf16(w * bf16(x * rstd)): the inner site carries the budget; the outer product of two bf16
numbers has at most 16 significant bits, so it is EXACT in fp32 and its rounding (RNE, ties included) is required of every element -- an
element whose inner value is near a boundary may be bf16(w * either inner neighbour), nothing else.

The budget (relative, u = 2^-24 the unit roundoff of fp32), derived and not tuned:
  sum of squares   each product f * f is rounded once (u); a lane adds its ceil(H / 64) products serially and the 64 lanes combine in a
                   6-level tree: every term passes through at most ceil(H / 64) + 6 additions.  All terms are non-negative, so the relative
                   error of the sum is at most (ceil(H / 64) + 7) u.  (k_pool_norm and k_rmsnorm_f32 split a row over 256 threads or add
                   four products per step: fewer additions per term, the same bound holds.)
  mean + eps       1 / H rounded (u) and multiplied (u), or one division (u); the addition of eps (u): 3 u.
  rsqrtf           halves the relative error of its argument and adds its own, R_RSQRT.
  => rstd_budget(H) = (ceil(H / 64) + 10) u / 2 + R_RSQRT,   plus u for each fp32 multiplication on the way to the rounded value.
R_RSQRT: no HIP math documentation is installed next to the compiler this project builds with (nothing under the ROCm tree states an ulp
bound of rsqrtf), so it is TWICE the largest relative error measured against 1 / sqrt in fp64: finalize_rscale with one partial, H = 1 and
eps = 0 is rsqrtf alone (tests/test_gpu_elementwise_reference.py::test_rsqrtf_alone measures it, requires it to stay within R_RSQRT_MEASURED
and writes the figure out on request)."""
import numpy as np

U32 = 2.0 ** -24
R_RSQRT_MEASURED = 2.0 ** -23          # what test_rsqrtf_alone may measure at most: 1 ulp at the low end of a binade (the ISA manual's figure for v_rsq_f32)
R_RSQRT = 2.0 * R_RSQRT_MEASURED
NEAR_CAP = 0.02                        # at most this share of a case's elements may be classed near-boundary (a condition, proven on the host)
POOLINGS = ("lasttoken", "cls", "mean", "second_to_last", "third_to_last")


# ---------------------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------------------
def bf16_round(v):
    """float64 -> the nearest bf16 number (RNE, 8 significant bits), as float64.  (Normal range only: no test goes near bf16's subnormals.)"""
    m, e = np.frexp(np.asarray(v, np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def bf16_neighbours(v):
    """(lo, hi, rel): the bf16 numbers below and above v (equal where v is one) and the distance of v from their midpoint, relative to |v|
    (inf where v is a bf16 number or zero: no boundary in reach)."""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(v)
    s = m * 256.0
    lo, hi = np.floor(s), np.ceil(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(lo == hi, np.inf, np.abs(s - lo - 0.5) / np.abs(s))
    return np.ldexp(lo, e - 8), np.ldexp(hi, e - 8), rel


def fp16_round(v):
    """float64 -> fp16 (RNE, saturating at +-65504 like the kernels' clamp), as float64.  numpy's float64 -> float16 cast rounds once."""
    return np.clip(np.asarray(v, np.float64), -65504.0, 65504.0).astype(np.float16).astype(np.float64)


def fp16_sat(v):
    """float64 -> fp16 under the STORE RULE of the kernels that write an fp16 GEMM operand (f2h_bits in lrx_gemm.hip, the clamp of
    k_embed_stream32<true>: fminf(fmaxf(v, -65504), 65504), then one RNE rounding): beyond the range +-65504 by sign, and a NaN -65504 --
    fmaxf(NaN, -65504) is -65504.  Never an inf, never a NaN.  Equal to fp16_round on every number."""
    v = np.asarray(v, np.float64)
    return fp16_round(np.where(np.isnan(v), -65504.0, v))


def fp16_ieee(v):
    """float64 -> fp16 as a plain conversion gives it (RNE; inf beyond 65520, NaN kept): what a store WITHOUT the clamp would write -- the
    wrong kernel the saturation inputs must tell from fp16_sat"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def rstd_budget(H):
    return (-(-H // 64) + 10) * U32 / 2 + R_RSQRT


def sum_budget(n_terms_per_thread, tree_levels):
    """relative error of a sum of non-negative fp32 products: one rounding each, then n serial additions and a tree"""
    return (n_terms_per_thread + tree_levels + 1) * U32


# ---------------------------------------------------------------------------------------------------------------
# the operations, in float64
# ---------------------------------------------------------------------------------------------------------------
def _rstd(x, eps, H=None):
    x = np.asarray(x, np.float64)
    return 1.0 / np.sqrt((x * x).sum(-1, keepdims=True) / (H or x.shape[-1]) + float(eps))


def rmsnorm_bf16(x, w, eps):
    """HF order.  -> (y, inner, outer): y = bf16(w * bf16(x * rstd)); inner = x * rstd and outer = w * bf16(inner) before their roundings."""
    inner = np.asarray(x, np.float64) * _rstd(x, eps)
    outer = np.asarray(w, np.float64) * bf16_round(inner)
    return bf16_round(outer), inner, outer


def rmsnorm_f32(x, w, eps):
    """One rounding.  -> (y, pre): y = bf16(pre), pre = w * x * rstd."""
    pre = np.asarray(w, np.float64) * np.asarray(x, np.float64) * _rstd(x, eps)
    return bf16_round(pre), pre


def row_rscale(x, eps):
    return _rstd(x, eps)[..., 0]


def finalize_rscale(ss_part, H, eps):
    return 1.0 / np.sqrt(np.asarray(ss_part, np.float64).sum(0) / H + float(eps))


def embed_stream32(table, ids, gamma, eps, f16=False):
    """-> (x32, a16, rs): the embedding rows (zeros for an id outside the table), the first projection's operand bf16(x * gamma) (fp16,
    saturating, with f16) and rs = rsqrt(mean(x^2) + eps).  x * gamma is a product of two bf16 numbers: exact before its rounding."""
    table, ids = np.asarray(table, np.float64), np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < table.shape[0])
    x = np.where(ok[:, None], table[np.where(ok, ids, 0)], 0.0)
    pre = x * np.asarray(gamma, np.float64)
    return x, (fp16_sat(pre) if f16 else bf16_round(pre)), row_rscale(x, eps)


def pooled_tokens(cu, pooling):
    """per sequence: the token rows its strategy pools, or None for an impossible sequence (empty, or shorter than the strategy needs)"""
    cu = [int(c) for c in cu]
    out = []
    for s0, s1 in zip(cu[:-1], cu[1:]):
        n = s1 - s0
        need = {"lasttoken": 1, "cls": 1, "mean": 1, "second_to_last": 2, "third_to_last": 3}[pooling]
        if n < need:
            out.append(None)
        elif pooling == "mean":
            out.append(list(range(s0, s1)))
        else:
            out.append([s0 if pooling == "cls" else s1 - need])
    return out


def l2_normalize(p, eps=1e-12):
    p = np.asarray(p, np.float64)
    return p / np.maximum(np.sqrt((p * p).sum(-1, keepdims=True)), eps)


def shard_bounds(rows):
    """{max ||row||, max ||row - fp16(row)||} over the rows, and their fp16 shadow"""
    rows = np.asarray(rows, np.float64)
    sh = fp16_round(rows)
    return np.sqrt((rows * rows).sum(-1)).max(), np.sqrt(((rows - sh) ** 2).sum(-1)).max(), sh


def pool_norm(hidden, w, cu, eps, pooling, out_dim, normalize, f32):
    """-> (out, info).  out [B, out_dim]: the pooled, final-normed (over all H columns), sliced and optionally L2-normalised rows; a zero row
    for an impossible sequence.  f32: the fp32-stream form (no rounding inside), else HF's two bf16 roundings per token.
    info: 'tokens' (pooled_tokens), 'unnorm' (the rows before the L2 normalisation), 'normed' / 'inner' (every token's final-norm row [T, H] and,
    for the bf16 form, its inner pre-rounding value), 'shadow', 'bounds' (the shard form's fp16 shadow and {max |row|, max |row - fp16(row)|})."""
    hidden = np.asarray(hidden, np.float64)
    if f32:
        normed, inner = np.asarray(w, np.float64) * hidden * _rstd(hidden, eps), None
    else:
        normed, inner, _ = rmsnorm_bf16(hidden, w, eps)
    toks = pooled_tokens(cu, pooling)
    un = np.zeros((len(toks), out_dim))
    for b, t in enumerate(toks):
        if t is not None:
            un[b] = normed[t, :out_dim].sum(0) / len(t)
    out = l2_normalize(un) if normalize else un
    r, e, sh = shard_bounds(out)
    return out, {"tokens": toks, "unnorm": un, "normed": normed, "inner": inner, "shadow": sh, "bounds": (r, e)}


def gather_last_rows(src, cu):
    """dst[b] = src[cu[b + 1] - 1]; a zero row for an empty sequence"""
    src, cu = np.asarray(src), [int(c) for c in cu]
    dst = np.zeros((len(cu) - 1,) + src.shape[1:], src.dtype)
    for b in range(len(cu) - 1):
        if cu[b + 1] > cu[b]:
            dst[b] = src[cu[b + 1] - 1]
    return dst, [cu[b + 1] <= cu[b] for b in range(len(cu) - 1)]


def scatter_last_rows(src, cu, dst):
    """a copy of dst with dst[cu[b + 1] - 1, :width] = src[b]; nothing written for an empty sequence"""
    src, cu, dst = np.asarray(src), [int(c) for c in cu], np.array(dst, copy=True)
    for b in range(len(cu) - 1):
        if cu[b + 1] > cu[b]:
            dst[cu[b + 1] - 1, :src.shape[1]] = src[b]
    return dst, [cu[b + 1] <= cu[b] for b in range(len(cu) - 1)]


# ---------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------
def hf_candidates(inner, w, budget):
    """The results HF's rounding order allows a kernel whose inner value is within `budget` (relative) of the fp64 one:
    -> (want, alt, near).  want = bf16(w * bf16(inner)); alt = bf16(w * the other bf16 neighbour of inner) where inner lies within the budget
    of a rounding boundary (near), else want."""
    lo, hi, rel = bf16_neighbours(inner)
    near = rel <= budget
    r = bf16_round(inner)
    other = np.where(r == lo, hi, lo)
    w = np.asarray(w, np.float64)
    want = bf16_round(w * r)
    return want, np.where(near, bf16_round(w * other), want), near


def one_rounding_candidates(pre, budget):
    """-> (want, alt, near) for y = bf16(pre) with pre known to `budget`"""
    lo, hi, rel = bf16_neighbours(pre)
    near = rel <= budget
    want = bf16_round(pre)
    return want, np.where(near, np.where(want == lo, hi, lo), want), near


def assert_bf16_rule(got, want, alt, near, what=""):
    """bit-equality with `want` wherever the element is not near a boundary (alt == want there), one of the two candidates elsewhere; and the
    precondition: at most NEAR_CAP of the elements may claim the second candidate.  -> the near share"""
    got = np.asarray(got, np.float64)
    share = float(near.mean()) if near.size else 0.0
    assert share <= NEAR_CAP, f"{what}: {share:.4f} of the elements are near a rounding boundary (cap {NEAR_CAP})"
    bad = (got != want) & (got != alt)
    assert not bad.any(), (f"{what}: {int(bad.sum())} / {bad.size} elements are neither allowed value; first at {np.argwhere(bad)[0].tolist()}: "
                           f"got {got[bad][0]!r}, want {want[bad][0]!r}" + (f" or {alt[bad][0]!r}" if alt[bad][0] != want[bad][0] else ""))
    return share


def assert_rel(got, want, budget, what="", floor=0.0):
    """|got - want| <= budget |want| + floor, elementwise.  -> the largest observed relative error"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    bad = ~(err <= budget * np.abs(want) + floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(want != 0, err / np.abs(want), 0.0))) if want.size else 0.0
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.size} elements beyond {budget:.3e} relative; worst {worst:.3e}"
    return worst


def pool_allowed(info, w, H, out_dim, f32):
    """The interval the un-normalised pooled row of a sequence may lie in, [B, out_dim] each: -> (lo, hi, near share).
    bf16 stream: every pooled token's row is one of the hf_candidates; one token: lo / hi are the two candidates (the caller asks for equality
    with one of them); the mean: the token values are added in fp32 in token order and scaled by 1 / L -- the sum of the smaller (larger)
    candidates, less (plus) (L + 1) u sum |y|, divided by L.  fp32 stream: w * (x * rstd) carries rstd_budget + 2 u, the mean adds the same sum term."""
    toks = info["tokens"]
    lo, hi = np.zeros((len(toks), out_dim)), np.zeros((len(toks), out_dim))
    near_n = tot = 0
    for b, t in enumerate(toks):
        if t is None:
            continue
        L = len(t)
        if f32:
            y = info["normed"][t, :out_dim]
            slack = (rstd_budget(H) + 2 * U32) * np.abs(y)
            a, c = y - slack, y + slack
        else:
            want, alt, near = hf_candidates(info["inner"][t, :out_dim], np.asarray(w, np.float64)[:out_dim], rstd_budget(H) + U32)
            a, c = np.minimum(want, alt), np.maximum(want, alt)
            near_n, tot = near_n + int(near.sum()), tot + near.size
        s = ((L + 1) * U32 * np.maximum(np.abs(a), np.abs(c)).sum(0)) if L > 1 else 0.0
        lo[b], hi[b] = (a.sum(0) - s) / L, (c.sum(0) + s) / L
    return lo, hi, (near_n / tot if tot else 0.0)


def normalize_budget(out_dim):
    """relative error of row[i] * (1 / max(sqrtf(sum row^2), 1e-12)) given the row: the sum of out_dim squares over 256 threads, a 6-level
    tree and 3 additions across the waves (halved by the root), sqrtf (1 ulp = 2 u), the division (u), the multiplication (u)"""
    return sum_budget(-(-out_dim // 256), 9) / 2 + 4 * U32


# ---------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (one place: tests/test_elementwise_reference_host.py checks the near-boundary share of exactly these)
# ---------------------------------------------------------------------------------------------------------------
ROWS = (1, 3, 4, 5, 9)                                   # rows % 4 = 1, 3, 0, 1 (two workgroups), 1 (three): four rows per workgroup
RMSNORM_H = (8, 64, 896, 1536, 3584, 8192)
RMSNORM_F32_H = (4, 12, 260, 896, 4096)
EMBED_H = (8, 896, 4096)
POOL_H = (64, 896, 3584)
POOL_LENS = (1, 2, 3, 129, 5)                            # a sequence of exactly each strategy's minimum length and one a token short
GATHER_W = (8, 520, 4096)
GATHER_N = (1, 4, 5)
EPS = 1e-5


def _bf(a):
    return bf16_round(a).astype(np.float32)


def norm_weight(rng, H):
    return _bf(1.0 + 0.1 * rng.standard_normal(H))


def rmsnorm_inputs(H):
    """x bf16-exact fp32 [max(ROWS), H] (the tests run its leading rows), w bf16-exact [H]"""
    rng = np.random.default_rng(1000 + H)
    return _bf(rng.standard_normal((max(ROWS), H)) * 3.0), norm_weight(rng, H)


def rmsnorm_f32_inputs(H):
    rng = np.random.default_rng(2000 + H)
    return (rng.standard_normal((max(ROWS), H)) * 5.0).astype(np.float32), norm_weight(rng, H)


SMALL_H = 896


def small_inputs():
    """rows of RMS 3 * 2^-9: mean(x^2) = 3.4e-5 is of the size of eps = 1e-5, so a lost or misplaced eps moves rstd by 12 % (on the other
    inputs eps is 1e-6 of the mean: within reach of the budget).  hidden [5 tokens, H] bf16-exact, w, cu of two sequences"""
    x, w = rmsnorm_inputs(SMALL_H)
    return (x[:5] * np.float32(2.0 ** -9)), w, np.array([0, 2, 5], np.int32)


def finalize_inputs(n_parts, rows):
    rng = np.random.default_rng(3000 + 7 * n_parts + rows)
    return (rng.random((n_parts, rows)) * 900.0 + 1.0).astype(np.float32)


def embed_inputs(H):
    """table bf16-exact [V, H], ids with the first and the last table row, -1 and V (7 tokens: a second, partly filled workgroup), gamma"""
    rng = np.random.default_rng(4000 + H)
    V = 11
    return _bf(rng.standard_normal((V, H))), np.array([0, V - 1, -1, V, 3, 3, 7], np.int32), _bf(1.0 + 0.2 * rng.standard_normal(H))


def pool_inputs(H, f32, lens=POOL_LENS):
    """hidden [sum(lens), H] (fp32 values, bf16-exact unless f32), w, cu"""
    rng = np.random.default_rng(5000 + H + int(f32))
    x = rng.standard_normal((sum(lens), H)) * 2.0
    return (x.astype(np.float32) if f32 else _bf(x)), norm_weight(rng, H), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def legacy_pool_inputs(H, out_dim, lens):
    """the inputs of tests/test_gpu_kernels.py::test_pool_norm (its seeds, unchanged)"""
    rng = np.random.default_rng(H + out_dim)
    x = _bf(rng.standard_normal((sum(lens), H)).astype(np.float32) * np.float32(2.0))
    return x, _bf(1 + 0.1 * rng.standard_normal(H).astype(np.float32)), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def legacy_strategy_inputs(lens):
    """... and of the real-norm half of test_pool_norm_strategies_against_the_reference_pooling"""
    rng = np.random.default_rng(5)
    x = _bf(rng.standard_normal((sum(lens), 256)).astype(np.float32) * np.float32(2.0))
    return x, _bf(1 + 0.1 * rng.standard_normal(256).astype(np.float32)), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def probe_inputs(rows, H, seed=0):
    """Exact probe: x[r, c] = +-1 with a sign of its own, w[c] = an odd integer below 128 times a power of two (bf16-exact; no two of any 1024
    consecutive columns are equal in magnitude).  With eps = 0 the row statistic is 1 to within rsqrtf's error, bf16(+-1 * rstd) = +-1, and y = w * x bit for bit."""
    rng = np.random.default_rng(6000 + seed + H)
    x = np.where(rng.random((rows, H)) < 0.5, -1.0, 1.0).astype(np.float32)
    c = np.arange(H)
    w = ((2 * (c % 64) + 1) * 2.0 ** ((c // 64) % 16 - 8) * np.where(c % 3 == 0, -1.0, 1.0)).astype(np.float32)   # odd * 2^p: 1024 columns all differ
    return x, w


def gather_inputs(width, n_seqs):
    """an asymmetric bf16-exact source: every element differs from its neighbours in row and column"""
    rng = np.random.default_rng(7000 + width + n_seqs)
    lens = rng.integers(1, 6, size=n_seqs)
    T = int(lens.sum())
    src = _bf((np.arange(T)[:, None] * 3 + 1) * 0.5 + (np.arange(width)[None, :] % 251) * 0.001953125)
    return src, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def near_share_cases():
    """(name, near mask) of every bf16-rounding input above: what the host test caps at NEAR_CAP"""
    for H in RMSNORM_H:
        x, w = rmsnorm_inputs(H)
        yield f"rmsnorm H={H}", hf_candidates(rmsnorm_bf16(x, w, EPS)[1], w, rstd_budget(H) + U32)[2]
    for H in RMSNORM_F32_H:
        x, w = rmsnorm_f32_inputs(H)
        yield f"rmsnorm_f32 H={H}", one_rounding_candidates(rmsnorm_f32(x, w, EPS)[1], rstd_budget(H) + 2 * U32)[2]
    for H in POOL_H + (8192,):
        lens = POOL_LENS if H != 8192 else (2, 3)
        x, w, _ = pool_inputs(H, False, lens)
        yield f"pool_norm bf16 H={H}", hf_candidates(rmsnorm_bf16(x, w, EPS)[1], w, rstd_budget(H) + U32)[2]
    for H, od in ((256, 256), (256, 64), (2048, 2048), (2048, 256)):
        x, w, _ = legacy_pool_inputs(H, od, [3, 1, 40, 17])
        yield f"test_pool_norm H={H} out_dim={od}", hf_candidates(rmsnorm_bf16(x, w, EPS)[1], w, rstd_budget(H) + U32)[2]
    x, w, _ = small_inputs()
    yield "small rows bf16", hf_candidates(rmsnorm_bf16(x, w, EPS)[1], w, rstd_budget(SMALL_H) + U32)[2]
    yield "small rows fp32", one_rounding_candidates(rmsnorm_f32(x, w, EPS)[1], rstd_budget(SMALL_H) + 2 * U32)[2]
    x, w, _ = legacy_strategy_inputs([3, 40, 17, 129, 5])
    yield "strategy test H=256", hf_candidates(rmsnorm_bf16(x, w, EPS)[1], w, rstd_budget(256) + U32)[2]
