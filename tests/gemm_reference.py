"""The reference of the bf16 GEMM kernel (lightretriever_amd/csrc/lrx_gemm.hip, k_gemm_bf16_nt) and its six exported epilogues, written once:
each entry point restated in numpy float64 as include/lrx.h and the kernel's comments define it, the error budget an fp32 epilogue may spend
before its 16-bit rounding, the comparison rule built on it, operand generators whose accumulators are EXACT in fp32, and the list of cases
the GPU file runs -- generated here so that the host file proves the preconditions (exact accumulator, exempt share) on the same arrays.
Plain numpy; nothing from lightretriever_amd and no torch.

Exact accumulator.  Operands are small integers times a power of two (bf16-exact).  Every product and every partial sum is then an integer
multiple of one unit with |sum| < 2^24 units: exact in fp32 whatever the summation order and whatever the MFMA rounds internally
(tests/test_gemm_reference_host.py proves it per case).  What follows the accumulator can therefore be required bit for bit at any K.

Comparison rule (the one of tests/elementwise_reference.py, with an absolute budget).  Each reference returns the rounded result, the float64
value before the final rounding (`pre`) and a per-element budget: the bound on |fp32 evaluation - float64| given the exact accumulator.  An
element is required BIT-EQUAL to round(pre) unless a rounding boundary of the output type lies within the budget of pre; then it may be
either neighbour: anything in round(pre - budget) .. round(pre + budget), one output ulp apart unless the value is the small
remainder of a cancellation.  The budget is zero wherever every fp32 step is exact.

Budget bookkeeping (u = 2^-24).  A value is carried as (float64 value, error bound).  One fp32 operation on it
  mul(x, y):  value x y,  error  ex |y| + ey |x| + [inexact] u |x y|
  add(x, y):  value x + y, error ex + ey        + [inexact] u |x + y|
where [inexact] is 1 if an operand already carries an error or the float64 result is not an fp32 number (float64 holds the product of two
fp32 numbers exactly, and every sum used here), else 0: an exact step costs nothing.  The compiler may contract a multiplication and the
following addition into one fma, which rounds once instead of twice: the bound covers both forms."""
import numpy as np

from oracle import lrx_oracle as O
from elementwise_reference import NEAR_CAP, U32, bf16_round, fp16_ieee, fp16_round, fp16_sat

TILE, GBK = 256, 64
BF16_MIN = float(O.BF16_MIN)
SENTINEL = -768.0                                        # bf16-, fp16- and fp32-exact


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def _f64(x):
    return np.asarray(x, np.float64)


def _inexact(v):
    return v.astype(np.float32).astype(np.float64) != v


def mul(x, ex, y, ey=0.0):
    p = x * y
    e = ex * np.abs(y) + ey * np.abs(x)
    return p, e + np.where((e > 0) | _inexact(p), U32 * np.abs(p), 0.0)


def add(x, ex, y, ey=0.0):
    s = x + y
    e = ex + ey + 0.0 * s
    return s, e + np.where((e > 0) | _inexact(s), U32 * np.abs(s), 0.0)


def acc64(A, B):
    return _f64(A) @ _f64(B).T


def n_tiles(N):
    return -(-N // TILE)


def tile_sums(sq, N):
    """[M, N] -> [ceil(N / 256), M]: the sum over each 256-column tile"""
    return np.stack([sq[:, t * TILE:min(N, (t + 1) * TILE)].sum(1) for t in range(n_tiles(N))])


# ---------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------
def store(A, B, bias=None, rscale=None):
    """lrx_gemm_bf16_nt_fused, epilogue 0: C = bf16(acc * rscale[m] + bias[n]).
    Kernel (lrx_gemm.hip, the EPI_STORE branch of the staging loop): v = acc; v *= rs (one fp32 product); v += bias (one fp32 sum); f2bf(v).
    Budget: mul then add of the module docstring -- u |acc rs| if the product is inexact, plus u |acc rs + bias| if the sum is (or inherits
    an error).  Zero for a power-of-two rscale and integer bias on the exact operands.  -> (C, pre, budget)"""
    v = acc64(A, B)
    e = np.zeros_like(v)
    if rscale is not None:
        v, e = mul(v, e, _f64(rscale)[:, None])
    if bias is not None:
        v, e = add(v, e, _f64(bias)[None, :])
    return bf16_round(v), v, e


# roundings any term of ss_part passes: residual epilogue (lrx_gemm.hip, `ssq += f * f` over the 8 elements of a chunk, then row_ror:8,
# row_ror:4, two quad_perm and one __shfl_xor 16): the squares of bf16 numbers are exact, 7 inexact serial additions (the first adds to 0)
# + 5 tree levels
SS_ROUNDINGS_RESID = 12
# fp32 residual epilogue (`(v0 v0 + v1 v1) + (v2 v2 + v3 v3)`, then row_ror:8, row_ror:4, two quad_perm, row_bcast:15, row_bcast:31): one
# rounding of the square, 2 additions, 6 tree levels
SS_ROUNDINGS_RESID32 = 9


def resid(A, B, R):
    """lrx_gemm_bf16_nt_fused, epilogue 1: C = bf16(fp32(bf16(acc)) + R), the reference model's bf16 `residual + linear(x)`.
    Kernel: f2bf(acc) is staged; the read-out computes f2bf(bf2f(staged) + bf2f(resid)): one fp32 addition (RNE), one rounding to bf16.
    With an exact accumulator every step is a single IEEE rounding of exactly known operands, restated here in numpy float32: the budget
    is ZERO everywhere.  ss_part[tn, m] = sum over tile tn's columns of C[m, n]^2 (float64 here; the kernel's fixed tree spends
    SS_ROUNDINGS_RESID roundings per term, all terms non-negative: relative bound SS_ROUNDINGS_RESID * u).  -> (C, pre, budget, ss_part)"""
    inner = O.round_bf16(acc64(A, B).astype(np.float32))
    s = inner + _f32(R)                                              # numpy float32 addition: one RNE rounding
    C = O.round_bf16(s).astype(np.float64)
    return C, _f64(inner) + _f64(R), np.zeros_like(C), tile_sums(C * C, C.shape[1])


def gate_up_columns(N):
    """interleave_gate_up: rows [32 j, 32 j + 16) of the weight are gate rows 16 j .., rows [32 j + 16, 32 j + 32) up rows 16 j .."""
    n = np.arange(N)
    return n[n % 32 < 16], n[n % 32 >= 16]


def interleave_gate_up(Wg, Wu):
    I, H = Wg.shape
    return np.stack([Wg.reshape(I // 16, 16, H), Wu.reshape(I // 16, 16, H)], 1).reshape(2 * I, H)


def swiglu(A, Bi, rscale=None, fmt="bf16"):
    """lrx_gemm_bf16_nt_fused, epilogue 2 on the interleaved weight Bi [N, K]: C[M, N / 2] = bf16(silu(g rs) (u rs)).
    fmt = "fp16": the fp16-operand form (lrx_gemm_nt_fused_ex, f16 = 1; k_gemm_bf16_nt<EPI_SWIGLU, true>) -- the same fp32 arithmetic
    behind the accumulator, the same budget; only the stored format changes: fp16 under the store rule (fp16_sat).
    Kernel: g = acc_g * rs, up = acc_u * rs (fp32 products); sg = v_rcp_f32(1 + v_exp_f32(g * c32)), c32 = fp32(-log2 e); t = g * sg * up.
    Budget, with s(x) = 1 / (1 + exp(-x)) and e = exp(-g):
      the exponent argument g c32 carries the rounding of the constant (u) and of the product (u): 2 u |g| log2 e in the argument, i.e.
        ln 2 times that = 2 u |g| RELATIVE in e (the |g| ln 2 amplification); v_exp_f32 adds 1 ulp = 2 u: e to (2 |g| + 2) u;
      1 + e: the error of e weighs e / (1 + e) = s(-g) in the sum, the addition adds u; v_rcp_f32 1 ulp = 2 u; the two products u each:
        relative (2 |g| + 2) s(-g) u + 5 u of |t|;
      the roundings of g and up themselves (mul above) pass through d silu / dg = s (1 + g (1 - s)) and through silu(g).
    -> (C, pre, budget)"""
    acc = acc64(A, Bi)
    gc, uc = gate_up_columns(Bi.shape[0])
    g, eg = acc[:, gc], np.zeros((acc.shape[0], len(gc)))
    up, eu = acc[:, uc], np.zeros((acc.shape[0], len(uc)))
    if rscale is not None:
        g, eg = mul(g, eg, _f64(rscale)[:, None])
        up, eu = mul(up, eu, _f64(rscale)[:, None])
    s = 1.0 / (1.0 + np.exp(-g))
    pre = g * s * up
    budget = np.abs(up * s * (1.0 + g * (1.0 - s))) * eg + np.abs(g * s) * eu + np.abs(pre) * U32 * ((2.0 * np.abs(g) + 2.0) * (1.0 - s) + 5.0)
    return (fp16_sat(pre) if fmt == "fp16" else bf16_round(pre)), pre, budget


def rotary_pair_order(nq, nkv, d):
    """ops.rotary_pair_order in numpy: physical row 32 g + 16 i + t of a q / k head = logical row i d/2 + 16 g + t; v rows in place"""
    t = np.arange(d)
    head = ((t % 32) // 16) * (d // 2) + 16 * (t // 32) + t % 16
    return np.concatenate([h * d + head for h in range(nq + nkv)] + [np.arange((nq + nkv) * d, (nq + 2 * nkv) * d)])


def rope_table(d, n_pos, theta=10000.0):
    """an fp32 cos / sin table [n_pos, d / 2] (the kernel takes whatever table it is handed; position 0 is cos = 1, sin = 0 exactly)"""
    inv = (1.0 / theta ** (np.arange(0, d, 2, dtype=np.float64) / d)).astype(np.float32)
    fr = (np.arange(n_pos, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return np.cos(fr).astype(np.float32), np.sin(fr).astype(np.float32)


def qkv_rope(A, Wp, positions, cos, sin, nq, nkv, d, bias_p=None, rscale=None, head0=0, n_heads=None):
    """lrx_gemm_qkv_rope_slice: Wp / bias_p in rotary-pair (physical) order; -> the fp16 columns of heads [head0, head0 + n_heads), physical
    order.  Restated in LOGICAL order -- x = acc rs + bias; apply_rotary_pos_emb on every q and k head: (x1, x2) = the halves of the head,
    out = (x1 c - x2 s, x2 c + x1 s) with c, s = table[position] -- and permuted back with rotary_pair_order; v columns are not rotated.
    Kernel (EPI_ROPE): x *= rs; x += bias; x1' = a c - b s, x2' = b c + a s in fp32; one rounding to fp16, saturating at +-65504.
    Budget: mul and add of the module docstring for the row scale and bias, then mul, mul, add for each output of the rotation (a product
    with c or s in {0, +-1} is exact: position 0 costs nothing).
    -> (C, pre, budget)"""
    n_all = nq + 2 * nkv
    n_heads = n_all - head0 if n_heads is None else n_heads
    perm = rotary_pair_order(nq, nkv, d)
    Wl = np.empty_like(_f64(Wp))
    Wl[perm] = _f64(Wp)
    v = acc64(A, Wl)
    e = np.zeros_like(v)
    if rscale is not None:
        v, e = mul(v, e, _f64(rscale)[:, None])
    if bias_p is not None:
        bl = np.empty(len(perm))
        bl[perm] = _f64(bias_p)
        v, e = add(v, e, bl[None, :])
    M, h2 = v.shape[0], d // 2
    rot = (nq + nkv) * d
    x, ex = v[:, :rot].reshape(M, nq + nkv, d), e[:, :rot].reshape(M, nq + nkv, d)
    c, s = _f64(cos)[np.asarray(positions)][:, None, :], _f64(sin)[np.asarray(positions)][:, None, :]
    x1, e1, x2, e2 = x[..., :h2], ex[..., :h2], x[..., h2:], ex[..., h2:]
    ac, bs, bc, as_ = mul(x1, e1, c), mul(x2, e2, s), mul(x2, e2, c), mul(x1, e1, s)
    o1, f1 = add(ac[0], ac[1], -bs[0], bs[1])
    o2, f2 = add(bc[0], bc[1], as_[0], as_[1])
    ro, re = np.concatenate([o1, o2], -1), np.concatenate([f1, f2], -1)
    pre = np.concatenate([ro.reshape(M, rot), v[:, rot:]], 1)[:, perm]
    bud = np.concatenate([re.reshape(M, rot), e[:, rot:]], 1)[:, perm]
    sl = slice(head0 * d, (head0 + n_heads) * d)
    return fp16_round(pre[:, sl]), pre[:, sl], bud[:, sl]


def resid32(A, B, x32, gamma=None, fmt="bf16"):
    """lrx_gemm_bf16_nt_resid32: x32 = fp32(x32 + acc); a16 = bf16(fp32(x32 gamma[n])); ss_part from the fp32 row.
    fmt = "fp16" (lrx_gemm_nt_resid32_ex, out_f16 = 1; the OUTH branch): a16 = fp16(fp32(x32 gamma[n])) under the store rule.  Two
    roundings of one number: an exact product within half an fp32 ulp of an fp16 midpoint (one element in 2^13) rounds otherwise than
    fp16(x32 gamma) would, so the value handed to the comparison as `pre_a` is the fp32 PRODUCT, restated in numpy float32 -- the kernel's
    own sequence -- and the budget stays zero.  (The bf16 form keeps the exact product as pre_a: there the two differ in one element in
    2^16.)  fp16 operands (f16 = 1) change nothing here: the accumulator is exact either way.
    Kernel (EPI_RESID32): v = staged acc + x32 (one fp32 addition of exactly known operands), stored; f2bf(v * gm) -- one fp32 product, one
    rounding to bf16, nothing an fma could merge.  Each step is one IEEE rounding, restated in numpy float32: budget ZERO for both outputs.
    ss_part: float64 sum of the new row's squares per tile (kernel: SS_ROUNDINGS_RESID32 roundings per term).
    -> (x32, a16, pre_x, pre_a, budget, ss_part)"""
    acc = acc64(A, B)
    x = _f32(x32) + acc.astype(np.float32)
    g = np.ones(x.shape[1], np.float32) if gamma is None else _f32(gamma)
    x64 = _f64(x)
    if fmt == "fp16":
        with np.errstate(over="ignore", invalid="ignore"):
            pa = _f64(x * g[None, :])
        return x64, fp16_sat(pa), _f64(x32) + acc, pa, np.zeros_like(x64), tile_sums(x64 * x64, x.shape[1])
    a16 = O.round_bf16(x * g[None, :])
    return x64, _f64(a16), _f64(x32) + acc, x64 * _f64(g)[None, :], np.zeros_like(x64), tile_sums(x64 * x64, x.shape[1])


def row_segments(cu, tok_mask):
    """k_build_row_seg: the sequence of token t where tok_mask selects it, else -1"""
    seg = np.full(int(cu[-1]), -1, np.int64)
    for b in range(len(cu) - 1):
        seg[int(cu[b]):int(cu[b + 1])] = b
    return np.where(np.asarray(tok_mask).astype(bool), seg, -1)


def max_aggregate(A, B, bias, row_seg, n_seqs, init=BF16_MIN):
    """lrx_sparse_max_aggregate: out[seg, n] = max(out[seg, n], bf16(acc + bias[n])) over the rows with seg >= 0, from `init`.
    Kernel (EPI_MAXAGG): v = acc + bias (one fp32 addition of exactly known operands), f2bf, maxima: restated in numpy float32, budget ZERO.
    -> (out fp32, the bf16 logits, budget)"""
    acc = acc64(A, B).astype(np.float32)
    logits = O.round_bf16(acc + _f32(bias)[None, :] if bias is not None else acc)
    out = np.full((n_seqs, logits.shape[1]), init, np.float32)
    for b in range(n_seqs):
        rows = logits[np.asarray(row_seg) == b]
        if len(rows):
            out[b] = np.maximum(out[b], rows.max(0))
    return out, logits, np.zeros(out.shape)


# ---------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------
def _round(fmt):
    return {"bf16": bf16_round, "fp16": fp16_sat, "fp32": lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)}[fmt]


def ulp(v, fmt):
    bits = {"bf16": 8, "fp16": 11, "fp32": 24}[fmt]
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.ldexp(1.0, e - bits)


def allowed(pre, budget, fmt):
    """-> (want, lo, hi, exempt): round(pre), and the two ends of what an evaluation within `budget` of pre may round to"""
    r = _round(fmt)
    want, lo, hi = r(pre), r(pre - budget), r(pre + budget)
    return want, lo, hi, lo != hi


def exempt_share(pre, budget, fmt, what=""):
    """the precondition of the rule, from the reference alone: at most NEAR_CAP of the elements may be exempt, none where the budget is zero.
    (An exempt element normally has ONE boundary in reach and its two candidates are neighbours; where a rotation or a bias cancels most of
    the value, the budget -- a multiple of the operands' size, not of the result's -- can span a few ulps of the small result: such an
    element is held to [lo, hi] and counts as exempt like any other.)  -> the share"""
    _, lo, hi, ex = allowed(pre, budget, fmt)
    share = float(ex.mean()) if ex.size else 0.0
    assert share <= NEAR_CAP, f"{what}: {share:.4f} of the elements lie within their budget of a rounding boundary (cap {NEAR_CAP})"
    assert not (ex & (np.asarray(budget) == 0)).any(), f"{what}: an element with zero budget is exempt"
    return share


def check(got, pre, budget, fmt, what="", describe=None):
    """bit-equality with round(pre) outside the exemption, [lo, hi] inside.  -> {exempt, mismatches, dist}: the exempt share, the number of
    elements that differ from round(pre), and the largest distance of such an element's pre from the boundary it crossed, in budgets"""
    got = np.asarray(got, np.float64)
    want, lo, hi, ex = allowed(pre, budget, fmt)
    share = exempt_share(pre, budget, fmt, what)
    diff = got != want
    bad = np.where(ex, (got < lo) | (got > hi) | np.isnan(got), diff)
    if bad.any():
        i = tuple(np.argwhere(bad)[0].tolist())
        extra = f" ({describe(i, got[i])})" if describe else ""
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.size} elements are not what the rounding sequence gives; first at {list(i)}: "
                             f"got {got[i]!r}, want {want[i]!r}, pre {pre[i]!r}, budget {np.broadcast_to(budget, pre.shape)[i]:.3e}{extra}")
    dist = 0.0
    if diff.any():
        b = np.broadcast_to(budget, pre.shape)[diff]
        dist = float((np.abs(pre[diff] - (got[diff] + want[diff]) / 2) / b).max())
    return {"exempt": share, "mismatches": int(diff.sum()), "dist": dist}


def check_ss(got, want, roundings, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    bad = ~(err <= roundings * U32 * want)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.size} partial sums beyond {roundings} u relative; first at {np.argwhere(bad)[0].tolist()}"
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(want > 0, err / want, 0.0)) / U32) if want.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
# operand generators
# ---------------------------------------------------------------------------------------------------------------
def int_range(K):
    """largest operand integer: 15 up to K = 512 (225 * 512 < 2^17 units), 7 beyond (49 * 8192 < 2^19 units)"""
    return 15 if K <= 512 else 7


def exact_operands(rng, M, N, K, a_scale=2.0 ** -3, b_scale=2.0 ** -4):
    """A [M, K], B [N, K]: integers in [-int_range, int_range] times a power of two: bf16-exact, no subnormals, |sum| < 2^24 units"""
    r = int_range(K)
    return (rng.integers(-r, r + 1, (M, K)) * a_scale).astype(np.float32), (rng.integers(-r, r + 1, (N, K)) * b_scale).astype(np.float32)


def wide_operands(rng, M, N, K):
    """The wide-mantissa exact family, which no bf16 operand can express: A = integers in +-1023 times 2^-10 (all 11 significant bits of
    fp16; 3 more than bf16 holds), B = integers in +-15 times 2^-4.  K <= 512: |sum| <= 1023 * 15 * 512 < 2^23 units of 2^-14."""
    assert K <= 512
    return (rng.integers(-1023, 1024, (M, K)) * 2.0 ** -10).astype(np.float32), (rng.integers(-15, 16, (N, K)) * 2.0 ** -4).astype(np.float32)


def one_hot_rows_wide(M, N, K):
    """one_hot_rows with 11-bit B values: B[n, k] = +-(1024 + (53 n + 7 k) mod 1023), odd and even, every one of them needing bits that bf16
    drops; C[m, n] = B[n, pi(m)] names the K element and the row that were read, to the last of fp16's 11 bits"""
    A, _ = one_hot_rows(M, N, K)
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    return A, ((1024 + (53 * n + 7 * k) % 1023) * np.where((n + k) % 2, -1.0, 1.0)).astype(np.float32)


def subnormal_probe(M, K):
    """fp16-SUBNORMAL operands: one-hot A (pi of one_hot_rows), B[n, k] = j 2^-24 with j = 1 + (n K + k) mod 1023 -- every fp16 subnormal
    1 .. 1023 for N K >= 1023.  IEEE arithmetic gives C[m, n] = B[n, pi(m)] exactly (1 x a subnormal, summed with zeros)."""
    N = 16
    A, _ = one_hot_rows(M, N, K)
    j = 1 + (np.arange(N)[:, None] * K + np.arange(K)[None, :]) % 1023
    return A, (j * 2.0 ** -24).astype(np.float32)


def is_fp16_exact(a):
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):
        return bool((a.astype(np.float16).astype(np.float32) == a).all())


def has_fp16_subnormals(a):
    a = np.abs(np.asarray(a, np.float64))
    return bool(((a > 0) & (a < 2.0 ** -14)).any())


def sum_units(A, B):
    """the largest |A| . |B| row sum in units of the smallest product: what must stay below 2^24"""
    A, B = np.abs(_f64(A)), np.abs(_f64(B))
    unit = A[A > 0].min() * B[B > 0].min()
    return float((A @ B.T).max() / unit), unit


def swiglu_b_scale(K):
    """pre-activations of standard deviation ~ 3-5 at every K: mostly within +-8, with a tail"""
    r = int_range(K)
    sd = (r * (r + 1) / 3.0) * np.sqrt(K) * 2.0 ** -3                # sd of sum of K products of two uniform integers, A scaled by 2^-3
    return 2.0 ** -int(np.ceil(np.log2(sd / 4.0)))


def bf16_values(rng, shape, scale=1.0):
    return O.round_bf16((rng.standard_normal(shape) * scale).astype(np.float32))


def one_hot_rows(M, N, K):
    """A[m, pi(m)] = 1 with pi(m) = (37 m + 11) mod K, B[n, k] a small integer that depends on both n and k: C[m, n] = B[n, pi(m)] names
    the K element and the row that were read"""
    A = np.zeros((M, K), np.float32)
    A[np.arange(M), (37 * np.arange(M) + 11) % K] = 1.0
    B = (((np.arange(N)[:, None] * 7 + np.arange(K)[None, :] * 3) % 127 + 1) * np.where((np.arange(N)[:, None] + np.arange(K)[None, :]) % 2, -1.0, 1.0)).astype(np.float32)
    return A, B


def identity_operands(K, N):
    """A = I against an asymmetric B (tests/test_gpu_kernels.py::test_gemm_identity_asymmetric, at other K)"""
    return np.eye(K, dtype=np.float32), ((np.arange(N)[:, None] * 3 + np.arange(K)[None, :] % 7) % 61).astype(np.float32)


def coded_operands(M, N, K=GBK):
    """C[m, n] = (-1)^(m / 256 + n / 256) 2^(m mod 199 - 99) (128 + n mod 127) / 128: a bf16 number (sign, exponent, mantissa) that encodes
    the row (mod 199: rows 256 apart differ), the column (mod 127) and the parity of the tile pair.  A is one-hot at column m mod K."""
    m, n = np.arange(M), np.arange(N)
    A = np.zeros((M, K), np.float32)
    A[m, m % K] = np.ldexp(np.where((m // TILE) % 2, -1.0, 1.0), m % 199 - 99)
    B = np.repeat((np.where((n // TILE) % 2, -1.0, 1.0) * (128 + n % 127) / 128.0)[:, None], K, 1).astype(np.float32)
    return A, B


def decode_coded(i, v):
    if v == 0 or not np.isfinite(v):
        return f"value {v!r} is no code"
    m, e = np.frexp(abs(v))
    return (f"the value found there is the code of a row = {int(e - 1 + 99)} mod 199 and a column = {int(round(m * 256 - 128))} mod 127, tile parity "
            f"{'odd' if v < 0 else 'even'}; expected row {i[0]} = {i[0] % 199} mod 199, column {i[1]} = {i[1] % 127} mod 127")


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_gemm_reference.py
# ---------------------------------------------------------------------------------------------------------------
K_LOOP = [(300, 264, 64 * nk) for nk in (1, 2, 3, 4, 5, 7)] + [(131, 64, 8192)]
# every M % 256 in {0, 1, 127, 128, 129, 255} and N % 256 in {0, 8, 248}, nk in {1, 3, 4}; N = 8 and N = 264 (resid32)
EDGES = [(256, 256, 64), (257, 8, 192), (127, 248, 256), (128, 264, 64), (129, 504, 192), (255, 520, 256)]
# SwiGLU: N % 32 == 0 and N / 2 no multiple of 128
EDGES_SWIGLU = [(256, 224, 64), (257, 32, 192), (127, 288, 256), (128, 480, 64), (129, 544, 192), (255, 96, 256)]
# max aggregate: the vocabulary need not be a multiple of 8
EDGES_MAXAGG = [(256, 256, 64), (257, 13, 192), (127, 250, 256), (128, 259, 64), (129, 504, 192), (255, 521, 256), (600, 300, 64)]
TILE_MAP = [(3333, 520), (2049, 8), (1, 8), (257, 1032), (512, 512)]
# (d, nq, nkv, bias, rscale, M, K): (nq + nkv) d = 384 / 384 lies inside a 256-column tile, 512 / 256 on a tile edge
ROPE = [(64, 4, 2, False, False, 257, 64), (128, 2, 1, True, True, 127, 192), (128, 2, 2, True, False, 129, 256), (64, 3, 1, False, True, 255, 64)]
N_POS = 128


def _case(name, epi, family, M, N, K, **kw):
    return dict(name=name, epi=epi, family=family, M=M, N=N, K=K, **kw)


def gpu_cases():
    cs = []
    for M, N, K in K_LOOP:
        cs.append(_case(f"kloop-store-nk{K // GBK}", "store", "exact", M, N, K))
    for M, N, K in EDGES:
        for fam in ("exact", "general"):
            cs.append(_case(f"store-{fam}-{M}x{N}x{K}", "store", fam, M, N, K))
            cs.append(_case(f"resid-{fam}-{M}x{N}x{K}", "resid", fam, M, N, K))
            cs.append(_case(f"resid32-{fam}-{M}x{N}x{K}", "resid32", fam, M, N, K))
    for M, N, K in EDGES_SWIGLU:
        cs.append(_case(f"swiglu-{M}x{N}x{K}", "swiglu", "general", M, N, K))
    # the tile map under the SwiGLU value of group_m (6: groups of 6, 6 and 2 m-tiles), 14 x 3 workgroups
    cs.append(_case("swiglu-tilemap-3333x544x64", "swiglu", "general", 3333, 544, 64))
    for M, N, K in EDGES_MAXAGG:
        cs.append(_case(f"maxagg-{M}x{N}x{K}", "maxagg", "exact", M, N, K))
    cs.append(_case("maxagg-negative-300x264x192", "maxagg", "exact", 300, 264, 192, negative=True))
    for d, nq, nkv, b, r, M, K in ROPE:
        for pos0 in (False, True):
            if pos0 and (b or r):
                continue
            cs.append(_case(f"rope-d{d}-q{nq}kv{nkv}-b{int(b)}r{int(r)}-{M}x{K}" + ("-pos0" if pos0 else ""), "rope", "exact" if pos0 else "general",
                            M, (nq + 2 * nkv) * d, K, d=d, nq=nq, nkv=nkv, bias=b, rscale=r, pos0=pos0))
    return cs


def gpu_cases_f16():
    """the fp16-operand / fp16-output instantiations (lrx_*_ex): the shapes above and nothing larger.  f16: A and B are fp16; out_f16
    (resid32): a16 is fp16; the SwiGLU output is fp16 with f16.  The operands are the SAME arrays as the bf16 case of the same shape would
    get (the seed is taken from `base`), all fp16-exact."""
    cs = []
    for d, nq, nkv, b, r, M, K in ROPE:
        for pos0 in (False, True):
            if pos0 and (b or r):
                continue
            base = f"rope-d{d}-q{nq}kv{nkv}-b{int(b)}r{int(r)}-{M}x{K}" + ("-pos0" if pos0 else "")
            cs.append(_case("f16-" + base, "rope", "exact" if pos0 else "general", M, (nq + 2 * nkv) * d, K, d=d, nq=nq, nkv=nkv, bias=b, rscale=r,
                            pos0=pos0, f16=1, base=base))
    for M, N, K in EDGES:
        for fam in ("exact", "general"):
            for f16, oh in ((1, 1), (0, 1)):
                cs.append(_case(f"resid32-f{f16}h{oh}-{fam}-{M}x{N}x{K}", "resid32", fam, M, N, K, f16=f16, out_f16=oh, base=f"resid32-{fam}-{M}x{N}x{K}"))
    # the last layer's down-projection: fp16 operands, nothing written for a next projection
    cs.append(_case("resid32-f1h1-noa16-exact-129x504x192", "resid32", "exact", 129, 504, 192, f16=1, out_f16=1, no_a16=True, base="resid32-exact-129x504x192"))
    for M, N, K in EDGES_SWIGLU:
        cs.append(_case(f"f16-swiglu-{M}x{N}x{K}", "swiglu", "general", M, N, K, f16=1, base=f"swiglu-{M}x{N}x{K}"))
    cs.append(_case("f16-swiglu-tilemap-3333x544x64", "swiglu", "general", 3333, 544, 64, f16=1, base="swiglu-tilemap-3333x544x64"))
    for M, N, K in K_LOOP:                                           # the fp32 x32 output shows the accumulator exactly
        cs.append(_case(f"kloop-resid32-f1h1-nk{K // GBK}", "resid32", "exact", M, N, K, f16=1, out_f16=1))
    cs.append(_case("resid32-f1h1-tilemap-3333x520x64", "resid32", "exact", 3333, 520, 64, f16=1, out_f16=1))
    # the wide-mantissa family: every M % 256 / N % 256 class once more, nk = 3, 4, 8
    for M, N, K in ((129, 504, 192), (255, 520, 256), (300, 264, 512)):
        cs.append(_case(f"resid32-f1h1-wide-{M}x{N}x{K}", "resid32", "exact", M, N, K, f16=1, out_f16=1, wide=True))
    return cs


F16_CASES_BY_NAME = None


def f16_case(name):
    global F16_CASES_BY_NAME
    if F16_CASES_BY_NAME is None:
        F16_CASES_BY_NAME = {c["name"]: c for c in gpu_cases_f16()}
    return F16_CASES_BY_NAME[name]


SATURATION = ("swiglu-f1", "resid32-f1h1", "resid32-f0h1")


def saturation_inputs(which):
    """Inputs on which the fp16 stores of the SwiGLU (f16) and resid32 (out_f16) epilogues leave fp16's range -- defined behaviour with finite
    stores: +-65504 by sign, a NaN as -65504.  -> (case, inp, ref without ss_part)
      swiglu:   rows 3, 100, 128 under a row scale of 2^10 (a power of two: g and u stay exact; |silu(g) u| reaches 1e8 where g > 0, and is 0
                where g << 0); row 7 is a zero row of A under an infinite row scale: 0 x inf = NaN in every column.
      resid32:  gamma = +-2^14 on columns 5 and 300 (|x32| <= 110: saturated wherever |x32| > 3.998, exact below), and a NaN, a +inf and a
                -inf in the incoming x32 (x32 keeps them; a16 holds -65504, or +-65504 by the sign of inf x gamma, or -65504 for inf x 0)."""
    if which == "swiglu-f1":
        case = dict(f16_case("f16-swiglu-129x544x192"), name="saturation-" + which)
        inp = {k: (None if v is None else v.copy()) for k, v in case_inputs(case).items()}
        inp["A"][7] = 0.0
        inp["rscale"] = np.ones(case["M"], np.float32)
        inp["rscale"][[3, 100, 128]] = 2.0 ** 10
        inp["rscale"][7] = np.inf
    else:
        case = dict(f16_case(which + "-exact-129x504x192"), name="saturation-" + which)
        inp = {k: v.copy() for k, v in case_inputs(case).items()}
        inp["gamma"][5], inp["gamma"][300] = 2.0 ** 14, -2.0 ** 14
        inp["x32"][7, 9], inp["x32"][7, 10], inp["x32"][8, 10], inp["x32"][8, 5] = np.nan, np.inf, -np.inf, np.inf
    with np.errstate(all="ignore"):
        ref = case_reference(case, inp)
    ref.pop("ss", None)
    return case, inp, ref


def _seed(case):
    case = dict(case, name=case.get("base", case["name"]))
    return int(np.frombuffer(case["name"].encode().ljust(64, b"\0")[:64], np.uint32).sum() % (2 ** 31))


def max_agg_layout(M):
    """cu_seqlens and tok_mask: lengths 1, 3, 9 (several segments inside one lane's row walk, which visits every 8th row), long ones that cross
    the 256-row tile boundaries, one sequence without any selected token, and masked rows at tile starts and ends"""
    lens, pat, i = [], (1, 3, 9, 120, 2, 5, 250, 1, 3, 9, 9, 40), 0
    while sum(lens) < M:
        lens.append(min(pat[i % len(pat)], M - sum(lens)))
        i += 1
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    mask = np.ones(M, np.uint8)
    for r in (0, 255, 256, 257, 511, 512, M - 1):
        if 0 <= r < M:
            mask[r] = 0
    mask[10::17] = 0
    if len(lens) > 5:
        mask[cu[5]:cu[6]] = 0                                        # sequence 5 keeps the initial value
    return cu, mask


def case_inputs(case):
    """every array of a case, as float32 / int numpy arrays holding bf16-exact values where the kernel takes bf16"""
    rng = np.random.default_rng(_seed(case))
    M, N, K, epi, exact = case["M"], case["N"], case["K"], case["epi"], case["family"] == "exact"
    inp = {}
    if epi == "swiglu":
        A, Wg = exact_operands(rng, M, N // 2, K, b_scale=swiglu_b_scale(K))
        _, Wu = exact_operands(rng, 1, N // 2, K, b_scale=swiglu_b_scale(K))
        inp.update(A=A, B=interleave_gate_up(Wg, Wu), rscale=rng.uniform(0.2, 3.0, M).astype(np.float32) if M % 2 else None)
        return inp
    A, B = wide_operands(rng, M, N, K) if case.get("wide") else exact_operands(rng, M, N, K)
    if case.get("negative"):
        A, B = np.abs(A) + np.float32(2.0 ** -3), -np.abs(B) - np.float32(2.0 ** -4)
    inp.update(A=A, B=B)
    ints = lambda shape, r=8: rng.integers(-r, r + 1, shape).astype(np.float32)
    if epi == "store":
        inp["bias"] = ints(N) if exact else bf16_values(rng, N, 2.0)
        inp["rscale"] = (2.0 ** rng.integers(-2, 3, M)).astype(np.float32) if exact else rng.uniform(0.2, 3.0, M).astype(np.float32)
    elif epi == "resid":
        inp["R"] = ints((M, N)) if exact else bf16_values(rng, (M, N), 3.0)
    elif epi == "resid32":
        inp["x32"] = ints((M, N), 64) if exact else (rng.standard_normal((M, N)) * 3.0).astype(np.float32)
        inp["gamma"] = ints(N, 4) if exact else O.round_bf16((1.0 + 0.3 * rng.standard_normal(N)).astype(np.float32))
    elif epi == "maxagg":
        inp["bias"] = ints(N)
        if case.get("negative"):
            inp["bias"] = -np.abs(inp["bias"])
        inp["cu"], inp["mask"] = max_agg_layout(M)
        if not case.get("negative"):
            # exact zeros among the logits: zero rows of A under a bias that holds +0 and -0 (0 + -0 = +0 in fp32: the logit is +0), next to
            # rows whose logits are negative in those columns
            A[3::11] = 0.0
            inp["bias"][::5] = 0.0
            inp["bias"][::10] = -0.0
    elif epi == "rope":
        d, nq, nkv = case["d"], case["nq"], case["nkv"]
        inp["cos"], inp["sin"] = rope_table(d, N_POS)
        inp["positions"] = np.zeros(M, np.int32) if case["pos0"] else rng.integers(0, N_POS, M).astype(np.int32)
        inp["bias"] = bf16_values(rng, N, 2.0) if case["bias"] else None
        inp["rscale"] = rng.uniform(0.2, 3.0, M).astype(np.float32) if case["rscale"] else None
    return inp


def case_reference(case, inp):
    """-> {output name: (want, pre, budget, fmt)} and, under 'ss', (ss_part, roundings)"""
    epi = case["epi"]
    if epi == "store":
        return {"C": store(inp["A"], inp["B"], inp["bias"], inp["rscale"]) + ("bf16",)}
    if epi == "resid":
        C, pre, b, ss = resid(inp["A"], inp["B"], inp["R"])
        return {"C": (C, pre, b, "bf16"), "ss": (ss, SS_ROUNDINGS_RESID)}
    if epi == "swiglu":
        fmt = "fp16" if case.get("f16") else "bf16"
        return {"C": swiglu(inp["A"], inp["B"], inp["rscale"], fmt) + (fmt,)}
    if epi == "resid32":
        fmt = "fp16" if case.get("out_f16") else "bf16"
        x, a, px, pa, b, ss = resid32(inp["A"], inp["B"], inp["x32"], inp["gamma"], fmt)
        ref = {"x32": (x, px, b, "fp32"), "a16": (a, pa, b, fmt), "ss": (ss, SS_ROUNDINGS_RESID32)}
        if case.get("no_a16"):
            del ref["a16"]
        return ref
    if epi == "maxagg":
        out, _, b = max_aggregate(inp["A"], inp["B"], inp["bias"], row_segments(inp["cu"], inp["mask"]), len(inp["cu"]) - 1)
        return {"out": (_f64(out), _f64(out), b, "fp32")}
    if epi == "rope":
        return {"C": qkv_rope(inp["A"], inp["B"], inp["positions"], inp["cos"], inp["sin"], case["nq"], case["nkv"], case["d"], inp["bias"], inp["rscale"]) + ("fp16",)}
    raise KeyError(epi)
