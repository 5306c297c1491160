"""The norm, pooling and row-statistic kernels of lrx_elementwise.hip against their float64 restatement (tests/elementwise_reference.py), at
the hidden sizes the served backbones have (896 -- the one with a tail in the per-thread column loops --, 1536, 3584, 4096), at the limits
of each kernel (H = 8 and 8192 of k_rmsnorm's register row, the dynamic-LDS branch of k_pool_norm, the refusals above both) and at every
rows % 4 (four rows per workgroup).

bf16 results follow the comparison rule of elementwise_reference: BIT-EQUAL unless the fp64 pre-rounding value lies within the kernel's fp32
error budget of a rounding boundary, then one of the two neighbours.  The budget is derived there (ER.rstd_budget) from the summation order,
one fp32 rounding per operation and rsqrtf's error.  No HIP math documentation ships with the compiler, so the last is a measured figure,
doubled: test_rsqrtf_alone measures rsqrtf alone over 2^18 arguments and requires the measurement to stay within ER.R_RSQRT_MEASURED =
2^-23, one unit in the last place at the low end of a binade -- the accuracy the CDNA ISA manual states for v_rsq_f32, which the compiler
emits for rsqrtf.  fp32 results are compared relatively within the same budget.  The host file proves that at most 0.21 % of any case's
elements are near a boundary (cap 2 %; 2 budget / 2^-8 predicts 0.1 % at H = 64 and 0.3 % at H = 8192).

Set LRX_ELEMENTWISE_PROFILE=<file> to have the measured figures (largest relative error of rstd, share of near-boundary elements) written
there, one JSON line per kernel and shape."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import elementwise_reference as ER

pytestmark = pytest.mark.gpu

U = ER.U32
_FIGURES = []


def _record(kernel, shape, **fig):
    _FIGURES.append(dict(kernel=kernel, shape=shape, **fig))


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("LRX_ELEMENTWISE_PROFILE")
    if path:
        with open(path, "w") as f:
            for r in _FIGURES:
                f.write(json.dumps(r) + "\n")


def bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(torch.bfloat16).contiguous()


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def i32(a):
    return torch.tensor([int(v) for v in a], dtype=torch.int32, device="cuda")


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def errors(reset=True):
    from lightretriever_amd import _lib
    return int(_lib.lib().lrx_device_error_count(int(reset)))


# ---------------------------------------------------------------------------------------------------------------
# rsqrtf alone, the row statistic
# ---------------------------------------------------------------------------------------------------------------
def test_rsqrtf_alone():
    """finalize_rscale with one partial, H = 1, eps = 0 computes rsqrtf(ss * 1.0f + 0.0f) = rsqrtf(ss): the one ingredient of the budget that
    is measured.  The figure the budget doubles (ER.R_RSQRT_MEASURED) must cover what this run sees."""
    from lightretriever_amd import ops
    rng = np.random.default_rng(0)
    v = np.concatenate([2.0 ** rng.uniform(-20, 20, 1 << 17), rng.uniform(1.0, 4.0, 1 << 17)]).astype(np.float32)
    got = host(ops.finalize_rscale(f32(v)[None, :], 1, 0.0))
    rel = np.abs(got * np.sqrt(v.astype(np.float64)) - 1.0)
    _record("rsqrtf", [v.size], max_rel=float(rel.max()), max_rel_log2=float(np.log2(rel.max())))
    print("rsqrtf: largest relative error", rel.max(), "= 2^%.2f" % np.log2(rel.max()))
    assert rel.max() <= ER.R_RSQRT_MEASURED


@functools.lru_cache(maxsize=None)
def _rms_ref(H):
    x, w = ER.rmsnorm_inputs(H)
    _, inner, _ = ER.rmsnorm_bf16(x, w, ER.EPS)
    return x, w, ER.hf_candidates(inner, w, ER.rstd_budget(H) + U), ER.row_rscale(x, ER.EPS)


@pytest.mark.parametrize("H", ER.RMSNORM_H)
def test_rmsnorm_and_row_rscale(H):
    from lightretriever_amd import ops
    x, w, (want, alt, near), rs = _rms_ref(H)
    xd, wd = bf(x), bf(w)
    worst = 0.0
    for rows in ER.ROWS:
        y = ops.rmsnorm(xd[:rows].contiguous(), wd, ER.EPS)
        share = ER.assert_bf16_rule(host(y), want[:rows], alt[:rows], near[:rows], f"rmsnorm H={H} rows={rows}")
        worst = max(worst, ER.assert_rel(host(ops.row_rscale(xd[:rows].contiguous(), ER.EPS)), rs[:rows], ER.rstd_budget(H), f"row_rscale H={H} rows={rows}"))
    _record("rmsnorm", [max(ER.ROWS), H], near_share=share)
    _record("row_rscale", [max(ER.ROWS), H], rstd_max_rel=worst, budget=ER.rstd_budget(H))
    # rows = 0 (valid pointers: an empty torch tensor has none): OK, and nothing is written
    from lightretriever_amd import _lib
    y, r = torch.full_like(xd, 7.0), torch.full((4,), 7.0, device="cuda")
    _lib.check(_lib.lib().lrx_rmsnorm(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(y), 0, H, ER.EPS, _lib.current_stream()))
    _lib.check(_lib.lib().lrx_row_rscale(_lib.ptr(xd), 0, H, ER.EPS, _lib.ptr(r), _lib.current_stream()))
    assert bool((y == 7.0).all()) and bool((r == 7.0).all())


def test_rmsnorm_refuses_a_row_beyond_its_registers():
    from lightretriever_amd import _lib, ops
    x = torch.zeros(1, 8200, dtype=torch.bfloat16, device="cuda")
    y = torch.full_like(x, 7.0)
    with pytest.raises(_lib.LrxError, match="hidden=8200"):
        _lib.check(_lib.lib().lrx_rmsnorm(_lib.ptr(x), _lib.ptr(x), _lib.ptr(y), 1, 8200, 1e-5, _lib.current_stream()))
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                    # refused before any launch: nothing was written
    with pytest.raises(_lib.LrxError):
        ops.rmsnorm(x[:, :8196].contiguous(), x[0, :8196].contiguous(), 1e-5)           # not a multiple of 8


@pytest.mark.parametrize("H", ER.RMSNORM_F32_H)
def test_rmsnorm_f32(H):
    from lightretriever_amd import ops
    x, w = ER.rmsnorm_f32_inputs(H)
    want, alt, near = ER.one_rounding_candidates(ER.rmsnorm_f32(x, w, ER.EPS)[1], ER.rstd_budget(H) + 2 * U)
    xd, wd = f32(x), bf(w)
    for rows in ER.ROWS:
        share = ER.assert_bf16_rule(host(ops.rmsnorm_f32(xd[:rows].contiguous(), wd, ER.EPS)), want[:rows], alt[:rows], near[:rows], f"rmsnorm_f32 H={H} rows={rows}")
    _record("rmsnorm_f32", [max(ER.ROWS), H], near_share=share)
    from lightretriever_amd import _lib
    y = torch.full((1, H), 7.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().lrx_rmsnorm_f32(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(y), 0, H, ER.EPS, _lib.current_stream()))      # rows = 0: OK, nothing written
    assert bool((y == 7.0).all())


@pytest.mark.parametrize("n_parts", [1, 3, 32])
def test_finalize_rscale(n_parts):
    """the partials are added serially in index order: n_parts - 1 additions of non-negative terms, then the mean, eps and rsqrtf as in rstd_budget"""
    from lightretriever_amd import ops
    H = 896
    budget = (n_parts - 1 + 3) * U / 2 + ER.R_RSQRT
    for rows in (1, 255, 256, 257):
        ss = ER.finalize_inputs(n_parts, rows)
        worst = ER.assert_rel(host(ops.finalize_rscale(f32(ss), H, ER.EPS)), ER.finalize_rscale(ss, H, ER.EPS), budget, f"finalize n_parts={n_parts} rows={rows}")
        _record("finalize_rscale", [n_parts, rows], rstd_max_rel=worst, budget=budget)


@pytest.mark.parametrize("H", ER.EMBED_H)
def test_embed_stream32(H):
    from lightretriever_amd import ops
    table, ids, gamma = ER.embed_inputs(H)
    x32, a16, rs = ER.embed_stream32(table, ids, gamma, ER.EPS)
    errors()
    gx, ga, gr = ops.embed_stream32(bf(table), i32(ids), bf(gamma), ER.EPS)
    np.testing.assert_array_equal(host(gx), x32)                                           # the rows themselves; zeros for ids -1 and V
    np.testing.assert_array_equal(host(ga), a16)                                           # a product of two bf16 numbers is exact before its rounding
    worst = ER.assert_rel(host(gr), rs, ER.rstd_budget(H), f"embed_stream32 rs H={H}")
    assert errors() == 2
    _record("embed_stream32", [len(ids), H], rstd_max_rel=worst, budget=ER.rstd_budget(H))


def saturations():
    from lightretriever_amd import _lib
    return int(_lib.lib().lrx_device_saturation_count(1))


@pytest.mark.parametrize("H", ER.EMBED_H)
def test_embed_stream32_fp16_operand(H):
    """k_embed_stream32<true> (lrx_embed_stream32_ex, f16 = 1: the first launch of every default encoder): a16 is bit-equal to the
    saturating fp16 rounding of x * gamma -- the product of two bf16 numbers is exact in fp32, one rounding in all, budget zero -- and x32
    and rs are the bits the bf16 variant writes for the same inputs; a bad id gives a zero row and is counted"""
    from lightretriever_amd import ops
    table, ids, gamma = ER.embed_inputs(H)
    x32, a16, rs = ER.embed_stream32(table, ids, gamma, ER.EPS, f16=True)
    td, idd, gd = bf(table), i32(ids), bf(gamma)
    bx, ba, br = ops.embed_stream32(td, idd, gd, ER.EPS)
    errors(), saturations()
    gx, ga, gr = ops.embed_stream32(td, idd, gd, ER.EPS, a16_dtype=torch.float16)
    assert ga.dtype == torch.float16
    np.testing.assert_array_equal(host(ga), a16)
    np.testing.assert_array_equal(host(gx), x32)
    assert torch.equal(gx, bx) and torch.equal(gr, br)                                     # the flag changes a16 alone
    assert (host(ga)[[2, 3]] == 0).all() and errors() == 2 and saturations() == 0
    # what the test can see: the fp16 operand is not the bf16 operand converted (3 more bits survive), on a large share of the elements
    assert (host(ga) != host(ba)).mean() > 0.5


def test_embed_stream32_fp16_operand_saturates_by_sign_and_counts_every_element():
    """a norm weight of +-2^18 on two columns: |x * gamma| > 65504 wherever |x| >= 0.25 -- stored as +-65504 by sign, counted once per
    ELEMENT (this kernel has no wave vote); everything else bit-exact; the counter reads 0 after the reset"""
    from lightretriever_amd import ops
    H = 896
    table, ids, gamma = ER.embed_inputs(H)
    gamma = gamma.copy()
    gamma[5], gamma[H - 3] = 2.0 ** 18, -2.0 ** 18
    x32, a16, _ = ER.embed_stream32(table, ids, gamma, ER.EPS, f16=True)
    pre = x32 * gamma.astype(np.float64)
    n_sat = int((np.abs(pre) > 65504).sum())
    assert n_sat >= 4 and (a16 == 65504).any() and (a16 == -65504).any() and (np.abs(pre[:, [5, H - 3]]) < 65504).sum() >= 4       # (two zero rows)
    assert (ER.fp16_ieee(pre) != a16).sum() == n_sat                                       # the store without the clamp differs exactly there
    saturations()
    _, ga, _ = ops.embed_stream32(bf(table), i32(ids), bf(gamma), ER.EPS, a16_dtype=torch.float16)
    np.testing.assert_array_equal(host(ga), a16)
    assert saturations() == n_sat
    assert saturations() == 0


# ---------------------------------------------------------------------------------------------------------------
# pooling + final norm
# ---------------------------------------------------------------------------------------------------------------
def check_pool(got_un, got_n, info, w, H, out_dim, f32_stream, what):
    """the un-normalised rows by the rule (one pooled token: one of the two candidates, equal where the element is not near a boundary; the
    mean / the fp32 stream: inside the interval of ER.pool_allowed); the normalised rows against the float64 normalisation of the kernel's own
    un-normalised rows (same launch arguments otherwise, deterministic kernel) within ER.normalize_budget.  -> near share"""
    lo, hi, share = ER.pool_allowed(info, w, H, out_dim, f32_stream)
    assert share <= ER.NEAR_CAP, (what, share)
    single = np.array([t is not None and len(t) == 1 for t in info["tokens"]])[:, None]
    if f32_stream:
        ok = (got_un >= lo) & (got_un <= hi)
    else:
        ok = np.where(single, (got_un == lo) | (got_un == hi), (got_un >= lo) & (got_un <= hi))
    assert ok.all(), f"{what}: {int((~ok).sum())} / {ok.size} elements outside what the rounding rule allows; first at {np.argwhere(~ok)[0].tolist()}"
    bad = np.array([t is None for t in info["tokens"]])
    assert (got_un[bad] == 0).all(), what
    if got_n is not None:
        assert (got_n[bad] == 0).all(), what
        ER.assert_rel(got_n, ER.l2_normalize(got_un), ER.normalize_budget(out_dim), what + " normalised")
    return share


@functools.lru_cache(maxsize=None)
def _pool_ref(H, f32_stream, lens=ER.POOL_LENS):
    x, w, cu = ER.pool_inputs(H, f32_stream, lens)
    return x, w, cu, (f32(x) if f32_stream else bf(x)), bf(w), i32(cu)


@pytest.mark.parametrize("f32_stream", [False, True])
@pytest.mark.parametrize("H", ER.POOL_H)
def test_pool_norm(H, f32_stream):
    from lightretriever_amd import ops
    x, w, cu, xd, wd, cud = _pool_ref(H, f32_stream)
    for pooling in ER.POOLINGS:
        n_bad = sum(t is None for t in ER.pooled_tokens(cu, pooling))
        for out_dim in (1, 63, 64, H):
            _, info = ER.pool_norm(x, w, cu, ER.EPS, pooling, out_dim, False, f32_stream)
            errors()
            got_un = host(ops.pool_norm(xd, wd, cud, ER.EPS, out_dim, False, pooling=pooling))
            assert errors() == n_bad, (pooling, out_dim)                                    # lens 1, 2, 3: one and two sequences a token short
            got_n = host(ops.pool_norm(xd, wd, cud, ER.EPS, out_dim, True, pooling=pooling))
            share = check_pool(got_un, got_n, info, w, H, out_dim, f32_stream, f"pool_norm {pooling} H={H} out_dim={out_dim} f32={f32_stream}")
        if not f32_stream:
            _record("pool_norm", [H, pooling], near_share=share)
    errors()


def test_eps_counts_where_the_rows_are_small():
    """rows whose mean square is of the size of eps (ER.small_inputs): every kernel that takes eps, same rule and budget.  On the other inputs
    eps is a millionth of the mean square and its loss would hide inside the budget at the larger H."""
    from lightretriever_amd import ops
    x, w, cu = ER.small_inputs()
    H = x.shape[1]
    _, inner, _ = ER.rmsnorm_bf16(x, w, ER.EPS)
    assert ER.row_rscale(x, 0.0)[0] / ER.row_rscale(x, ER.EPS)[0] > 1.1                  # eps is worth more than 10 % of rstd here
    ER.assert_bf16_rule(host(ops.rmsnorm(bf(x), bf(w), ER.EPS)), *ER.hf_candidates(inner, w, ER.rstd_budget(H) + U), "rmsnorm small rows")
    ER.assert_bf16_rule(host(ops.rmsnorm_f32(f32(x), bf(w), ER.EPS)), *ER.one_rounding_candidates(ER.rmsnorm_f32(x, w, ER.EPS)[1], ER.rstd_budget(H) + 2 * U),
                        "rmsnorm_f32 small rows")
    ER.assert_rel(host(ops.row_rscale(bf(x), ER.EPS)), ER.row_rscale(x, ER.EPS), ER.rstd_budget(H), "row_rscale small rows")
    ss = (x.astype(np.float64) ** 2).sum(1).astype(np.float32)[None, :]
    ER.assert_rel(host(ops.finalize_rscale(f32(ss), H, ER.EPS)), ER.finalize_rscale(ss, H, ER.EPS), 3 * U / 2 + ER.R_RSQRT, "finalize_rscale small rows")
    _, _, rs = ER.embed_stream32(x, [4, 0], w, ER.EPS)
    ER.assert_rel(host(ops.embed_stream32(bf(x), i32([4, 0]), bf(w), ER.EPS)[2]), rs, ER.rstd_budget(H), "embed_stream32 small rows")
    for f32_stream in (False, True):
        for pooling in ("lasttoken", "mean"):
            _, info = ER.pool_norm(x, w, cu, ER.EPS, pooling, 64, False, f32_stream)
            xd = f32(x) if f32_stream else bf(x)
            check_pool(host(ops.pool_norm(xd, bf(w), i32(cu), ER.EPS, 64, False, pooling=pooling)), host(ops.pool_norm(xd, bf(w), i32(cu), ER.EPS, 64, True, pooling=pooling)),
                       info, w, H, 64, f32_stream, f"pool_norm small rows {pooling} f32={f32_stream}")


@pytest.mark.parametrize("pooling,H,f32_stream", [("mean", 8192, True), ("mean", 8192, False), ("lasttoken", 16384, True)])
def test_pool_norm_beyond_the_default_dynamic_lds(pooling, H, f32_stream):
    """(H + 4 + (mean ? H : 0)) * 4 bytes = 65552 > 64 KiB at both shapes: the launch has to raise the kernel's dynamic-LDS limit first"""
    from lightretriever_amd import ops
    x, w, cu, xd, wd, cud = _pool_ref(H, f32_stream, (2, 3))
    for out_dim in (64, H):
        _, info = ER.pool_norm(x, w, cu, ER.EPS, pooling, out_dim, False, f32_stream)
        got_un = host(ops.pool_norm(xd, wd, cud, ER.EPS, out_dim, False, pooling=pooling))
        got_n = host(ops.pool_norm(xd, wd, cud, ER.EPS, out_dim, True, pooling=pooling))
        check_pool(got_un, got_n, info, w, H, out_dim, f32_stream, f"pool_norm {pooling} H={H} out_dim={out_dim}")


@pytest.mark.parametrize("pooling,H", [("lasttoken", 40960), ("mean", 20480)])
def test_pool_norm_refuses_a_row_beyond_the_lds(pooling, H):
    from lightretriever_amd import _lib, ops
    x = torch.zeros(2, H, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.LrxError, match="does not fit the LDS"):
        ops.pool_norm(x, x[0].contiguous(), i32([0, 1, 2]), 1e-5, 64, True, pooling=pooling)


def shadow_off(r, k, D):
    """include/lrx.h: element k of row r of the tiled fp16 shadow"""
    return ((r >> 7) * (D // 64) + (k >> 6)) * 8192 + ((((r >> 4) & 7) * 2 + ((k >> 5) & 1)) * 64 + ((k >> 3) & 3) * 16 + (r & 15)) * 8 + (k & 7)


@pytest.mark.parametrize("out_dim", [64, 256])
def test_pool_norm_shard_form_shadow_bounds_and_saturation(out_dim):
    """The shard form also writes fp16(row) into the tiled shadow and raises the two bounds {max |row|, max |row - fp16(row)|}: the bounds are
    functions of the rows as STORED, so their reference is the float64 value over the kernel's own output rows (which the tests above pin).
    Too small a bound loses hits, too large a one costs time: both directions.  Upper side: the fp32 sum of out_dim squares over 256 threads
    (ER.sum_budget, halved by the root), sqrtf (2 u), the product with 1 + 1e-6f (u), and that factor itself."""
    from lightretriever_amd import _lib
    lib = _lib.lib()
    H, row0, sentinel = 256, 130, 77.0
    x, w, cu = ER.pool_inputs(H, False, (3, 1, 6))
    cud = i32(cu)
    budget = ER.sum_budget(-(-out_dim // 256), 9) / 2 + 3 * U

    def run(xa, wa, normalize):
        out = torch.full((3, out_dim), float("nan"), dtype=torch.float32, device="cuda")
        shadow = torch.full((2 * (out_dim // 64) * 8192,), sentinel, dtype=torch.float16, device="cuda")
        bounds = torch.zeros(2, dtype=torch.float32, device="cuda")
        _lib.check(lib.lrx_pool_norm_mode(_lib.ptr(bf(xa)), _lib.ptr(bf(wa)), _lib.ptr(cud), 3, H, ER.EPS, _lib.POOLING["lasttoken"], _lib.ptr(out), out_dim, out_dim,
                                          int(normalize), _lib.ptr(shadow), row0, _lib.ptr(bounds), 0, _lib.current_stream()))
        rows, sh, b = host(out), host(shadow), host(bounds)
        r, e, want_sh = ER.shard_bounds(rows)
        idx = np.array([[shadow_off(row0 + i, k, out_dim) for k in range(out_dim)] for i in range(3)])
        np.testing.assert_array_equal(sh[idx], want_sh)
        rest = np.ones(sh.size, bool)
        rest[idx.ravel()] = False
        assert (sh[rest] == sentinel).all()
        assert r <= b[0] <= r * (1 + budget + 1e-6) and e <= b[1] <= e * (1 + budget + 1e-6), (b, r, e)
        return rows

    lib.lrx_device_saturation_count(1)
    _, info = ER.pool_norm(x, w, cu, ER.EPS, "lasttoken", out_dim, False, False)
    check_pool(run(x, w, False), run(x, w, True), info, w, H, out_dim, False, f"shard form out_dim={out_dim}")
    assert lib.lrx_device_saturation_count(1) == 0
    # one row beyond fp16: sequence 1's pooled token times a weight of 2^18 at columns 3 and 40 (one wave instruction: lanes 3 and 40 of wave 0
    # in its first pass) and, where the row is wide enough, column 70 (wave 1).  k_pool_norm promises one count per wave instruction that met any.
    cols = [3, 40] + ([70] if out_dim > 64 else [])
    xs, ws = x.copy(), w.copy()
    xs[:, cols] = 0.0
    xs[cu[2] - 1, cols] = 4.0
    ws[cols] = 2.0 ** 18
    rows = run(xs, ws, False)
    assert (np.abs(rows[1, cols]) > 65504).all() and (np.abs(np.delete(rows, 1, 0)) < 65504).all()
    assert lib.lrx_device_saturation_count(1) == (2 if out_dim > 64 else 1)


# ---------------------------------------------------------------------------------------------------------------
# exact probes: no tolerance
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 896, 3584, 8192])
def test_probe_rows_of_plus_minus_one(H):
    """x = +-1 with eps = 0: mean(x^2) = 1, rstd = 1 to within rsqrtf's error, bf16(+-1 * rstd) = +-1 (the nearest boundary is 2^-9 away), and
    the result is w * x bit for bit -- each (row, column) has its own sign, each column its own weight: a wrong row, column, chunk or lane
    shows as a wrong number."""
    from lightretriever_amd import ops
    x, w = ER.probe_inputs(9, H)
    want = (w.astype(np.float64) * x)
    for rows in ER.ROWS:
        np.testing.assert_array_equal(host(ops.rmsnorm(bf(x[:rows]), bf(w), 0.0)), want[:rows])
        np.testing.assert_array_equal(host(ops.rmsnorm_f32(f32(x[:rows]), bf(w), 0.0)), want[:rows])
    # the embedding kernel's operand a16 = bf16(x * gamma), rows picked by id
    ids = np.array([8, 0, 3, 3, 5, 1, 7], np.int32)
    gx, ga, gr = ops.embed_stream32(bf(x), i32(ids), bf(w), 0.0)
    np.testing.assert_array_equal(host(ga), want[ids])
    np.testing.assert_array_equal(host(gx), x[ids])
    ER.assert_rel(host(gr), np.ones(len(ids)), ER.rstd_budget(H), "probe rs")


@pytest.mark.parametrize("H", [64, 896, 3584])
def test_probe_pooling_picks_the_right_rows(H):
    """... through k_pool_norm without the L2 normalisation, bf16 stream (its result is a bf16 number; the fp32 stream's w * (x * rstd) is
    exact only if rsqrtf(1) is exactly 1, which no bound promises -- the budget tests cover it).  Token counts are powers of two: the mean of
    +-w over them is exact in fp32 as well (sums of at most 64 odd multiples of a power of two, a division by a power of two)."""
    from lightretriever_amd import ops
    lens = [4, 8, 16, 64, 4]
    cu = np.concatenate([[0], np.cumsum(lens)])
    x, w = ER.probe_inputs(int(cu[-1]), H, seed=1)
    for pooling in ER.POOLINGS:
        for out_dim in (63, H):
            want, _ = ER.pool_norm(x, w, cu, 0.0, pooling, out_dim, False, False)
            got = host(ops.pool_norm(bf(x), bf(w), i32(cu), 0.0, out_dim, False, pooling=pooling))
            np.testing.assert_array_equal(got, want, err_msg=f"{pooling} out_dim={out_dim}")
    assert errors() == 0


@pytest.mark.parametrize("width", ER.GATHER_W)
def test_gather_and_scatter_last_rows(width):
    from lightretriever_amd import _lib, ops
    lib = _lib.lib()
    for n in ER.GATHER_N:
        src, cu = ER.gather_inputs(width, n)
        want, _ = ER.gather_last_rows(src, cu)
        got = ops.gather_last_rows(bf(src), i32(cu))
        np.testing.assert_array_equal(host(got), want)
        # the inverse, into rows wider than the source: dst_row_stride > width, a sentinel everywhere else
        stride, T = width + 24, int(cu[-1])
        dst0 = np.full((T, stride), -3.0, np.float32)
        dst = bf(dst0)
        _lib.check(lib.lrx_scatter_last_rows(_lib.ptr(got), _lib.ptr(i32(cu)), n, width, _lib.ptr(dst), stride, _lib.current_stream()))
        np.testing.assert_array_equal(host(dst), ER.scatter_last_rows(want, cu, dst0)[0])
    assert errors() == 0


# ---------------------------------------------------------------------------------------------------------------
# impossible sequences: cu[b] == cu[b + 1]
# ---------------------------------------------------------------------------------------------------------------
# Every input lives 8 rows into a larger allocation of the test's own, so that row cu[b + 1] - 1 = -1 of an empty FIRST sequence is memory this
# test owns whatever a kernel does with it: the leading rows hold 1e30 (a read of them cannot pass for a zero row) or the sentinel (a write
# to them is seen).
GUARD = 8
EMPTY_LAYOUTS = ([0, 3, 3, 7], [0, 0, 4])


def _without_empty(cu):
    return [c for i, c in enumerate(cu) if i == 0 or c > cu[i - 1]]


@pytest.mark.parametrize("f32_stream", [False, True])
@pytest.mark.parametrize("pooling", ER.POOLINGS)
def test_pool_norm_answers_an_empty_sequence_with_a_zero_row(pooling, f32_stream):
    from lightretriever_amd import ops
    H = 64
    x, w, _ = ER.pool_inputs(H, f32_stream, (3, 4))
    big = torch.full((GUARD + 7, H), 1e30, dtype=torch.float32 if f32_stream else torch.bfloat16, device="cuda")
    big[GUARD:] = f32(x) if f32_stream else bf(x)
    for cu in EMPTY_LAYOUTS:
        view = big[GUARD:GUARD + cu[-1]]
        errors()
        got = host(ops.pool_norm(view, bf(w), i32(cu), ER.EPS, pooling=pooling))
        assert errors() == 1, (pooling, cu)
        ref = host(ops.pool_norm(view, bf(w), i32(_without_empty(cu)), ER.EPS, pooling=pooling))
        assert errors() == 0
        b = [i for i in range(len(cu) - 1) if cu[i + 1] == cu[i]][0]
        assert (got[b] == 0).all(), (pooling, cu, got[b][:4])
        np.testing.assert_array_equal(np.delete(got, b, 0), ref)                           # the neighbours: bit for bit the run without it
        assert np.abs(ref).max() > 0.01


@pytest.mark.parametrize("width", [8, 520])
def test_gather_and_scatter_skip_an_empty_sequence(width):
    from lightretriever_amd import _lib, ops
    lib = _lib.lib()
    src, _ = ER.gather_inputs(width, 5)
    src = src[:7]
    big = torch.full((GUARD + 7, width), 1e30, dtype=torch.bfloat16, device="cuda")
    big[GUARD:] = bf(src)
    for cu in EMPTY_LAYOUTS:
        b = [i for i in range(len(cu) - 1) if cu[i + 1] == cu[i]][0]
        want, empty = ER.gather_last_rows(src, cu)
        assert empty[b] and sum(empty) == 1
        errors()
        got = ops.gather_last_rows(big[GUARD:GUARD + cu[-1]], i32(cu))
        assert errors() == 1, cu
        np.testing.assert_array_equal(host(got), want)                                      # a zero row for the empty sequence
        # scatter: the destination is a view into a sentinel-filled allocation, with guard rows before and after it
        stride, T = width + 8, cu[-1]
        whole = torch.full((GUARD + T + GUARD, stride), -3.0, dtype=torch.bfloat16, device="cuda")
        payload = bf(np.arange(1, (len(cu) - 1) * width + 1, dtype=np.float32).reshape(len(cu) - 1, width) % 251 + 1)
        _lib.check(lib.lrx_scatter_last_rows(_lib.ptr(payload), _lib.ptr(i32(cu)), len(cu) - 1, width, _lib.ptr(whole[GUARD:]), stride, _lib.current_stream()))
        assert errors() == 1, cu
        want_dst, _ = ER.scatter_last_rows(host(payload), cu, np.full((T, stride), -3.0))
        np.testing.assert_array_equal(host(whole[GUARD:GUARD + T]), want_dst)               # the empty sequence's payload row went nowhere
        assert bool((whole[:GUARD] == -3.0).all()) and bool((whole[GUARD + T:] == -3.0).all())
