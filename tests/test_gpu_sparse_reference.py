"""The sparsify, compaction and hit-fusion kernels (lightretriever_amd/csrc/lrx_sparse.hip, lrx_fuse.hip) against their restatement
(tests/sparse_reference.py) at their edges: widths below, at and above one pass of a workgroup, strided rows, capacities that cut inside a
wave / at a wave end / at a chunk end / at the count, tied and holed hit lists, the 4096-entry limit of the fusion sort, four systems.

Bit-level almost everywhere (the module docstring of sparse_reference says why): the selection, the quantisation and the float64 fusion are
exactly reproducible; the bf16-rounded log1p is compared exhaustively over every positive bf16 argument with nothing left out; only the
unrounded log1p carries a budget, BUDGET_ULP = twice the error test_log1pf_alone measures, and only there may elements be left out of a
quantised comparison (those the host test proves near a half, at most 0.5 %).

Where a stride, a capacity or a caller-owned output matters the C entry points are called through _lib on buffers prefilled with a
sentinel: row padding, unused output slots and a guard stretch behind every buffer must come back untouched.

Set LRX_SPARSE_PROFILE=<file> to have the measured log1pf figure written there as one JSON line."""
import json
import os

import numpy as np
import pytest
import torch

import sparse_reference as SR

pytestmark = pytest.mark.gpu

GUARD = 8                     # sentinel elements behind the last row of every buffer


def _lib():
    from lightretriever_amd import _lib as L
    return L


def put(x, ld, sentinel, dtype):
    """a device buffer of rows * ld + GUARD elements holding x [rows, cols] at row stride ld, everything else the sentinel"""
    x = np.atleast_2d(np.asarray(x, dtype))
    rows, cols = x.shape
    flat = np.full(rows * ld + GUARD, sentinel, dtype)
    flat[:rows * ld].reshape(rows, ld)[:, :cols] = x
    return torch.from_numpy(flat).cuda()


def blank(rows, cols, ld, sentinel, dtype):
    return torch.from_numpy(np.full(rows * ld + GUARD, sentinel, dtype)).cuda()


def take(t, rows, cols, ld):
    """-> (the [rows, cols] payload, everything else in the buffer)"""
    a = t.cpu().numpy()
    body = a[:rows * ld].reshape(rows, ld)
    return body[:, :cols].copy(), np.concatenate([body[:, cols:].ravel(), a[rows * ld:]])


def untouched(rest, sentinel, dtype):
    want = np.full(rest.shape, sentinel, dtype)
    return np.array_equal(rest.view(np.uint8), want.view(np.uint8))


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,))
    bad = bad.any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.size} elements differ; first at {np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, want {want[bad][0]!r}"


def sparsify_raw(t, rows, cols, ld, relu, log1p, round_bf16, top_k, min_keep):
    L = _lib()
    L.check(L.lib().lrx_sparsify(L.ptr(t), rows, cols, ld, int(relu), int(log1p), int(round_bf16), int(top_k), int(min_keep), L.current_stream()))


# ---------------------------------------------------------------------------------------------------------------
# threshold select
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", SR.THRESHOLD_COLS)
def test_threshold_select(cols):
    """relu = log1p = 0: the k-th largest value by a 4-pass radix select, everything strictly below it becomes +0.0, survivors (ties with the
    k-th, -0.0, denormals, infinities) keep their bits; row padding keeps the sentinel."""
    for top_k, min_keep in SR.threshold_calls(cols):
        k = SR.effective_k(top_k, min_keep, cols)
        for name, x in SR.threshold_matrices(cols, k).items():
            want = SR.topk_threshold(x, k)
            for ld in (cols, cols + SR.PAD):
                t = put(x, ld, SR.PAD_SENTINEL, np.float32)
                sparsify_raw(t, x.shape[0], cols, ld, 0, 0, 0, top_k, min_keep)
                got, rest = take(t, x.shape[0], cols, ld)
                what = f"cols={cols} top_k={top_k} min_keep={min_keep} {name} ld={ld}"
                same_bits(got, want, what)
                assert untouched(rest, SR.PAD_SENTINEL, np.float32), what
    # top_k = 0: no selection at all
    x = SR.threshold_matrices(cols, 1)["edge"]
    t = put(x, cols + SR.PAD, SR.PAD_SENTINEL, np.float32)
    sparsify_raw(t, x.shape[0], cols, cols + SR.PAD, 0, 0, 0, 0, 8)
    got, rest = take(t, x.shape[0], cols, cols + SR.PAD)
    same_bits(got, x)
    assert untouched(rest, SR.PAD_SENTINEL, np.float32)


# ---------------------------------------------------------------------------------------------------------------
# transform
# ---------------------------------------------------------------------------------------------------------------
def test_relu_alone_is_exact():
    """compared by value: the sign of a zero coming out of fmaxf(-0.0, 0.0) is not specified"""
    for cols in (7, 257, 1025):
        x = np.concatenate([SR.threshold_matrices(cols, 2)[n] for n in ("edge", "radix0", "random")])
        for ld in (cols, cols + SR.PAD):
            t = put(x, ld, SR.PAD_SENTINEL, np.float32)
            sparsify_raw(t, x.shape[0], cols, ld, 1, 0, 0, 0, 8)
            got, rest = take(t, x.shape[0], cols, ld)
            np.testing.assert_array_equal(got, np.maximum(x, np.float32(0)))
            assert untouched(rest, SR.PAD_SENTINEL, np.float32)
            same_bits(got[x > 0], x[x > 0])                                  # the positive denormals among them


def test_log1pf_alone(capsys):
    """relu = 1, log1p = 1, round_bf16 = 0 is log1pf alone.  The figure the budget doubles: the largest error against float64, in fp32 ulps of
    the float64 result, over every positive bf16 argument and 2^18 random fp32 arguments in [2^-30, 2^30]."""
    from lightretriever_amd import ops
    a = SR.log1pf_arguments()
    assert a.size % 3 == 0
    got = ops.sparsify_(torch.from_numpy(a.reshape(3, -1).copy()).cuda(), True, True, False, 0, 8).cpu().numpy().ravel()
    err = SR.log1pf_error_ulp(got, a)
    n16 = SR.N_POSITIVE_BF16
    i = int(np.argmax(err))
    with capsys.disabled():
        print("\nlog1pf: largest error %.4f ulp (bf16 arguments %.4f, random fp32 %.4f) at x = %r; sparse_reference has %.4f, budget %g"
              % (err.max(), err[:n16].max(), err[n16:].max(), float(a[i]), SR.LOG1PF_MEASURED_ULP, SR.BUDGET_ULP))
    path = os.environ.get("LRX_SPARSE_PROFILE")
    if path:
        with open(path, "w") as f:
            f.write(json.dumps(dict(kernel="log1pf", n=int(a.size), max_ulp=float(err.max()), max_ulp_bf16=float(err[:n16].max()), at=float(a[i]))) + "\n")
    assert err.max() <= SR.LOG1PF_MEASURED_ULP
    assert SR.BUDGET_ULP == np.ceil(2 * SR.LOG1PF_MEASURED_ULP) and SR.BUDGET_ULP <= SR.MIDPOINT_CLEAR_ULP


def test_unrounded_log1p_within_the_budget():
    from lightretriever_amd import ops
    x = SR.exhaustive_bf16()
    want, y64 = SR.sparsify(x, True, True, False)
    for ld in (x.shape[1], x.shape[1] + SR.PAD):
        t = put(x, ld, SR.PAD_SENTINEL, np.float32)
        sparsify_raw(t, x.shape[0], x.shape[1], ld, 1, 1, 0, 0, 8)
        got, rest = take(t, *x.shape, ld)
        assert untouched(rest, SR.PAD_SENTINEL, np.float32)
        err = np.abs(got.astype(np.float64) - y64) / SR.ulp32(y64)
        assert (err <= SR.BUDGET_ULP).all(), (float(err.max()), float(x.ravel()[np.argmax(err)]))
        same_bits(got[x <= 0], np.zeros(2, np.float32))                      # log1p(0) == +0.0 exactly; BF16_MIN gives 0 behind relu
    edge = ops.sparsify_(torch.tensor([[0.0, float(SR.BF16_MIN), float("inf"), -0.0, -1.0]], device="cuda"), True, True, False, 0, 8).cpu().numpy()
    assert edge.tolist() == [[0.0, 0.0, np.inf, 0.0, 0.0]]


def test_rounded_log1p_exhaustive():
    """round_bf16 = 1 over every positive bf16 argument: each output is a bf16 number and equals bf16_rne(fp32(log1p64(x))) bit for bit --
    nothing is excluded (no result lies within 4 ulp of a rounding midpoint: test_sparse_reference_host.py)."""
    x = SR.exhaustive_bf16()
    assert x.shape[1] % 1024 != 0
    want = SR.sparsify(x, True, True, True)[0]
    for ld in (x.shape[1], x.shape[1] + SR.PAD):
        t = put(x, ld, SR.PAD_SENTINEL, np.float32)
        sparsify_raw(t, x.shape[0], x.shape[1], ld, 1, 1, 1, 0, 8)
        got, rest = take(t, *x.shape, ld)
        assert (SR.bits(got) & 0xFFFF == 0).all()
        same_bits(got, want, f"ld={ld}")
        assert untouched(rest, SR.PAD_SENTINEL, np.float32)


def _compaction_forms(reps, q):
    """the capacity form and the CSR form of the same rows: -> (ids rows, weight rows, counts), asserted equal to each other"""
    from lightretriever_amd import ops
    ids, w, cnt = (t.cpu().numpy() for t in ops.sparse_compact(reps, q))
    rows = ops.sparse_compact_csr(reps, q, empty_marker=False).to("cpu")
    off = rows.row_off.numpy()
    np.testing.assert_array_equal(off[1:] - off[:-1], cnt)
    out_i, out_w = [], []
    for b in range(len(cnt)):
        out_i.append(ids[b, :cnt[b]])
        out_w.append(w[b, :cnt[b]])
        np.testing.assert_array_equal(rows.terms.numpy()[off[b]:off[b + 1]], out_i[-1])
        np.testing.assert_array_equal(rows.weights.numpy()[off[b]:off[b + 1]], out_w[-1])
    return out_i, out_w, cnt


@pytest.mark.parametrize("top_k", [16, 0])
def test_production_chain_is_exact(top_k):
    """sparsify_(relu, log1p, round_bf16, top_k) -> sparse_compact(q = 100) and sparse_compact_csr(q = 100) on the exhaustive input: values,
    terms, weights and counts equal the reference exactly, and the two compaction forms agree."""
    from lightretriever_amd import ops
    x = SR.exhaustive_bf16()
    want = SR.sparsify(x, True, True, True, top_k, 8)[0]
    reps = ops.sparsify_(torch.from_numpy(x.copy()).cuda(), True, True, True, top_k, 8)
    same_bits(reps.cpu().numpy(), want)
    if top_k:
        assert ((want != 0).sum(1) >= 16).all() and ((want != 0).sum(1) < 200).all()
    got_i, got_w, cnt = _compaction_forms(reps, SR.Q_PRODUCTION)
    want_i, want_w, want_cnt = SR.compact(want, SR.Q_PRODUCTION)
    np.testing.assert_array_equal(cnt, want_cnt)
    for b in range(len(cnt)):
        np.testing.assert_array_equal(got_i[b], want_i[b])
        np.testing.assert_array_equal(got_w[b], want_w[b])


def test_unrounded_chain_is_exact_away_from_the_halves():
    """round_bf16 = 0, q = 100: the quantised weights equal the reference's except where float64 log1p(x) * q lies within the budget of a
    half-integer (there either neighbour); the share left out is asserted."""
    from lightretriever_amd import ops
    x = SR.exhaustive_bf16()
    want, y64 = SR.sparsify(x, True, True, False)
    near = SR.near_half(y64, SR.Q_PRODUCTION)
    share = float(near.mean())
    print("unrounded chain: %d of %d elements left out (%.3f %%)" % (near.sum(), near.size, 100 * share))
    assert share <= SR.NEAR_HALF_CAP
    reps = ops.sparsify_(torch.from_numpy(x.copy()).cuda(), True, True, False, 0, 8)
    got_i, got_w, cnt = _compaction_forms(reps, SR.Q_PRODUCTION)
    dense = np.zeros(x.shape, np.int64)
    for b in range(len(cnt)):
        assert (np.diff(got_i[b]) > 0).all()
        dense[b, got_i[b]] = got_w[b]
    wq = SR.quantise(want, SR.Q_PRODUCTION)
    np.testing.assert_array_equal(dense[~near], wq[~near])
    assert (np.abs(dense[near] - wq[near]) <= 1).all()


# ---------------------------------------------------------------------------------------------------------------
# capacity compaction
# ---------------------------------------------------------------------------------------------------------------
def compact_raw(x, ld, q, capacity):
    """lrx_sparse_compact on rows at stride ld with sentinel-filled outputs -> (ids [B, cap], weights [B, cap], counts [B]); asserts that the
    guard stretches behind the three outputs are intact"""
    L = _lib()
    B, cols = x.shape
    t = put(x, ld, SR.COMPACT_PAD_VALUE, np.float32)
    ids, w = blank(B, capacity, capacity, SR.OUT_SENTINEL, np.int32), blank(B, capacity, capacity, SR.OUT_SENTINEL, np.int32)
    cnt = blank(1, B, B, SR.OUT_SENTINEL, np.int32)
    L.check(L.lib().lrx_sparse_compact(L.ptr(t), B, cols, ld, q, capacity, L.ptr(ids), L.ptr(w), L.ptr(cnt), L.current_stream()))
    (gi, ri), (gw, rw), (gc, rc) = take(ids, B, capacity, capacity), take(w, B, capacity, capacity), take(cnt, 1, B, B)
    assert untouched(ri, SR.OUT_SENTINEL, np.int32) and untouched(rw, SR.OUT_SENTINEL, np.int32) and untouched(rc, SR.OUT_SENTINEL, np.int32), \
        f"cols={cols} ld={ld} capacity={capacity}: written behind an output"
    _, rest = take(t, B, cols, ld)
    assert untouched(rest, SR.COMPACT_PAD_VALUE, np.float32)
    return gi, gw, gc[0]


def check_compact(x, q, capacity, ld):
    gi, gw, gc = compact_raw(x, ld, q, capacity)
    want_i, want_w, want_c = SR.compact(x, q, capacity)
    what = f"cols={x.shape[1]} ld={ld} q={q} capacity={capacity}"
    np.testing.assert_array_equal(gc, want_c, err_msg=what)                  # the true number, whatever the capacity
    for b in range(x.shape[0]):
        n = min(int(want_c[b]), capacity)
        np.testing.assert_array_equal(gi[b, :n], want_i[b], err_msg=what)
        np.testing.assert_array_equal(gw[b, :n], want_w[b], err_msg=what)
        assert (np.diff(gi[b, :n]) > 0).all()
        assert (gi[b, n:] == SR.OUT_SENTINEL).all() and (gw[b, n:] == SR.OUT_SENTINEL).all(), f"{what} row {b}: a slot beyond min(count, capacity) was written"


@pytest.mark.parametrize("cols", SR.COMPACT_COLS)
def test_capacity_compaction(cols):
    x = SR.compact_rows(cols)
    for capacity in SR.compact_capacities(cols):
        for ld in (cols, cols + SR.PAD):
            check_compact(x, SR.Q_PRODUCTION, capacity, ld)


def test_compaction_of_exact_products():
    """q = 64: halves round to even, the largest product below 2^31 converts exactly, NaN gives no entry"""
    x = SR.exact_rows()
    for capacity in (1, 63, 64, 65, 66, 70):
        check_compact(x, SR.Q_EXACT, capacity, x.shape[1] + SR.PAD)
    gi, gw, gc = compact_raw(x, x.shape[1], SR.Q_EXACT, 70)
    got = dict(zip(gi[0, :gc[0]].tolist(), gw[0, :gc[0]].tolist()))
    assert got[67] == int(SR.MAX_PRODUCT) and got[1] == 2 and got[2] == 2 and got[3] == 4 and 0 not in got and 65 not in got and gc.tolist() == [65, 0]


# ---------------------------------------------------------------------------------------------------------------
# fusion
# ---------------------------------------------------------------------------------------------------------------
def contributions_raw(sc, ids, method, p0, p1, pad):
    L = _lib()
    Q, k = ids.shape
    ld = k + pad
    ts, ti = put(sc, ld, SR.SCORE_PAD_SENTINEL, np.float64), put(ids, ld, SR.ID_PAD_SENTINEL, np.int64)
    ldc = k + (2 * pad if pad else 0)                                        # the contributions' stride is a parameter of its own
    out = blank(Q, k, ldc, SR.OUT_F64_SENTINEL, np.float64)
    L.check(L.lib().lrx_hit_contributions(L.ptr(ts), L.ptr(ti), Q, k, ld, 0 if method == "rrf" else 1, float(p0), float(p1), L.ptr(out), ldc, L.current_stream()))
    got, rest = take(out, Q, k, ldc)
    assert untouched(rest, SR.OUT_F64_SENTINEL, np.float64), "contributions written outside their rows"
    return got


def union_raw(ids_cat, con_cat, pad):
    L = _lib()
    Q, n = ids_cat.shape
    ld = n + pad
    ti, tc = put(ids_cat, ld, SR.ID_PAD_SENTINEL, np.int64), put(con_cat, ld, SR.SCORE_PAD_SENTINEL, np.float64)
    out_s, out_i = blank(Q, n, ld, SR.OUT_F64_SENTINEL, np.float64), blank(Q, n, ld, SR.OUT_I64_SENTINEL, np.int64)
    cnt = blank(1, Q, Q, SR.OUT_SENTINEL, np.int32)
    L.check(L.lib().lrx_hit_union(L.ptr(ti), L.ptr(tc), Q, n, ld, L.ptr(out_s), L.ptr(out_i), L.ptr(cnt), L.current_stream()))
    (gs, rs), (gi, ri), (gc, rc) = take(out_s, Q, n, ld), take(out_i, Q, n, ld), take(cnt, 1, Q, Q)
    assert untouched(rs, SR.OUT_F64_SENTINEL, np.float64) and untouched(ri, SR.OUT_I64_SENTINEL, np.int64) and untouched(rc, SR.OUT_SENTINEL, np.int32), \
        "the union wrote outside its rows"
    return gs, gi, gc[0]


def check_union(got, want, what):
    (gs, gi, gc), (ws, wi, wc) = got, want
    np.testing.assert_array_equal(gc, wc, err_msg=what)
    np.testing.assert_array_equal(gi, wi, err_msg=what)                      # order (score descending, lower id first) and -1 padding
    same_bits(gs, ws, what)                                                  # float64 sums bit for bit, -inf padding


@pytest.mark.parametrize("case", SR.fusion_cases(), ids=lambda c: c["name"])
def test_fusion(case):
    from lightretriever_amd.score_fuse_utils import fuse_hits
    systems = case["systems"]
    for method in ("rrf", "linear"):
        want_con, want = SR.fuse(systems, method, rrf_k=case["rrf_k"], weights=case["weights"], eps=case["eps"])
        for pad in (0, SR.FUSE_PAD):
            con = []
            for j, (sc, ids) in enumerate(systems):
                p0, p1 = (case["rrf_k"], 0.0) if method == "rrf" else (case["weights"][j], case["eps"])
                con.append(contributions_raw(sc, ids, method, p0, p1, pad))
                same_bits(con[-1], want_con[j], f"{case['name']} {method} system {j} pad={pad}")
            got = union_raw(np.concatenate([i for _, i in systems], 1), np.concatenate(con, 1), pad)
            check_union(got, want, f"{case['name']} {method} pad={pad}")
        # the array form the searchers call
        sc, ids, cnt = fuse_hits([(torch.from_numpy(s).cuda(), torch.from_numpy(i).cuda()) for s, i in systems], method=method, k=case["rrf_k"],
                                 weights=case["weights"], eps=case["eps"])
        check_union((sc.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().numpy()), want, f"{case['name']} {method} fuse_hits")


@pytest.mark.parametrize("case", SR.union_cases(), ids=lambda c: c[0])
def test_union(case):
    name, ids, con = case
    want = SR.union(ids, con)
    for pad in (0, SR.FUSE_PAD):
        check_union(union_raw(ids, con, pad), want, f"{name} pad={pad}")
