"""Host proof of tests/sparse_reference.py, the yardstick of tests/test_gpu_sparse_reference.py: the restatement agrees with what the project
already trusts (oracle.lrx_oracle, the reference project's goldens), and the inputs of the GPU tests have the properties they claim -- no
log1p result of a bf16 argument near a bf16 rounding midpoint, a capped share of quantisation products near a half, radix rows that reach the
bucket they name in every pass, a union case whose sum depends on the order.  No GPU."""
import json
import os

import numpy as np
import pytest

import sparse_reference as SR
from helpers import GOLDEN
from oracle import lrx_oracle as O


def same_bits(a, b):
    np.testing.assert_array_equal(SR.bits(a), SR.bits(b))


# ---------------------------------------------------------------------------------------------------------------
# number formats, key map
# ---------------------------------------------------------------------------------------------------------------
def test_bf16_rounding_and_key_map():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(5000).astype(np.float32) * 100, SR.SPECIALS, SR.positive_bf16()[::37]])
    same_bits(SR.bf16_rne(x), O.round_bf16(x))
    assert SR.positive_bf16().size == SR.N_POSITIVE_BF16 and np.isfinite(SR.positive_bf16()).all() and (SR.positive_bf16() > 0).all()
    # the key order is the value order, with -0.0 just below +0.0; the map is a bijection
    k = SR.f32_key(x)
    order = np.argsort(k, kind="stable")
    assert (np.diff(x[order].astype(np.float64)) >= 0).all()
    same_bits(SR.key_f32(k), x)
    assert SR.f32_key(np.float32(-0.0)) == 0x7FFFFFFF and SR.f32_key(np.float32(0.0)) == 0x80000000
    assert SR.ulp32(1.0) == 2.0 ** -23 and SR.ulp32(0.75) == 2.0 ** -24 and SR.ulp32(1e-45) == 2.0 ** -149


# ---------------------------------------------------------------------------------------------------------------
# oracle agreement: selection, transform, quantisation, compaction
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", SR.THRESHOLD_COLS)
def test_threshold_agrees_with_the_oracle(cols):
    for top_k, min_keep in SR.threshold_calls(cols):
        k = SR.effective_k(top_k, min_keep, cols)
        for name, x in SR.threshold_matrices(cols, k).items():
            assert x.shape == (SR.THRESHOLD_ROWS, cols) and not np.isnan(x).any(), name
            want = SR.topk_threshold(x, k)
            same_bits(want, O.top_k_sampling(x, top_k, min_tokens_to_keep=min_keep))
            same_bits(want, O.sparsify(x, relu=False, log1p=False, top_k=top_k, min_tokens_to_keep=min_keep))
            same_bits(want, SR.sparsify(x, False, False, False, top_k, min_keep)[0])
            kept = SR.bits(want) == SR.bits(x)
            assert (SR.bits(want)[~kept] == 0).all()                         # everything filtered is +0.0
            # the radix walk finds the same threshold as the sort, row by row
            for r in range(x.shape[0]):
                _, thr = SR.radix_trace(x[r], k)
                assert thr == np.sort(x[r])[::-1][k - 1], (name, r)
                same_bits(np.where(x[r] < thr, np.float32(0), x[r]), want[r])


def test_threshold_rows_are_what_they_claim():
    for cols in SR.THRESHOLD_COLS:
        for top_k, min_keep in SR.threshold_calls(cols):
            k = SR.effective_k(top_k, min_keep, cols)
            rng = np.random.default_rng(1)
            row, m, g = SR.tie_row(cols, k, rng)
            want = SR.topk_threshold(row, k)[0]
            assert (row == 1.5).sum() == m and (want == 1.5).sum() == m and (want != 0).sum() == g + m     # all m ties survive
            assert g < k <= g + m
            if cols >= k + 3:
                assert g + m > k                                                                       # ... and they straddle k
            z = SR.zero_threshold_row(cols, k, rng)
            wz = SR.topk_threshold(z, k)[0]
            assert np.sort(z)[::-1][k - 1] == 0
            neg_den = SR.bits(z) == SR.bits(-SR.DENORM)
            if cols > k + 1:
                assert neg_den.any()
            assert (SR.bits(wz)[neg_den] == 0).all()                                                   # the denormal below zero is filtered
            assert (SR.bits(wz)[z >= 0] == SR.bits(z)[z >= 0]).all()                                   # -0.0 and +1.4e-45 keep their bits
            edge = SR.threshold_matrices(cols, k)["edge"]
            assert (edge[0] == -1).all() and (edge[1] == SR.BF16_MIN).all()
            same_bits(SR.topk_threshold(edge[:2], k), edge[:2])                                        # all equal: everything survives


def test_radix_rows_reach_the_buckets_they_name(capsys):
    lines = []
    for cols in SR.THRESHOLD_COLS:
        for top_k, min_keep in SR.threshold_calls(cols):
            k = SR.effective_k(top_k, min_keep, cols)
            mats = SR.threshold_matrices(cols, k)
            for bucket, name in ((0, "radix0"), (255, "radix255")):
                for d in range(4):
                    row = mats[name][d]
                    keys = SR.f32_key(row)
                    others = keys & ~np.uint32(0xFF << (24 - 8 * d))
                    assert (others == others[0]).all()                       # the keys differ in byte d only
                    trace, _ = SR.radix_trace(row, k)
                    assert trace[d] == bucket, (cols, k, d, trace)
                    if bucket == 255 and cols > k:
                        assert ((keys >> np.uint32(24 - 8 * d)) & 255 == 255).sum() == k + 1          # ties straddle k
                    lines.append(f"cols={cols} k={k} digit={d} bucket={bucket}: trace {trace}")
            t_neg, v_neg = SR.radix_trace(mats["radix0"][4], k)
            t_pos, v_pos = SR.radix_trace(mats["radix255"][4], k)
            assert t_neg[0] == 0x7F and v_neg < 0 and t_pos[0] == 0x80 and v_pos > 0                   # the two sides of the sign flip
            lines.append(f"cols={cols} k={k} sign flip: traces {t_neg} {t_pos}")
    # every digit sees bucket 0 and bucket 255 at every width
    assert len(lines) == sum(len(SR.threshold_calls(c)) for c in SR.THRESHOLD_COLS) * 9
    with capsys.disabled():
        print("\nradix traces (%d); a sample:" % len(lines))
        print("\n".join(lines[i] for i in (0, 4, 8, len(lines) // 2, len(lines) - 2, len(lines) - 1)))


def test_transform_agrees_with_the_oracle():
    x = SR.exhaustive_bf16()
    assert x.shape == SR.EXHAUSTIVE_SHAPE and x.shape[1] % 1024 != 0
    assert np.array_equal(np.sort(x.ravel())[2:], SR.positive_bf16())        # every positive bf16 number, once
    # relu alone, and log1p: the oracle takes it in fp32 (numpy's log1pf), the reference in float64 rounded once
    np.testing.assert_array_equal(SR.sparsify(x, True, False, False)[0], O.sparsify(x, relu=True, log1p=False, top_k=0))
    got, y64 = SR.sparsify(x, True, True, False)
    err = np.abs(O.sparsify(x, relu=True, log1p=True, top_k=0).astype(np.float64) - y64) / SR.ulp32(y64)
    assert np.abs(got.astype(np.float64) - y64).max() <= 0.5 * SR.ulp32(y64).max() and (np.abs(got - y64) <= 0.5 * SR.ulp32(y64)).all()
    assert err.max() <= SR.MIDPOINT_CLEAR_ULP
    # ... so on the rounded path, where nothing is within 4 ulp of a midpoint, the two agree bit for bit, selection included
    for top_k in (0, 16):
        same_bits(SR.sparsify(x, True, True, True, top_k, 8)[0], O.sparsify(x, relu=True, log1p=True, top_k=top_k, min_tokens_to_keep=8, bf16=True))
    r = SR.sparsify(x, True, True, True)[0]
    assert (SR.bits(r) & 0xFFFF == 0).all()
    assert SR.sparsify(np.float32([[0.0, SR.BF16_MIN, np.inf]]), True, True, False)[0].tolist() == [[0.0, 0.0, np.inf]]
    # numpy's own fp32 log1p on the arguments the device figure is measured over (for orientation)
    a = SR.log1pf_arguments()
    assert a.size == SR.N_POSITIVE_BF16 + (1 << 18) and a.min() > 0 and np.isfinite(a).all()
    print("numpy fp32 log1p: largest error %.3f ulp over the measured arguments" % SR.log1pf_error_ulp(np.log1p(a), a).max())


def test_quantise_and_compact_agree_with_the_oracle_and_the_goldens():
    for cols in SR.COMPACT_COLS:
        x = SR.compact_rows(cols)
        for q in (SR.Q_PRODUCTION, SR.Q_EXACT, 7):
            np.testing.assert_array_equal(SR.quantise(x, q), O.quantize_sparse(x, q))
        ids, w, cnt = SR.compact(x, SR.Q_PRODUCTION)
        assert cnt[0] == cols and cnt[1] == 0 and cnt[2] == min(2, cols) and cnt[3] >= 1
        assert [{str(i): int(v) for i, v in zip(a, b)} or {"-1": 1} for a, b in zip(ids, w)] == O.sparse_reps_to_json(x, SR.Q_PRODUCTION)
        caps = SR.compact_capacities(cols)
        assert {37, 64, 1024} <= set(caps) and all({c for c in (int(n) - 1, int(n), int(n) + 1) if c >= 1} <= set(caps) for n in cnt)
        ids2, w2, cnt2 = SR.compact(x, SR.Q_PRODUCTION, capacity=caps[0])
        assert (cnt2 == cnt).all() and all(len(a) == min(n, caps[0]) for a, n in zip(ids2, cnt))     # counts stay the true number
    for x in (SR.sparsify(SR.exhaustive_bf16(), True, True, rb, tk, 8)[0] for rb in (True, False) for tk in (0, 16)):
        np.testing.assert_array_equal(SR.quantise(x, SR.Q_PRODUCTION), O.quantize_sparse(x, SR.Q_PRODUCTION))
    # the exact rows: half to even on exact products, the largest product below 2^31, NaN gives no entry
    ids, w, cnt = SR.compact(SR.exact_rows(), SR.Q_EXACT)
    half_even = [int(np.rint(n + 0.5)) for n in range(64)]
    assert half_even[:4] == [0, 2, 2, 4]
    want = {n: v for n, v in enumerate(half_even) if v} | {67: int(SR.MAX_PRODUCT), 69: 64}
    assert dict(zip(ids[0].tolist(), w[0].tolist())) == want and cnt.tolist() == [len(want), 0]
    # the reference project's converter
    g = np.load(os.path.join(GOLDEN, "sparse.npz"))
    with open(os.path.join(GOLDEN, "sparse_json.json")) as f:
        gold = json.load(f)
    for key, jkey in (("sparse_reps", "quant100"), ("sparse_reps_top16", "quant100_top16")):
        ids, w, cnt = SR.compact(g[key], 100)
        assert [{str(i): int(v) for i, v in zip(a, b)} or {"-1": 1} for a, b in zip(ids, w)] == gold[jkey]
    halves = np.array([[0.5 / 7, 1.5 / 7, 2.5 / 7, -3.0, 0.0, 0.07]], np.float32)
    ids, w, cnt = SR.compact(halves, 7, capacity=2)
    assert int(cnt[0]) == len(gold["quant7_halves"][0]) and [(str(i), int(v)) for i, v in zip(ids[0], w[0])] == list(gold["quant7_halves"][0].items())[:2]


# ---------------------------------------------------------------------------------------------------------------
# the two conditions of the log1p tests
# ---------------------------------------------------------------------------------------------------------------
def test_no_bf16_log1p_result_is_near_a_rounding_midpoint(capsys):
    """The condition that lets the GPU test of the rounded path leave nothing out."""
    x = SR.positive_bf16()
    y64 = np.log1p(x.astype(np.float64))
    dist = np.minimum(SR.midpoint_distance_ulp(y64), SR.midpoint_distance_ulp(y64.astype(np.float32)))
    # the same distance read off the fp32 bit pattern
    low = (SR.bits(y64.astype(np.float32)) & 0xFFFF).astype(np.int64)
    assert np.abs(np.abs(low - 0x8000) - SR.midpoint_distance_ulp(y64.astype(np.float32))).max() == 0
    near = int((dist <= SR.MIDPOINT_CLEAR_ULP).sum())
    i = int(np.argmin(dist))
    with capsys.disabled():
        print("\nbf16 arguments: %d; within %g ulp of a midpoint: %d; nearest: %.2f ulp at x = %r" % (x.size, SR.MIDPOINT_CLEAR_ULP, near, dist[i], float(x[i])))
    assert x.size == SR.N_POSITIVE_BF16 == 32639 and near == 0
    assert SR.BUDGET_ULP <= SR.MIDPOINT_CLEAR_ULP and SR.BUDGET_ULP == np.ceil(2 * SR.LOG1PF_MEASURED_ULP)


def test_near_half_share_is_capped(capsys):
    cases = list(SR.near_half_cases())
    assert cases
    for name, near, q in cases:
        share = near.mean()
        with capsys.disabled():
            print("\n%s: %d of %d elements within %g ulp of a half (%.3f %%), cap %.1f %%" % (name, near.sum(), near.size, SR.BUDGET_ULP, 100 * share, 100 * SR.NEAR_HALF_CAP))
        assert share <= SR.NEAR_HALF_CAP
        wide = SR.near_half(SR.sparsify(SR.exhaustive_bf16(), True, True, False)[1], q, SR.MIDPOINT_CLEAR_ULP)
        assert wide.mean() <= SR.NEAR_HALF_CAP and (wide | ~near).all()      # within the cap even at the largest budget allowed


# ---------------------------------------------------------------------------------------------------------------
# fusion
# ---------------------------------------------------------------------------------------------------------------
def test_fusion_reproduces_the_reference_goldens():
    with open(os.path.join(GOLDEN, "fusion.json")) as f:
        g = json.load(f)
    two, three = [g["dense"], g["sparse"]], [g["dense"], g["sparse"], g["third"]]

    def run(lists, method, **kw):
        qn, pn, systems = SR.dicts_to_systems(lists)
        _, (sc, ids, cnt) = SR.fuse(systems, method, **kw)
        return SR.fused_to_dicts(sc, ids, cnt, qn, pn)
    assert run(two, "rrf") == g["rrf"]
    assert run(two, "rrf", rrf_k=10) == g["rrf_k10"]
    assert run(three, "rrf") == g["rrf_three"]
    assert run(two, "linear", weights=[0.7, 0.3]) == g["linear"]
    assert run(two, "linear", weights=[0.5, 0.5], eps=1e-6) == g["linear_5050"]
    assert run(three, "linear", weights=[0.5, 0.3, 0.2]) == g["linear_three"]


def test_dict_conversion_is_the_products():
    from lightretriever_amd.score_fuse_utils import _dicts_to_arrays
    with open(os.path.join(GOLDEN, "fusion.json")) as f:
        g = json.load(f)
    lists = [g["dense"], g["sparse"], g["third"]]
    qn, pn, systems = SR.dicts_to_systems(lists)
    qn2, pn2, systems2 = _dicts_to_arrays(lists)
    assert qn == qn2 and pn == pn2
    for (s, i), (s2, i2) in zip(systems, systems2):
        assert np.array_equal(s, s2.numpy()) and np.array_equal(i, i2.numpy())


@pytest.mark.parametrize("case", SR.fusion_cases(), ids=lambda c: c["name"])
def test_fusion_agrees_with_the_oracle(case):
    systems = case["systems"]
    for sc, ids in systems:
        for row in ids:
            v = row[row >= 0]
            assert np.unique(v).size == v.size                               # unique within a list
    dicts = SR.systems_to_dicts(systems)
    for method in ("rrf", "linear"):
        con, (sc, ids, cnt) = SR.fuse(systems, method, rrf_k=case["rrf_k"], weights=case["weights"], eps=case["eps"])
        want = O.fuse_scores_rrf(dicts, k=case["rrf_k"]) if method == "rrf" else O.fuse_scores_linear(dicts, case["weights"], eps=case["eps"])
        got = SR.fused_to_dicts(sc, ids, cnt)
        assert got.keys() == want.keys()
        for q in want:
            assert got[q].keys() == want[q].keys()
            assert [np.float64(got[q][p]).view(np.int64) for p in want[q]] == [np.float64(want[q][p]).view(np.int64) for p in want[q]]    # bit for bit
        n = sum(i.shape[1] for _, i in systems)
        assert sc.shape == ids.shape == (len(cnt), n)
        for q in range(len(cnt)):
            c = int(cnt[q])
            assert (ids[q, c:] == -1).all() and np.isneginf(sc[q, c:]).all() and (np.diff(sc[q, :c]) <= 0).all()
            t = np.flatnonzero(np.diff(sc[q, :c]) == 0)
            assert (ids[q, t] < ids[q, t + 1]).all()
        for (s, i), c in zip(systems, con):
            assert (c[i < 0] == 0).all()


def test_fusion_cases_cover_what_they_claim():
    cases = SR.fusion_cases()
    ks = {i.shape[1] for c in cases for _, i in c["systems"]}
    totals = {sum(i.shape[1] for _, i in c["systems"]) for c in cases}
    assert {1, 2, 3, 63, 64, 65, 1000, 1024, 2048, 4096} <= ks and {1, 2, 5, 4095, 4096} <= totals
    assert {len(c["systems"]) for c in cases} == {1, 2, 3, 4} and {len(c["systems"][0][1]) for c in cases} == {1, 3}
    assert any([i.shape[1] for _, i in c["systems"]] == [1024] * 4 for c in cases)
    all_ids = np.concatenate([i.ravel() for c in cases for _, i in c["systems"]])
    assert ((all_ids > 2 ** 32) & (all_ids < 2 ** 33)).any() and (all_ids > 2 ** 62 - 20000).any()
    # ties: some list has a run of more than 50 equal scores; holes: a valid slot after an empty one; a list without a valid slot
    runs, interior, empty = 0, False, False
    for c in cases:
        for s, i in c["systems"]:
            for q in range(len(i)):
                v = i[q] >= 0
                runs = max(runs, int(np.unique(s[q][v], return_counts=True)[1].max()) if v.any() else 0)
                interior |= bool(v.any() and (~v[:np.flatnonzero(v)[-1]]).any())
                empty |= not v.any()
    assert runs > 50 and interior and empty
    # RRF really depends on the tie-break: ranking equal scores later-position-first changes a contribution
    s, i = np.array([[2.0, 2.0, 1.0]]), np.array([[7, 8, 9]])
    assert SR.contributions(s, i, "rrf", 60).tolist() == [[1 / 61, 1 / 62, 1 / 63]]
    edges = [c for c in cases if c["name"].startswith("linear edges")]
    assert sorted(c["eps"] for c in edges) == [1e-8, 1e-6] and all(c["weights"][3] == 0.0 for c in edges)
    con = SR.contributions(*edges[0]["systems"][0], "linear", 0.5, 1e-8)
    assert (con == 0).all()                                                  # all equal / one valid slot / none: den = eps, numerator 0


def test_union_cases_depend_on_the_order_of_the_sum():
    name, ids, con = SR.union_cases()[0]
    assert name == "order"
    a, b, c, d = (np.float64(v) for v in SR.ORDER_CONTRIB)
    in_order, other = ((np.float64(0.0) + a) + b + c) + d, ((np.float64(0.0) + a) + c + b) + d
    assert in_order == 1.0 and other == 2.0 and in_order != other            # otherwise the case proves nothing
    sc, out, cnt = SR.union(ids, con)
    assert (ids > 2 ** 32).any() and (ids > 2 ** 62 - 10000).any() and (ids == -1).any()
    for q in range(3):
        shared = np.isin(out[q, :cnt[q]], ids[q][con[q] == 1e16])
        assert shared.sum() == 40 and (sc[q, :cnt[q]][shared] == 1.0).all() and cnt[q] == 40 + 4 * 10
    name, ids, con = SR.union_cases()[1]
    sc, out, cnt = SR.union(ids, con)
    assert out[0, :5].tolist() == [1, 3, 5, 8, 2 ** 40] and (sc[0, :5] == 0.5).all() and cnt.tolist() == [5, 0, 2]
    assert out[2, :2].tolist() == [2, 4] and sc[2, :2].tolist() == [1.0, 1.0] and (out[1] == -1).all() and np.isneginf(sc[1]).all()
