"""The host model of the shared top-k selection (select_reference.py) against itself, and the preconditions of every case of
test_gpu_select_paths.py on the model alone: each case lands on the branch its table entry names, the cases together cover every branch,
each harness reproduces its intended score row through the index's own yardstick bit for bit, the band of the rescoring selects stays inside
one level, and every case with ties would catch a wrong tie rule.  No GPU."""
import os
import re

import numpy as np
import pytest

import pq_yardstick
import select_reference as R
import sq8_yardstick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lightretriever_amd", "csrc")
_ROWS = {}


def rows_of(case):
    if case["name"] not in _ROWS:
        _ROWS[case["name"]] = R.case_rows(case)
    return _ROWS[case["name"]]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def define(header, name):
    m = re.search(rf"^#define {name} (\d+)\b", open(os.path.join(CSRC, header)).read(), re.M)
    assert m, f"{header}: no #define {name}"
    return int(m.group(1))


def test_constants_are_the_headers():
    """A changed cap means the cases no longer sit on it."""
    assert define("lrx_search_select.h", "SEL_CAND") == R.SEL_CAND == 4096
    assert define("lrx_search_select.h", "SEL_EQCAP") == R.SEL_EQCAP == 2048
    assert define("lrx_search_select.h", "SEL_MAXK") == R.SEL_MAXK == 2048
    assert define("lrx_search_filter.h", "SP_ROWS") == R.SP_ROWS == 128
    assert define("lrx_search_sq8.h", "SQ8_NMAX") == R.SQ8_NMAX
    assert 2 * R.SEL_EQCAP == R.SEL_CAND           # the block lists (2 * SEL_EQCAP entries) and the candidate buffer share one cap in the case table


def test_key_is_monotone_over_the_special_values():
    s = np.concatenate([R.SPECIALS, np.float32([2.5, -2.5, 65535.0])])
    k = R.key(np.sort(s)).astype(np.int64)
    assert (np.diff(k) > 0).all()
    assert R.key(np.float32([-0.0]))[0] + 1 == R.key(np.float32([0.0]))[0]          # only -0 < +0 is finer than the float order
    assert R.key(np.float32([np.inf]))[0] == 0xFF800000 and R.key(np.float32([-np.inf]))[0] == 0x007FFFFF


@pytest.mark.parametrize("n,k", [(1, 1), (1, 5), (37, 37), (1000, 10), (1000, 999), (5000, 2048), (300, 400)])
def test_topk_equals_a_plain_python_sort(n, k):
    rng = np.random.default_rng(n * 7 + k)
    s = rng.standard_normal(n).astype(np.float32)
    s[rng.permutation(n)[:n // 2]] = rng.choice(s, 3)[rng.integers(0, 3, n // 2)]          # half of the rows share three values
    s[rng.permutation(n)[:n // 10]] = -R.FLT_MAX                                            # real rows at the padding's score
    ky = R.key(s).tolist()
    order = sorted(range(n), key=lambda r: (-ky[r], r))[:k]
    D, I = R.topk(s, k, id_base=50)
    assert I[:len(order)].tolist() == [r + 50 for r in order] and np.array_equal(bits(D[:len(order)]), bits(s[order]))
    assert (I[len(order):] == -1).all() and (D[len(order):] == -R.FLT_MAX).all() and len(D) == len(I) == k
    row_map = rng.permutation(10 * n)[:n]
    assert R.topk(s, k, row_map=row_map)[1][:len(order)].tolist() == row_map[order].tolist()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["name"])
def test_every_case_lands_on_its_label(case):
    v, S = rows_of(case)
    for k, label in zip(case["ks"], case["labels"]):
        got, counts = R.select_path(S[0], k)
        assert got in R.SELECT_LABELS
        if label is not None:
            assert got == label, (case["name"], k, got, counts)
        for name, want in case["counts"].get(k, {}).items():
            assert counts[name] == want, (case["name"], k, name, counts)


def test_the_cases_cover_every_select_path_and_mix_paths_inside_one_launch():
    seen, mixed = set(), 0
    for case in R.CASES:
        v, S = rows_of(case)
        for k in case["ks"]:
            labels = {R.select_path(s, k)[0] for s in S}
            seen |= labels
            mixed += len(labels) > 1
    assert seen == set(R.SELECT_LABELS)
    assert mixed >= 5                                # the queries of one call take different branches in several cases


def test_the_case_table_is_complete():
    names = {c["name"] for c in R.CASES}
    assert {f"tiny-{n}" for n in (1, 127, 128, 129, 300)} <= names and all(R.CASE_BY_NAME[f"tiny-{n}"]["id_base"] == 7000 for n in (1, 127, 128, 129, 300))
    assert {"direct-cap-4096", "direct-cap-4097", "fast-20000", "cand-cap-4096", "cand-cap-4097", "cand-overflow-distinct", "block-cap-4096",
            "block-cap-4097", "block-cap-4097-partial", "special-order"} <= names
    assert {f"tie-caps-{g}-{e}" for g, e in ((500, 2047), (500, 2048), (500, 2049), (999, 2049), (0, 2049))} <= names
    shape = lambda name: (len(rows_of(R.CASE_BY_NAME[name])[0]), R.CASE_BY_NAME[name]["ks"])
    assert shape("direct-cap-4096") == (4096, (1, 100, 2048)) and shape("direct-cap-4097") == (4097, (1, 100, 2048))
    assert shape("fast-20000") == (20000, (1, 10, 157, 158)) and shape("cand-cap-4097") == (20000, (10,))
    assert shape("block-cap-4096")[0] == 4096 * 128 and shape("block-cap-4097")[0] == 4097 * 128 and shape("block-cap-4097-partial")[0] == 4097 * 128 - 100
    assert shape("special-order") == (5000, (2048,)) and shape("tie-caps-0-2049") == (8192, (1000,))
    for n in (127, 128, 129, 300):                   # every special value on several rows
        assert np.bincount(rows_of(R.CASE_BY_NAME[f"tiny-{n}"])[0], minlength=11).min() >= 2
    v = rows_of(R.CASE_BY_NAME["cand-cap-4097"])[0]
    assert len(np.unique(np.flatnonzero(v == 60000) // 128)) == 157                 # the top level is spread over all blocks
    assert len(np.unique(rows_of(R.CASE_BY_NAME["direct-cap-4097"])[0])) == 4097    # a permutation: distinct scores
    assert {c["name"] for c in R.BAND_CASES} == {"band-cap-4096", "band-cap-4097", "band-direct", "band-merge", "band-maxk", "band-blocks-4096",
                                                 "band-blocks-4097"}


def test_tiny_cases_keep_a_real_flt_max_row_ahead_of_the_padding():
    case = R.CASE_BY_NAME["tiny-129"]
    v, S = rows_of(case)
    D, I = R.topk(S[0], 400, id_base=7000)
    real = np.flatnonzero(bits(D[:129]) == bits(-R.FLT_MAX))
    assert len(real) >= 2 and (I[real] >= 7000).all() and (I[129:] == -1).all() and (bits(D[129:]) == bits(-R.FLT_MAX)).all()
    assert (D[:129][real[-1] + 1:] == -np.inf).all()                                # -inf rows follow them, still before the padding


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["name"])
def test_pq_harness_reproduces_the_intended_rows_through_the_yardstick(case):
    v, S = rows_of(case)
    C = R.pq_tables(case["special"])
    with np.errstate(all="ignore"):
        got = pq_yardstick.scores(pq_yardstick.lut(R.pq_queries(case["queries"]), C), R.pq_codes(v, case["special"]))
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(S))
    if case["special"]:
        assert np.array_equal(bits(S[0]), bits(R.SPECIALS[v])) and np.array_equal(bits(S[1]), bits(np.float32(0) - R.SPECIALS[v]))
        if len(v) >= 127:
            assert len(np.unique(bits(S[0]))) == 11                                 # infinities, +-FLT_MAX, +-FLT_MIN, denormals: all there
    else:
        assert np.array_equal(S[0], v.astype(np.float32)) and np.array_equal(S[3], -v.astype(np.float32)) and v.max() < 65536


@pytest.mark.parametrize("case", R.BAND_CASES, ids=lambda c: c["name"])
def test_flat_and_sq8_harnesses_reproduce_the_levels(case):
    lv = case["make"]()
    assert lv.min() >= 1 and lv.max() <= 255
    # flat: a float64 matmul over the rows gives +-level exactly
    q = R.e0_queries(2, R.FLAT_D)
    got = (q.astype(np.float64) @ R.flat_rows(lv).astype(np.float64).T).astype(np.float32)
    assert np.array_equal(bits(got), bits(R.flat_intended(lv, 2)))
    # SQ8: the yardstick's scores, gathered per level, are the yardstick's scores of the rows and order like the levels
    S = R.sq8_expected_scores(lv, 2)
    sample = np.random.default_rng(0).permutation(len(lv))[:3000]
    direct = sq8_yardstick.scores(R.e0_queries(2, R.SQ8_D), R.sq8_codes(lv[sample]), R.SQ8_TRAINED)
    assert np.array_equal(bits(S[:, sample]), bits(direct))
    a, b = R.topk(S[0], case["k"]), R.topk(lv.astype(np.float32), case["k"])
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(R.topk(S[1], case["k"])[1], R.topk(-lv.astype(np.float32), case["k"])[1])


def test_sq8_scores_step_by_one_per_level():
    per = sq8_yardstick.scores(R.e0_queries(2, R.SQ8_D), R.sq8_codes(np.arange(256)), R.SQ8_TRAINED).astype(np.float64)
    assert np.abs(np.diff(per[0]) - 1.0).max() < 1e-4 and np.abs(np.diff(per[1]) + 1.0).max() < 1e-4
    assert np.abs(per[0] - (np.arange(256) + 0.5)).max() < 1e-4


def test_band_gap_holds_from_the_formulas():
    """2 eps 1.01 < half a level: about 0.012 for the flat harness, about 3e-4 for the SQ8 one."""
    assert 0.010 < 2 * R.flat_eps() < 0.014 and R.band_gap_ok("flat")
    assert 1e-4 < 2 * R.sq8_eps() < 5e-4 and R.band_gap_ok("sq8")


@pytest.mark.parametrize("case", R.BAND_CASES, ids=lambda c: c["name"])
def test_every_band_case_takes_its_form(case):
    lv = case["make"]()
    assert tuple(R.band_forms(lv, case["k"], 2)) == case["forms"]
    for harness in ("flat", "sq8"):                  # the band the kernel takes (kth - 2 eps, scores within eps of the level) gives the same form
        gap = 4 * R.BAND_EPS[harness]() * 1.01
        assert (R.band_form(lv.astype(np.float32), case["k"], gap), R.band_form(-lv.astype(np.float32), case["k"], gap)) == case["forms"]
    assert R.band_forms(lv, case["k"], 40) == list(case["forms"]) * 20


def test_band_cases_cover_the_forms_and_their_constructions():
    assert {f for c in R.BAND_CASES for f in c["forms"]} == set(R.BAND_LABELS)
    rows = lambda name, sign=1: R.band_counts(sign * R.BAND_BY_NAME[name]["make"]().astype(np.float32), R.BAND_BY_NAME[name]["k"], R.BAND_GAP)
    assert rows("band-cap-4096")[0] == 4096 and rows("band-cap-4097")[0] == 4097
    assert rows("band-direct") == (4097, 33)
    assert rows("band-blocks-4096") == (4096, 4096) and rows("band-blocks-4097") == (4097, 4097)
    assert rows("band-maxk")[0] == 4500 and R.BAND_BY_NAME["band-maxk"]["k"] == R.SEL_MAXK
    lv = R.BAND_BY_NAME["band-merge"]["make"]()
    high = np.flatnonzero(lv > 200)
    assert len(high) == 50 and len(np.unique(lv[high])) == 50 and len(np.unique(high // R.SEL_MAXK)) >= 5 and (lv == 200).sum() == 5000
    D, I = R.topk(lv.astype(np.float32), 100)
    assert set(I[:50].tolist()) == set(high.tolist()) and I[50:].tolist() == np.flatnonzero(lv == 200)[:50].tolist()     # the 50, then the 50 lowest tie rows
    assert len(np.unique(I[50:] // R.SEL_MAXK)) == 1 and len(np.unique(np.flatnonzero(lv == 200) // R.SEL_MAXK)) >= 5    # ... out of ties in every window


# ---- discrimination: a wrong tie rule applied to the model gives other ids than the expected ones -------------------------------------------
def wrong_higher_row(s, k):
    n = len(s)
    return np.lexsort((-np.arange(n), -R.key(s).astype(np.int64)))[:k]


def wrong_not_by_row(s, k):
    n = len(s)
    scramble = ((np.arange(n, dtype=np.int64) + 77) * 2654435761) % 1000003
    return np.lexsort((scramble, -R.key(s).astype(np.int64)))[:k]


def wrong_drops_one_tie(s, k):
    ky = R.key(s)
    kth = np.sort(ky)[len(s) - min(k, len(s))]
    keep = np.ones(len(s), bool)
    keep[np.flatnonzero(ky == kth)[0]] = False
    rows = np.flatnonzero(keep)
    return rows[np.lexsort((rows, -ky[rows].astype(np.int64)))[:k]]


def tie_rows():
    """(name, score row, k) of every query of every case whose k-th key is shared by more rows than the top-k takes of it."""
    out = []
    for case in R.CASES:
        v, S = rows_of(case)
        for k in case["ks"]:
            for i, s in enumerate(S):
                if len(s) > k:
                    ky = R.key(s)
                    kth = np.sort(ky)[len(s) - k]
                    if (ky == kth).sum() > k - (ky > kth).sum():
                        out.append((f"{case['name']}/k={k}/q={i}", s, k))
    for case in R.BAND_CASES:
        lv = case["make"]().astype(np.float32)
        out += [(f"{case['name']}/+", lv, case["k"]), (f"{case['name']}/-", -lv, case["k"])]
    return out


def test_every_tie_case_discriminates():
    ties = tie_rows()
    names = {t[0].split("/")[0] for t in ties}
    assert {"cand-cap-4097", "tie-caps-500-2047", "tie-caps-500-2048", "tie-caps-500-2049", "tie-caps-999-2049", "tie-caps-0-2049", "block-cap-4097",
            "block-cap-4097-partial", "special-order", "tiny-300", "band-merge", "band-maxk", "band-direct"} <= names
    for name, s, k in ties:
        want = R.topk(s, k)[1]
        for rule in (wrong_higher_row, wrong_not_by_row, wrong_drops_one_tie):
            got = rule(s, k)
            assert len(got) != len(want) or not np.array_equal(got, want), (name, rule.__name__)
