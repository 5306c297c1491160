"""The host side of the index life-cycle check (index_lifecycle.py), no GPU: the generator's conditions for every (family, seed)
test_gpu_index_lifecycle.py runs, the op table against the classes, the model's `live` after every named sequence, and that the expected side
of every checkpoint can be computed from the yardsticks alone."""
import numpy as np
import pytest

import index_lifecycle as L

CASES = [(f, s) for f in L.FAMILIES for s in L.SEEDS]


@pytest.mark.parametrize("family,seed", CASES)
def test_generated_sequence_meets_every_condition(family, seed):
    ops = L.sequence(family, seed)
    assert ops == L.sequence(family, seed)                                   # deterministic from the seed alone
    cond = L.conditions(family, ops)
    assert all(cond.values()), {k: v for k, v in cond.items() if not v}
    assert len(ops) <= 14 and sum(o[0] == "check" for o in ops) <= 6
    feats = L.features(family, ops)
    assert all(feats[f] for f in L.wanted_features(family, seed)), feats
    lo, hi = L.SPECS[family].big
    for op in ops:                                                           # sizes: the edges, or the family's [200, 900]; a post-reset size below 256
        if op[0] == "add":
            assert op[1] in L.EDGE_SIZES or lo <= op[1] <= hi or op[1] < 256
        if op[0] == "slot":
            assert op[2] in (0, op[1] // 2, op[1])


@pytest.mark.parametrize("family", L.FAMILIES)
def test_seeds_differ_in_op_order_and_cover_every_op_value(family):
    """The seeds of a family are different SEQUENCES, not one script with other sizes, and between them they issue every value the op table
    names: an empty add on a non-empty index, a slot committed whole, a reserve below, equal to and above ntotal on a non-empty index, and
    reset / reload / slot / reserve in both orders."""
    seqs = [L.sequence(family, s) for s in L.SEEDS]
    assert len({tuple(o[0] for o in ops) for ops in seqs}) == len(L.SEEDS)
    spec = L.SPECS[family]
    held = {f for ops in seqs for f, v in L.features(family, ops).items() if v}
    want = {"add_0"}
    if "slot" in spec.ops:
        want |= {"slot_all", "slot_after_reset"}
        assert any(o[0] == "slot" and o[2] < o[1] for ops in seqs for o in ops)
    if "reserve" in spec.ops:
        want |= {"reserve_below", "reserve_equal", "reserve_above", "reserve_after_reload"}
    if "reload" in spec.ops:
        want.add("reset_before_reload")
        assert any(not L.features(family, ops)["reset_before_reload"] for ops in seqs)          # ... and a reload before the reset
    if "toggle" in spec.ops:
        want.add("toggle")
        assert {o[1] for ops in seqs for o in ops if o[0] == "toggle"} == {"shadow_f16", "two_pass"}
    assert want <= held, want - held


def test_conditions_reject_what_they_should():
    ops = L.sequence("pq", 0)
    grown_once = [("check",), ("add", 300), ("check",), ("check",), ("reset",), ("add", 5), ("check",)]     # the only growth is from nothing
    assert not L.conditions("pq", grown_once)["realloc"]
    assert L.conditions("pq", grown_once[:2] + [("reserve", 5000)] + grown_once[2:])["realloc"]
    assert not L.conditions("pq", grown_once[:2] + [("reserve", 300)] + grown_once[2:])["realloc"]
    assert not L.conditions("pq", ops[:-1])["ends_with_check"] or ops[-2][0] == "check"
    assert not L.conditions("pq", [o for o in ops if o[0] != "reset"])["reset_shrinks"]
    assert not L.conditions("pq", [o for o in ops if o[0] != "slot"])["slot_partial"]
    assert L.conditions("pq", grown_once)["empty_check"] and not L.conditions("pq", grown_once[1:])["empty_check"]
    assert not L.conditions("ivf_flat", grown_once[:2] + [("reserve", 5000)])["served"]      # (reserve: the inverted-file classes have none)
    ivf = [("check",), ("add", 300), ("check",), ("add", 1), ("check",), ("check",), ("reset",), ("add", 5), ("check",)]
    c = L.conditions("ivf_sq", ivf)
    assert c["sorted_and_tail"] and c["finalize_no_op"] and c["empty_cell"]
    assert not L.conditions("ivf_sq", ivf[:5] + ivf[6:])["finalize_no_op"]
    assert not L.conditions("ivf_sq", ivf[:3] + ivf[5:])["sorted_and_tail"]
    assert not L.conditions("ivf_sq", ivf[:6] + [("check",)])["empty_cell"]


def test_op_table_matches_the_classes():
    import lightretriever_amd as A
    for family, spec in L.SPECS.items():
        cls = getattr(A, spec.cls)
        for op in L.OPS:
            has = all(hasattr(cls, name) for name in L.NEEDS[op])
            assert has == (op in spec.ops), f"{family}: op {op!r} is {'served by' if has else 'missing from'} {spec.cls}, the table says otherwise"
    for name, (families, ops, _) in L.NAMED.items():
        for f in families:
            assert all(o[0] in L.SPECS[f].ops or o[0] in ("add_cell", "set_contents", "add_docs") for o in ops), (name, f)


@pytest.mark.parametrize("name", list(L.NAMED))
def test_named_sequence_leaves_the_rows_its_comment_says(name):
    families, ops, ntotals = L.NAMED[name]
    family = families[-1]
    m, checks = L.replay(family, ops)
    assert [e["ntotal"] for e in checks] == ntotals == [t["after"] for t in L.simulate(family, ops) if t["op"][0] == "check"]
    assert m.n == ntotals[-1] and (family == "impact" or m.live.shape == (ntotals[-1], m.d_in))
    if name == "impact_new_largest_term":                                    # the postings, written out by hand from the five documents
        a, b = checks
        assert (a["n_terms"], a["nnz"], a["term_off"].tolist(), a["maxw"].tolist()) == (5, 5, [0, 1, 2, 4, 4, 5], [5, 2, 3, 0, 7])
        assert a["postings"].tolist() == [[0, 5], [2, 2], [0, 1], [1, 3], [1, 7]]
        assert (b["n_terms"], b["nnz"], b["term_off"].tolist()) == (10, 7, [0, 2, 3, 5, 5, 6, 6, 6, 6, 6, 7])
        assert b["postings"].tolist() == [[0, 5], [3, 6], [2, 2], [0, 1], [1, 3], [1, 7], [3, 4]] and b["maxw"].tolist() == [6, 2, 3, 0, 7, 0, 0, 0, 0, 4]
    if name == "ivf_reset_then_one_cell":
        assert (checks[-1]["list_sizes"] == np.eye(L.NLIST, dtype=np.int64)[3] * 40).all()
    if name == "reset_then_fewer_same_block":
        assert (ntotals[1] - 1) // 128 == (ntotals[0] - 1) // 128


@pytest.mark.parametrize("family", L.FAMILIES)
def test_expected_side_is_computable_and_a_function_of_the_live_rows(family):
    for seed in L.SEEDS[:2]:
        ops = L.sequence(family, seed)
        m, checks = L.replay(family, ops, seed)
        assert len(checks) == sum(o[0] == "check" for o in ops)
        assert [e["ntotal"] for e in checks] == [t["after"] for t in L.simulate(family, ops) if t["op"][0] == "check"]
        for e in checks:
            assert len(e["search"]) >= 3 and all(s["D"].shape == s["I"].shape == (L.NQ, s["k"]) for s in e["search"])
            assert ("range" in e) == (family in L.HAS_RANGE and e["ntotal"] > 0)
            if L.SPECS[family].kind == "ivf" and 0 < e["ntotal"] < L.NLIST:
                assert (e["list_sizes"] == 0).any()
        # the last checkpoint again from a fresh model that is handed the live rows in one piece: the same expectations
        fresh = L.make_model(family, seed)
        if family == "impact":
            fresh.live = list(m.live)
        else:
            fresh.append(m.live)
        a, b = checks[-1], fresh.expect()
        assert np.array_equal(a.get("codes", 0), b.get("codes", 0)) and all(np.array_equal(x["I"], y["I"]) and np.array_equal(x["D"], y["D"])
                                                              for x, y in zip(a["search"], b["search"]))
