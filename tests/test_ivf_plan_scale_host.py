"""CPU: the helpers of tests/test_gpu_ivf_plan_scale.py (tests/ivf_plan_cases.py) and the de-duplication of the five inverted-file yardsticks.
The yardsticks keep the cells a probe row names in a list and a set of seen cells, and the three over codes score a query's rows in one call
with a base term per row; here they are held against the loop they replaced -- a scan of the list per entry, one scoring call per cell --
restated in this file, on probe rows with repeats, negatives and entries >= nlist."""
import numpy as np
import pytest

import ivf_plan_cases as PC
import ivf_range_yardstick as R
import ivf_yardstick as IV
import ivfpq_yardstick as YPQ
import ivfsq8_yardstick as YS8
import ivfsq_yardstick as YSQ

F32 = np.float32
FAMILIES = ("flat", "sq_fp16", "sq8", "pq")
SEARCH = {"flat": IV.search, "sq_fp16": YSQ.search, "sq8": YS8.search, "pq": YPQ.search}


def old_cells(probe_row, nlist):
    """The de-duplication the yardsticks had: every entry looked up in the list of the cells kept so far -> [(entry index, cell)]."""
    cells, kept = [], []
    for j, c in enumerate(probe_row):
        if 0 <= c < nlist and c not in cells:
            cells.append(int(c))
            kept.append((j, int(c)))
    return kept


def old_search(fam, head, list_off, row_ids, probes, probe_scores, by_residual, k, max_scan_rows=None):
    """The yardsticks' search as it was: one scoring call per kept cell with that cell's base term."""
    q = head[0]
    nlist = len(list_off) - 1
    if fam == "pq":
        L = YPQ.PQ.lut(q, head[1])
    if fam == "sq8":
        y = YS8.S8.decode(head[1], head[2])
    D = np.full((len(q), k), -IV.FLT_MAX, F32)
    I = np.full((len(q), k), -1, np.int64)
    for i in range(len(q)):
        sc, rows = [np.zeros(0, F32)], [np.zeros(0, np.int64)]
        for j, c in old_cells(probes[i], nlist):
            pos = np.arange(list_off[c], list_off[c + 1])
            base = float(F32(probe_scores[i][j])) if by_residual else 0.0
            if fam == "flat":
                sc.append(IV.exact_scores(q[i], head[1][pos]))
            elif fam == "sq_fp16":
                sc.append(YSQ.row_scores(q[i], head[1][pos], base))
            elif fam == "sq8":
                sc.append(YS8.row_scores(q[i], y[pos], base))
            else:
                sc.append(YPQ.row_scores(L[i], head[2][pos], F32(base)))
            rows.append(row_ids[pos])
        sc, rows = np.concatenate(sc), np.concatenate(rows)
        if max_scan_rows is not None and rows.size > max_scan_rows:
            continue
        order = np.lexsort((rows, -sc.astype(np.float64)))[:k]
        D[i, :order.size] = sc[order]
        I[i, :order.size] = rows[order]
    return D, I


def small_store(fam, seed=3):
    """(head, list_off, row_ids, probes with repeats, negatives and entries >= nlist, probe scores) of a dozen cells."""
    rng = np.random.default_rng(seed)
    sizes = [0, 3, 1, 0, 5, 2, 7, 1, 4, 0, 6, 2]
    nlist, n, d, Q = len(sizes), sum(sizes), 32, 5
    cells = rng.permutation(np.repeat(np.arange(nlist), sizes))
    row_ids, list_off = IV.cell_order(cells, nlist)
    q = rng.standard_normal((Q, d)).astype(F32)
    if fam == "flat":
        head = (q, rng.standard_normal((n, d)).astype(F32))
    elif fam == "sq_fp16":
        head = (q, rng.standard_normal((n, d)).astype(np.float16))
    elif fam == "sq8":
        head = (q, rng.integers(0, 256, (n, d)).astype(np.uint8), np.concatenate([np.full(d, -1.0), np.full(d, 2.0)]).astype(F32))
    else:
        head = (q, rng.standard_normal((4, 256, d // 4)).astype(F32), rng.integers(0, 256, (n, 4)).astype(np.uint8))
    probes = np.array([[4, 4, -1, 6, nlist, 4, 1, 6, 2 ** 40, 0],
                       [0, 3, 0, 9, 3, -5, 2 ** 62, nlist + 1, 9, 0],
                       [10, 8, 6, 4, 2, 1, 5, 7, 11, 3],
                       [7, -1, 7, -1, 7, nlist, 7, 11, 11, 7],
                       [-1, -1, -1, nlist, nlist, 2 ** 40, -1, -1, -1, -1]], np.int64)
    return head, list_off, row_ids, probes, rng.standard_normal(probes.shape).astype(F32)


@pytest.mark.parametrize("by_residual", [True, False])
@pytest.mark.parametrize("fam", FAMILIES)
def test_the_seen_set_keeps_the_cells_the_list_scan_kept(fam, by_residual):
    head, list_off, row_ids, probes, ps = small_store(fam)
    nlist, n = len(list_off) - 1, int(list_off[-1])
    kept = [old_cells(p, nlist) for p in probes]
    assert [len(k) for k in kept] == [4, 3, 10, 2, 0]                        # (empty cells are kept: they hold no rows)
    for i, p in enumerate(probes):
        want = np.concatenate([np.arange(list_off[c], list_off[c + 1]) for _, c in kept[i]] + [np.zeros(0, np.int64)])
        assert np.array_equal(R.scanned_positions(p, list_off), want)
    for k, bound in ((n, None), (4, None), (n, 12)):
        want = old_search(fam, head, list_off, row_ids, probes, ps, by_residual and fam != "flat", k, bound)
        got = IV.search(*head, list_off, row_ids, probes, k, max_scan_rows=bound) if fam == "flat" else \
            SEARCH[fam](*head, list_off, row_ids, probes, ps, by_residual, k, max_scan_rows=bound)
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)) and np.array_equal(got[1], want[1])
        assert (want[1][:, 0] >= 0).any()
    scanned = R.scanned_rows(probes, list_off)
    assert (scanned > 12).any() and (scanned[scanned <= 12] > 0).any()       # the bound drops a query and keeps one


@pytest.mark.parametrize("fam", FAMILIES)
def test_one_cached_search_gives_every_top_k_and_every_range_result(fam):
    head, list_off, row_ids, probes, ps = small_store(fam)
    n = int(list_off[-1])
    br = None if fam == "flat" else True
    for bound in (None, 12):
        ref = PC.CachedSearch(SEARCH[fam], head, list_off, row_ids, probes, None if br is None else ps, br, max_scan_rows=bound)
        for k in (1, 4, n):
            want = IV.search(*head, list_off, row_ids, probes, k, max_scan_rows=bound) if fam == "flat" else \
                SEARCH[fam](*head, list_off, row_ids, probes, ps, True, k, max_scan_rows=bound)
            got = ref.topk(k)
            assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)) and np.array_equal(got[1], want[1])
        for radius in (-np.inf, ref.median(), np.inf):
            want = R.expected(SEARCH[fam], head, probes, list_off, row_ids, radius, max_scan_rows=bound, probe_scores=None if br is None else ps, by_residual=br)
            got = ref.range(radius)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
        assert np.array_equal(ref.scanned(), R.scanned_rows(probes, list_off, bound))
        assert R.some_query_is_partial(ref.range(ref.median())[0], ref.scanned())


def test_the_scale_store_puts_cells_on_the_boundaries_of_the_item_scan():
    sizes = np.array(PC.scale_sizes())
    assert sizes.size == 2500 and (sizes.size + 1 + 1023) // 1024 == 3                   # k_ivf_items: runs of 3 cells
    assert sizes[0] == 0 and 190 <= (sizes == 0).sum() <= 215 and 6000 <= sizes.sum() <= 8000
    assert all(sizes[c] == s for c, s in PC.BIG_CELLS.items())
    assert {2 // 3, 3 // 3} == {0, 1} and {191 // 3 // 64, 192 // 3 // 64} == {0, 1}     # a thread-run boundary, a wave boundary
    small = np.delete(sizes, list(PC.BIG_CELLS))
    assert small.max() == 3 and set(small.tolist()) == {0, 1, 2, 3}
    assert (sizes > 0).sum() > PC.NPROBE_MAX                                             # 2048 distinct non-empty cells exist
    for nlist in (1023, 1024, 1025):
        e = np.array(PC.edge_sizes(nlist))
        assert e.size == nlist and e[0] == 0 and e[-1] == 129 and set(e[:-1].tolist()) == {0, 1, 2}
    assert [(nl + 1 + 1023) // 1024 for nl in (1023, 1024, 1025)] == [1, 2, 2]           # the run length changes between 1023 and 1024 cells


def test_prefix_probes_and_the_row_helpers():
    rng = np.random.default_rng(0)
    sizes = np.array(PC.scale_sizes())
    list_off = np.concatenate([[0], np.cumsum(sizes)])
    p = PC.prefix_probes(rng, 6, 257, np.arange(2500))
    assert p.shape == (6, 257) and p.dtype == np.int64 and all(len(set(r.tolist())) == 257 for r in p)
    assert (sizes[p] == 0).any()                                                         # empty cells are named
    full = PC.prefix_probes(rng, 3, 2048, np.flatnonzero(sizes > 0))
    assert (sizes[full] > 0).all() and all(len(set(r.tolist())) == 2048 for r in full)
    w = PC.with_cell(p, 2499, [0, 3], rng)
    assert (w[0] == 2499).any() and (w[3] == 2499).any() and (w != p).sum() <= 2 and np.array_equal(w[[1, 2, 4, 5]], p[[1, 2, 4, 5]])
    lf, scanned = PC.largest_first(p, list_off)
    assert np.array_equal(scanned, R.scanned_rows(lf, list_off)) and scanned[0] == scanned.max() and (scanned[1:] < scanned[0]).all()
    assert sorted(map(tuple, lf.tolist())) == sorted(map(tuple, p.tolist()))


def test_the_crafted_rows_hold_the_patterns_they_are_named_for():
    sizes = np.array(PC.scale_sizes())
    nlist = sizes.size
    P = PC.crafted_probes(sizes)
    assert P.shape == (7, 2048) and P.dtype == np.int64
    valid = (P >= 0) & (P < nlist)
    bad = P >= nlist
    first = np.zeros_like(valid)                                                         # the first occurrence of a cell in its row
    for i in range(7):
        _, idx = np.unique(P[i], return_index=True)
        first[i, idx] = True
    live = valid & first & (sizes[np.where(valid, P, 0)] > 0)                            # the entries that own rows
    a, b, c, d, e, f, g = range(7)
    # a: whole thread runs (8 entries) of each kind of skip, and across the wave boundary at 512 and the one at 1024
    assert (P[a, 8:16] == -1).all() and bad[a, 24:32].all() and (valid & ~first)[a, 40:48].all()
    assert (P[a, 504:512] == -1).all() and bad[a, 512:520].all() and (valid & ~first)[a, 1016:1024].all() and bad[a, 1024:1032].all()
    assert {int(v) for v in P[a][bad[a]]} == {nlist, 2 ** 40, 2 ** 62}
    assert live[a, :8].any() and live[a, 520:1016].any() and live[a, 1032:].any()
    # b: no entry of wave 1 owns rows, by all three kinds of skip; the waves around it do
    assert not live[b, 512:1024].any() and (P[b, 512:1024] == -1).sum() == 171 and bad[b, 512:1024].sum() == 171
    assert (valid & ~first)[b, 512:1024].sum() == 170 and live[b, :512].any() and live[b, 1024:].any()
    # c: one cell of many rows at entry 0 and again at 7, 8, 511, 512, 2047
    x = P[c, 0]
    assert sizes[x] >= 100 and np.flatnonzero(P[c] == x).tolist() == [0, 7, 8, 511, 512, 2047] and live[c, 0] and not live[c, [7, 8, 511, 512, 2047]].any()
    # d: an empty cell twice and an entry >= nlist twice
    assert P[d, 5] == P[d, 700] and sizes[P[d, 5]] == 0 and P[d, 9] == P[d, 1500] == 2 ** 40 and bad[d].sum() == 2
    # e, f, g
    assert np.flatnonzero(live[e]).tolist() == [2047] and np.flatnonzero(live[f]).tolist() == [0] and not live[g].any()
    for i in (e, f, g):
        assert bad[i].any() and (P[i] == -1).any() and (valid[i] & (sizes[np.where(valid[i], P[i], 0)] == 0)).any()
    list_off = np.concatenate([[0], np.cumsum(sizes)])
    assert R.scanned_rows(P, list_off)[[e, f, g]].tolist() == [129, 129, 0]
