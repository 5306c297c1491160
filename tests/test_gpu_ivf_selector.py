"""GPU: row-selector filtered search of the four inverted-file indexes (lrx_selector_*, lrx_ivf_*_ip_search_sel / _range_search_sel,
torch.ops.lrx.ivf_*_sel, ops.ivf_*_sel, RowSelector, search(sel=) / range_search_probed(sel=), FaissIndex).  Every comparison is
on bits and needs no tolerance: every scanned (query, row) pair is scored independently of the others, so a filtered result IS the
unfiltered full result restricted to the selected rows (tests/ivf_selector_yardstick.py), and with every cell probed the flat family's IS the
flat index's over the selected rows alone.  The hand-made cells are those of tests/test_gpu_ivf_range.py (tests/ivf_store.py's Store)."""
import numpy as np
import pytest
import torch

import ivf_selector_yardstick as Y
import ivf_store as RG
from ivf_store import FAMILIES, Store, dev, errors

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
FLT_MAX = float(np.finfo(F32).max)
SIZES_N = (1, 31, 32, 33, 64, 65, 1000)


def host(t):
    return t.cpu().numpy()


def same_topk(got, want):
    (gD, gI), (wD, wI) = ((host(t) if isinstance(t, torch.Tensor) else t for t in pair) for pair in (got, want))
    return gD.shape == wD.shape and np.array_equal(gD.view(np.int32), wD.view(np.int32)) and np.array_equal(gI, wI)


def same_range(got, want):
    g, w = ([host(t) if isinstance(t, torch.Tensor) else t for t in x] for x in (got, want))
    return np.array_equal(g[0], w[0]) and g[1].shape == w[1].shape and np.array_equal(g[1].view(np.int32), w[1].view(np.int32)) and np.array_equal(g[2], w[2])


def selector(mask):
    from lightretriever_amd import RowSelector
    return RowSelector.from_mask(np.asarray(mask, bool))


# ---- 1. the selector kernels against the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES_N)
def test_the_constructors_pack_what_the_yardstick_packs(n):
    from lightretriever_amd import RowSelector
    rng = np.random.default_rng(n)
    empty = RowSelector(n)
    assert empty.n == n and empty.words.dtype == torch.int32 and empty.words.is_cuda and empty.words.is_contiguous()
    assert tuple(empty.words.shape) == ((n + 31) // 32,) and not empty.words.any() and empty.count() == 0
    for mask in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) % 2 == 1, np.arange(n) == n - 1):
        want = Y.pack(mask)
        for sel in (RowSelector.from_mask(mask), RowSelector.from_mask(torch.from_numpy(mask)), RowSelector.from_mask(torch.from_numpy(mask).cuda())):
            assert np.array_equal(host(sel.words), want) and Y.tail_is_clear(host(sel.words), n)
            assert np.array_equal(host(sel.to_mask()), mask) and sel.to_mask().dtype == torch.bool and sel.to_mask().is_cuda
            assert sel.count() == int(mask.sum())
        rows = np.flatnonzero(mask).astype(np.int64)
        rows = rng.permutation(np.concatenate([rows, rows[: len(rows) // 2], rows[:1]]))                # duplicates, any order
        by_rows = RowSelector.from_rows(torch.from_numpy(rows), n)
        assert np.array_equal(host(by_rows.words), want)
        inv = sel.invert()
        assert inv is not sel and np.array_equal(host(inv.words), Y.pack(~mask)) and Y.tail_is_clear(host(inv.words), n)
        assert np.array_equal(host(sel.words), want)                                                   # the source is left alone
        assert np.array_equal(host(inv.invert().words), want)
    for lo, hi in ((0, n), (0, 0), (n // 2, n), (n // 3, n // 3 + 1), (1, n - 1), (-5, n + 5), (n, n), (31, 33), (32, 64)):
        m = np.zeros(n, bool)
        m[max(lo, 0):max(min(hi, n), 0)] = True
        got = RowSelector.from_range(lo, hi, n)
        assert np.array_equal(host(got.words), Y.pack(m)), (n, lo, hi)
    assert errors() == 0


@pytest.mark.parametrize("n", SIZES_N)
def test_rows_outside_the_selector_are_skipped_and_counted(n):
    from lightretriever_amd import RowSelector
    errors()
    inside = np.arange(0, n, 3, dtype=np.int64)
    rows = np.concatenate([[n], inside, [-1]]).astype(np.int64)
    sel = RowSelector.from_rows(rows, n)
    assert errors() == 2
    m = np.zeros(n, bool)
    m[inside] = True
    assert np.array_equal(host(sel.words), Y.pack(m)) and Y.tail_is_clear(host(sel.words), n)
    assert errors() == 0


def test_the_in_place_setters_keep_the_storage_and_refuse_other_shapes():
    from lightretriever_amd import RowSelector
    n = 1000
    rng = np.random.default_rng(0)
    a, b = rng.random(n) < 0.3, rng.random(n) < 0.7
    sel = RowSelector.from_mask(a)
    p = sel.words.data_ptr()
    assert sel.set_mask_(b) is sel and sel.words.data_ptr() == p and np.array_equal(host(sel.words), Y.pack(b))
    assert sel.set_rows_(torch.from_numpy(np.flatnonzero(a))) is sel and sel.words.data_ptr() == p and np.array_equal(host(sel.words), Y.pack(a))
    strided = torch.from_numpy(np.stack([b, ~b], axis=1)).cuda()[:, 0]                                 # a column: not contiguous
    assert sel.set_mask_(strided).words.data_ptr() == p and np.array_equal(host(sel.words), Y.pack(b))
    view = torch.from_numpy(np.concatenate([[True], a])).cuda()[1:]                                   # a mask that is not 16-byte aligned
    assert np.array_equal(host(sel.set_mask_(view).words), Y.pack(a))
    for bad in (np.ones(n + 1, bool), np.ones(n, np.uint8), np.ones((n, 1), bool)):
        with pytest.raises(ValueError, match="mask"):
            sel.set_mask_(bad)
    with pytest.raises(ValueError, match="rows"):
        sel.set_rows_(np.arange(3, dtype=np.int32))
    with pytest.raises(ValueError, match="n=-1"):
        RowSelector(-1)
    assert RowSelector(0).words.numel() == 0 and RowSelector(0).count() == 0 and RowSelector(0).invert().n == 0
    assert errors() == 0


# ---- 2. an oracle that runs none of the new code: the flat index over the selected rows alone ---------------------------------------------------
_FLAT = {}


def flat_case(Q, n, d, nlist):
    if (Q, n, d, nlist) not in _FLAT:
        from lightretriever_amd import IVFFlatIndex
        rng = np.random.default_rng(n + d)
        x = dev(rng.standard_normal((n, d)).astype(F32))
        q = dev(rng.standard_normal((Q, d)).astype(F32))
        idx = IVFFlatIndex(d, nlist, nprobe=nlist)
        idx.train(x, niter=1)
        idx.add(x)
        _FLAT[(Q, n, d, nlist)] = (x, q, idx)
    return _FLAT[(Q, n, d, nlist)]


@pytest.mark.parametrize("share", [0.5, 0.05])
@pytest.mark.parametrize("Q, n, d, nlist, k", [(3, 300, 96, 7, 10), (4, 600, 2112, 16, 10), (130, 5000, 256, 64, 100), (2, 300, 32, 4, 300)])
def test_probing_every_cell_under_a_selector_is_the_flat_search_over_the_selected_rows(Q, n, d, nlist, k, share):
    from lightretriever_amd import FlatIPIndex
    x, q, idx = flat_case(Q, n, d, nlist)
    mask = np.random.default_rng(int(share * 100) + n).random(n) < share
    rows = dev(np.flatnonzero(mask).astype(np.int64))
    assert 0 < len(rows) < n
    flat = FlatIPIndex(d)
    flat.add(x[rows])
    D, I = flat.search(q, k)
    want = (D, torch.where(I >= 0, rows[I.clamp(min=0)], I))                 # row_map = the selected row numbers
    got = idx.search(q, k, sel=selector(mask))
    assert same_topk(got, want)
    if k > len(rows):
        assert (got[1][:, len(rows):] == -1).all() and (got[0][:, len(rows):] == -FLT_MAX).all() and (got[1][:, :len(rows)] >= 0).all()
    assert mask[host(got[1])[host(got[1]) >= 0]].all()
    assert errors() == 0


# ---- 3. all four families, top k and range, against their own unfiltered full result ----------------------------------------------------------
SIZES = [0, 1, 7, 9, 160, 50, 40, 33]             # empty; 1, 7, 9 rows; one cell with more than half of the 300 rows: two groups of 128 at d = 32
BIG = 4
CASES = [("flat", True), ("sq_fp16", True), ("sq_fp16", False), ("sq8", True), ("sq8", False), ("pq", True), ("pq", False)]
_STORES = {}


def store(fam, by_residual, d):
    key = (fam, by_residual, d)
    if key not in _STORES:
        _STORES[key] = Store(fam, SIZES, d=d, Q=130, seed=3, by_residual=by_residual)
    return _STORES[key]


def masks(S):
    """name -> bool [n] over the ORIGINAL rows."""
    n = S.n
    rng = np.random.default_rng(5)
    out = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "one": np.arange(n) == int(S.row_ids[S.list_off[BIG] + 130]),
           "alternating": np.arange(n) % 2 == 0, "edges": np.isin(np.arange(n), [31, 32, 63, 64]), "random": rng.random(n) < 0.3}
    cell = np.ones(n, bool)
    cell[S.row_ids[S.list_off[5]:S.list_off[6]]] = False                     # one whole cell cleared
    out["cell"] = cell
    group = np.ones(n, bool)                                                  # one whole staged group cleared inside the large cell: its
    first = 128 if S.d == 32 else 16                                          # first 128 stored rows at d = 32 (G = 128), its first 16 at
    group[S.row_ids[S.list_off[BIG]:S.list_off[BIG] + first]] = False         # d = 2048 (G = 8 for fp32 and 8-bit rows, 16 for fp16 codes)
    out["group"] = group
    return out


@pytest.mark.parametrize("d", [32, 2048])
@pytest.mark.parametrize("fam, by_residual", CASES)
def test_a_filtered_result_is_the_unfiltered_full_result_restricted_to_the_selected_rows(fam, by_residual, d, monkeypatch):
    from lightretriever_amd import RowSelector
    if fam == "pq" and d == 2048:
        monkeypatch.setattr(RG, "M_PQ", 32)                                  # (the Store's 8 sub-spaces would be 256 wide: PQIndex serves <= 64)
    S = store(fam, by_residual, d)
    assert S.n == 300 and max(SIZES) > S.n // 2
    k = 20
    sel = RowSelector(S.n)
    idx = S.index(1)
    for nprobe in (1, 3, S.nlist):
        for Q in (3, 130):
            q = dev(S.q[:Q])
            full = tuple(host(t) for t in idx.range_search_probed(q, -INF, nprobe))  # every scanned pair, in segment order, original rows
            assert int(full[0][-1]) > 0
            radius = float(np.median(full[1]))
            above = tuple(host(t) for t in idx.range_search_probed(q, radius, nprobe))
            plain_topk = idx.search(q, k, nprobe=nprobe)
            for name, mask in masks(S).items():
                sel.set_mask_(mask)
                got_k = idx.search(q, k, nprobe=nprobe, sel=sel)
                assert same_topk(got_k, Y.filter_topk(*Y.split(*full), mask, k)), (name, nprobe, Q)
                got_r = idx.range_search_probed(q, radius, nprobe, sel=sel)
                assert same_range(got_r, Y.filter_range(*above, mask)), (name, nprobe, Q)
                got_all = idx.range_search_probed(q, -INF, nprobe, sel=sel)
                assert same_range(got_all, Y.filter_range(*full, mask)), (name, nprobe, Q)
                if name == "all":
                    assert same_topk(got_k, plain_topk) and same_range(got_r, above) and same_range(got_all, full)
                if name == "none":
                    assert (got_k[1] == -1).all() and (got_k[0] == -FLT_MAX).all() and not got_r[0].any() and got_r[1].numel() == 0
                if name == "one" and nprobe == S.nlist:
                    assert (got_k[1][:, 0] >= 0).all() and (got_k[1][:, 1:] == -1).all() and host(got_all[0]).tolist() == list(range(Q + 1))
    assert errors() == 0


# ---- 4. stale words: the workspace is not cleared between calls -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam, by_residual", [("flat", True), ("sq_fp16", True), ("sq8", True), ("pq", True)])
def test_alternating_selectors_on_one_workspace_leave_no_stale_words(fam, by_residual):
    S = store(fam, by_residual, 32)
    idx = S.index(S.nlist)
    q = dev(S.q[:5])
    k = 50
    full = tuple(host(t) for t in idx.range_search_probed(q, -INF))
    sparse = np.random.default_rng(1).random(S.n) < 0.05
    first = tuple(t.clone() for t in idx.search(q, k))
    ws = idx._ws.data_ptr()
    steps = [("unfiltered", None, np.ones(S.n, bool)), ("sparse", selector(sparse), sparse), ("inverse", selector(sparse).invert(), ~sparse),
             ("unfiltered", None, np.ones(S.n, bool))]
    for kind in ("topk", "range"):
        for name, sel, mask in steps:
            if kind == "topk":
                got = idx.search(q, k) if sel is None else idx.search(q, k, sel=sel)
                assert same_topk(got, Y.filter_topk(*Y.split(*full), mask, k)), name
                last = got
            else:
                got = idx.range_search_probed(q, -INF) if sel is None else idx.range_search_probed(q, -INF, sel=sel)
                assert same_range(got, Y.filter_range(*full, mask)), name
            assert idx._ws.data_ptr() == ws                                  # one workspace throughout
        if kind == "topk":
            assert same_topk(last, first)
    assert errors() == 0


# ---- 5. the probe-list rules, max_scan_rows and the id mapping are unchanged under a selector (ops level, hand-given probes) -------------------
NO_SEL = object()


def op_args(S, probes, base, scalar, words=NO_SEL, max_scan=None, id_base=0, row_map=None, row_ids=True):
    """The arguments of ops.ivf_<fam>_ip_{topk, range_search}_sel and of the torch ops of the same names (scalar: k or the radius; words: the
    selector's, or None); without `words`, those of the plain siblings."""
    q, probes = dev(S.q[:len(probes)]), dev(np.asarray(probes, np.int64))
    dids = S.dids if row_ids else None
    base = None if base is None else dev(np.asarray(base, F32))
    sel = () if words is NO_SEL else (words,)
    tail = (scalar, S.n if max_scan is None else max_scan, id_base, row_map)
    if S.fam == "flat":
        return (q, S.dhead[0], S.doff, dids, probes) + sel + tail
    mid = (S.doff, dids, probes, base) + sel + (bool(S.by_residual),)
    if S.fam == "sq8":
        return (q, S.dhead[0], S.dhead[1], 0) + mid + tail
    return (q,) + S.dhead + mid + tail


def both(S, kind, *a, **kw):
    """ops.py and the torch op, which must agree -> the result."""
    from lightretriever_amd import ops, torch_ops
    torch_ops.load()
    name = f"ivf_{S.fam}_ip_{kind}_sel"
    args = op_args(S, *a, **kw)
    r1, r2 = getattr(ops, name)(*args), getattr(torch.ops.lrx, name)(*args)
    assert (same_topk if kind == "topk" else same_range)(r1, r2)
    return r1


PROBES = np.array([[4, 2, 4, 6], [5, 5, 3, -1], [6, len(SIZES), 1, 2 ** 40], [7, 6, 5, 4], [0, 0, -1, -1], [1, 2, 3, 7]], np.int64)


@pytest.mark.parametrize("fam", FAMILIES)
def test_the_probe_rules_the_scan_bound_and_the_id_mapping_hold_under_a_selector(fam):
    S = store(fam, True, 32)
    base = S.base(PROBES.shape)
    mask = np.random.default_rng(2).random(S.n) < 0.4
    words = selector(mask).words
    k = 30
    errors()
    from lightretriever_amd import ops
    plain = lambda *a, **kw: tuple(host(t) for t in getattr(ops, f"ivf_{fam}_ip_range_search")(*op_args(S, *a, **kw)))
    full = plain(PROBES, base, -INF)                                         # the unfiltered full result of the same probe rows (plain ops)
    assert errors() == 2                                                     # query 2's two entries past nlist
    scanned = np.diff(full[0]).tolist()
    assert scanned == [160 + 7 + 40, 50 + 9, 40 + 1, 33 + 40 + 50 + 160, 0, 1 + 7 + 9 + 33]       # a cell named twice is scanned once
    want_k, want_r = Y.filter_topk(*Y.split(*full), mask, k), Y.filter_range(*full, mask)
    got_k = both(S, "topk", PROBES, base, k, words)
    got_r = both(S, "range_search", PROBES, base, -INF, words)
    assert errors() == 4 * 2                                                 # counted as without a selector, in each of the four calls
    assert same_topk(got_k, want_k) and same_range(got_r, want_r)
    assert host(got_r[0])[5] == host(got_r[0])[4] and (got_k[1][4] == -1).all()
    # no selector through the _sel names: the plain result
    assert same_range(both(S, "range_search", PROBES, base, -INF, None), full)
    errors()
    # one row short for query 3: padding and counted whatever the selector says; its neighbours keep their results
    short_k = both(S, "topk", PROBES, base, k, words, max_scan=scanned[3] - 1)
    short_r = both(S, "range_search", PROBES, base, -INF, words, max_scan=scanned[3] - 1)
    assert errors() == 4 * (2 + 1)
    keep = [0, 1, 2, 4, 5]
    assert (short_k[1][3] == -1).all() and same_topk((short_k[0][keep], short_k[1][keep]), (want_k[0][keep], want_k[1][keep]))
    lims = host(short_r[0])
    assert lims[4] == lims[3] and np.diff(lims)[keep].tolist() == np.diff(want_r[0])[keep].tolist()
    sparse_sel = selector(np.arange(S.n) == 0).words                         # ... even a selector that leaves one row
    assert (both(S, "topk", PROBES, base, k, sparse_sel, max_scan=scanned[3] - 1)[1][3] == -1).all() and errors() == 2 * (2 + 1)
    # id_base and row_map are applied after the filter: the selector speaks of rows, not of ids
    rm = dev(np.arange(S.n, dtype=np.int64)[::-1].copy() * 3 + 11)
    based = both(S, "topk", PROBES, base, k, words, id_base=1000)
    mapped = both(S, "topk", PROBES, base, k, words, row_map=rm)
    rows = torch.from_numpy(want_k[1]).cuda()
    assert torch.equal(based[1], torch.where(rows >= 0, rows + 1000, rows)) and torch.equal(mapped[1], torch.where(rows >= 0, rm[rows.clamp(min=0)], rows))
    assert torch.equal(based[0], got_k[0]) and torch.equal(mapped[0], got_k[0])
    mapped_r = both(S, "range_search", PROBES, base, -INF, words, row_map=rm)
    assert torch.equal(mapped_r[2], rm[torch.from_numpy(want_r[2]).cuda()])
    errors()
    # row_ids = None: the stored positions are the rows, and the selector is over positions
    n_pos = S.n if fam != "pq" else -(-S.n // 128) * 128                     # (the blocked PQ codes hold whole 128-row blocks)
    pos_mask = np.random.default_rng(4).random(n_pos) < 0.4
    clean = np.array([[4, 2, 6], [1, 3, 7]], np.int64)
    cbase = None if base is None else base[:2, :3]
    full_p = plain(clean, cbase, -INF, row_ids=False)
    assert np.array_equal(full_p[2][:160], np.arange(S.list_off[4], S.list_off[5]))                 # positions
    got_p = both(S, "range_search", clean, cbase, -INF, selector(pos_mask).words, row_ids=False)
    assert same_range(got_p, Y.filter_range(*full_p, pos_mask))
    assert errors() == 0


# ---- 6. a query's filtered result does not depend on its batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam, by_residual", [("flat", True), ("sq_fp16", True), ("sq8", False), ("pq", True)])
def test_a_querys_filtered_result_does_not_depend_on_its_batch(fam, by_residual):
    S = store(fam, by_residual, 32)
    idx = S.index(3)
    sel = selector(np.random.default_rng(6).random(S.n) < 0.3)
    q = dev(S.q)
    Dk, Ik = idx.search(q, 15, sel=sel)
    lims, D, I = idx.range_search_probed(q, -INF, sel=sel)
    for i in (0, 64, 129):
        one_k = idx.search(q[i:i + 1], 15, sel=sel)
        assert same_topk(one_k, (Dk[i:i + 1], Ik[i:i + 1]))
        one_r = idx.range_search_probed(q[i:i + 1], -INF, sel=sel)
        a, b = int(lims[i]), int(lims[i + 1])
        assert same_range(one_r, (np.array([0, b - a]), host(D[a:b]), host(I[a:b])))
    assert errors() == 0


# ---- 7. graph capture: the filter is data -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_a_captured_filtered_search_replays_under_the_selector_as_it_stands(fam):
    S = store(fam, True, 32)
    idx = S.index(3)
    q = dev(S.q[:16])
    rng = np.random.default_rng(8)
    m1, m2 = rng.random(S.n) < 0.5, rng.random(S.n) < 0.1
    sel = selector(m1)
    k = 12
    want1 = tuple(t.clone() for t in idx.search(q, k, sel=sel))              # (eager: the workspaces exist before the capture starts)
    want2 = tuple(t.clone() for t in idx.search(q, k, sel=selector(m2)))
    assert not same_topk(want1, want2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        idx.search(q, k, sel=sel)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Dg, Ig = idx.search(q, k, sel=sel)
    graph.replay()
    torch.cuda.synchronize()
    assert same_topk((Dg, Ig), want1)
    p = sel.words.data_ptr()
    sel.set_mask_(m2)
    assert sel.words.data_ptr() == p
    graph.replay()
    torch.cuda.synchronize()
    assert same_topk((Dg, Ig), want2)
    sel.set_rows_(torch.from_numpy(np.flatnonzero(m1)))
    graph.replay()
    torch.cuda.synchronize()
    assert same_topk((Dg, Ig), want1)
    assert errors() == 0


# ---- 8. refusals, empty inputs, the wrapper -------------------------------------------------------------------------------------------------------
def test_the_index_refuses_what_is_not_its_selector_and_empty_inputs_return_what_they_return_today():
    from lightretriever_amd import FlatIPIndex, IVFFlatIndex, RowSelector
    from lightretriever_amd.retriever import FaissIndex
    d, nlist = 32, 4
    rng = np.random.default_rng(9)
    x = dev(rng.standard_normal((200, d)).astype(F32))
    q = x[:3] + 0.25
    idx = IVFFlatIndex(d, nlist, nprobe=2)
    idx.train(x, niter=1)
    idx.add(x[:150])
    sel = RowSelector.from_range(10, 90, 150)
    got = idx.search(q, 5, sel=sel)
    assert (((got[1] >= 10) & (got[1] < 90)) | (got[1] == -1)).all() and (got[1][:, 0] >= 0).all()
    probes = idx.quantizer.search(q, 2)[1]
    assert same_range(idx.range_search_preassigned(q, -INF, probes, sel=sel), idx.range_search_probed(q, -INF, sel=sel))
    idx.add(x[150:])
    for call in (lambda s: idx.search(q, 5, sel=s), lambda s: idx.range_search_probed(q, 0.0, sel=s),
                 lambda s: idx.range_search_preassigned(q, 0.0, probes, sel=s)):
        with pytest.raises(ValueError, match="150.*200"):                    # made before the later add()
            call(sel)
        with pytest.raises(TypeError, match="RowSelector"):
            call(torch.ones(200, dtype=torch.bool, device="cuda"))
        with pytest.raises(TypeError, match="RowSelector"):
            call(sel.words)
    elsewhere = RowSelector(200)
    elsewhere.words = elsewhere.words.cpu()                                  # (one GPU is enough to stand for "another device")
    with pytest.raises(ValueError, match="cpu"):
        idx.search(q, 5, sel=elsewhere)
    with pytest.raises(ValueError, match="GPU"):
        RowSelector(5, device="cpu")
    sel = RowSelector.from_range(10, 90, 200)
    # empty inputs
    e = idx.search(q[:0], 5, sel=sel)
    assert e[0].shape == (0, 5) and e[1].shape == (0, 5)
    e = idx.range_search_probed(q[:0], 0.0, sel=sel)
    assert e[0].tolist() == [0] and e[1].numel() == 0
    empty = IVFFlatIndex(d, nlist, nprobe=2)
    empty.train(x, niter=1)
    none = empty.search(q, 5, sel=RowSelector(0))
    assert same_topk(none, empty.search(q, 5)) and (none[1] == -1).all()
    e = empty.range_search_probed(q, 0.0, sel=RowSelector(0))
    assert e[0].tolist() == [0, 0, 0, 0]
    # the wrapper: other index classes are refused by name; passage ids are applied to the filtered rows
    flat = FlatIPIndex(d)
    flat.add(x)
    with pytest.raises(TypeError, match="FlatIPIndex"):
        FaissIndex(flat).search(q, 5, sel=sel)
    with pytest.raises(TypeError, match="FlatIPIndex"):
        FaissIndex(flat).range_search_probed(q, 0.0, sel=sel)
    pids = (np.arange(200, dtype=np.int64)[::-1] * 10 + 7)
    fi = FaissIndex(idx, pids.tolist())
    D, I = idx.search(q, 100, sel=sel)
    fD, fI = fi.search(q, 100, sel=sel)
    assert (I[:, -1] == -1).all() and (I[:, 0] >= 0).all()                   # 80 selected rows: the tail is padding, and stays -1
    assert torch.equal(fD, D) and torch.equal(fI, torch.where(I >= 0, dev(pids)[I.clamp(min=0)], I))
    r, fr = idx.range_search_probed(q, -INF, sel=sel), fi.range_search_probed(q, -INF, sel=sel)
    assert torch.equal(fr[0], r[0]) and torch.equal(fr[1], r[1]) and torch.equal(fr[2], dev(pids)[r[2]])
    assert same_topk(fi.search(q, 7), (idx.search(q, 7)[0], dev(pids)[idx.search(q, 7)[1]]))        # without sel: as before
    assert errors() == 0
