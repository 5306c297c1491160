"""GPU: range search over the probed cells of the four inverted-file indexes (lrx_ivf_*_ip_range_search, torch.ops.lrx.ivf_*_ip_range_search,
ops.ivf_*_ip_range_search, range_search_probed / range_search_preassigned, FaissIndex.range_search_probed) against the numpy
yardstick (tests/ivf_range_yardstick.py), the indexes' own search and the flat range search.  Every comparison is on bits: lims equal, D as
int32 views, I equal.  Every test asserts from the yardstick that some query has a hit count strictly between 0 and the rows it scans."""
import numpy as np
import pytest
import torch

import ivf_range_yardstick as R
from ivf_store import FILL_D, FILL_I, FAMILIES, M_PQ, F32, Store, dev, errors, partial, same, same_slice, slices

pytestmark = pytest.mark.gpu



# nine cells: empty, 1, 7, 9 rows, one under / at / over the fill's 1024-word tile, one past the 2048-word mark, one more
SIZES = [0, 1, 7, 9, 1023, 1024, 1025, 2500, 300]
NLIST = len(SIZES)
_STORES = {}


def store(fam, by_residual=True):
    key = (fam, by_residual)
    if key not in _STORES:
        _STORES[key] = Store(fam, SIZES, by_residual=by_residual)
    return _STORES[key]


# ---- 1. hand-made cells: the C call, the op and ops.py against the yardstick -----------------------------------------------------------------------
PROBES = np.array([[7, 4, 0, 2], [5, 5, 3, -1], [6, NLIST, 1, 2 ** 40], [8, 6, 5, 4], [0, 0, -1, -1], [1, 2, 3, 8]], np.int64)
TOTALS = [2500 + 1023 + 7, 1024 + 9, 1025 + 1, 300 + 1025 + 1024 + 1023, 0, 1 + 7 + 9 + 300]


@pytest.mark.parametrize("fam", FAMILIES)
def test_hand_made_cells_against_the_yardstick(fam):
    S = store(fam)
    base = S.base(PROBES.shape)
    assert R.scanned_rows(PROBES, S.list_off).tolist() == TOTALS
    radius = S.median(PROBES, base)
    errors()
    got, want = S.all(PROBES, base, radius)
    assert errors() == 3 * 2                                                 # query 2's two entries past nlist, in each of the three calls
    assert partial(want[0], TOTALS)
    assert int(got[0][5]) == int(got[0][4])                                  # query 4 names the empty cell and padding alone
    # the neighbours of the bad entries are what they are without them
    clean = PROBES.copy()
    clean[2] = [6, -1, 1, -1]
    ref = S.c_trim(clean, base, radius)
    assert errors() == 0 and same(ref, got)
    # one row short for query 0: it has no hits and is counted, the others keep their slices
    short = S.all(PROBES, base, radius, max_scan=TOTALS[0] - 1)[0]
    assert errors() == 3 * (2 + 1)
    assert int(short[0][1]) == 0 and all(same_slice(short, i, got, i) for i in range(1, 6))
    assert partial(short[0], R.scanned_rows(PROBES, S.list_off, TOTALS[0] - 1))
    # ids: id_base and row_map
    rm = dev(np.arange(S.n, dtype=np.int64) * 3 + 11)
    S.all(PROBES, base, radius, id_base=1000)
    mapped, _ = S.all(PROBES, base, radius, row_map=rm)
    assert torch.equal(mapped[2], got[2] * 3 + 11)
    errors()


# ---- 2. strictness, signed zero, infinities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["flat", "sq8"])
def test_a_score_equal_to_the_radius_is_no_hit_and_zero_has_no_sign(fam):
    S = store(fam, by_residual=False)                                        # (flat: no residuals anyway; sq8: codes on the exact grid)
    probes = PROBES[[0, 1, 3, 5]]
    q = S.q[:4]
    every = S.want(probes, None, -np.inf, q=q)
    scanned = R.scanned_rows(probes, S.list_off)
    assert np.array_equal(np.diff(every[0]), scanned)
    sc = np.sort(np.unique(every[1]))
    v = sc[len(sc) // 2]                                                     # an attained score with scores on both sides
    nxt = sc[len(sc) // 2 + 1]
    assert (every[1] == v).sum() >= 1 and nxt > v
    got, want = S.all(probes, None, float(v), q=q)
    D = got[1].cpu().numpy()
    assert partial(want[0], scanned)
    assert len(D) == int((every[1] > v).sum()) and D.min() == nxt and not (D == v).any()
    # just under the attained score: the rows at it are in
    under = np.nextafter(v, F32(-np.inf), dtype=F32)
    got2, _ = S.all(probes, None, float(under), q=q)
    assert len(got2[1]) == len(D) + int((every[1] == v).sum())
    # the infinities
    assert int(S.all(probes, None, np.inf, q=q)[0][0][-1]) == 0
    assert same(S.all(probes, None, -np.inf, q=q)[0], every)
    # an all-zero query scores zero on every row
    z = np.zeros_like(q)
    assert int(S.all(probes, None, 0.0, q=z)[0][0][-1]) == 0
    assert int(S.all(probes, None, -0.0, q=z)[0][0][-1]) == 0
    allz, _ = S.all(probes, None, -1.0, q=z)
    assert np.array_equal(np.diff(allz[0].cpu().numpy()), scanned) and (allz[1] == 0).all()
    assert errors() == 0


# ---- 3. consistency with search and with the flat range search ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_the_range_result_is_the_search_result_above_the_radius(fam):
    S = store(fam)
    idx = S.index(3)
    q = dev(S.q)
    coarse, probes = idx.quantizer.search(q, 3)
    scanned = R.scanned_rows(probes.cpu().numpy(), S.list_off)
    small = [i for i in range(len(S.q)) if scanned[i] <= 2048]
    assert small and (scanned > 0).all()
    base = coarse.cpu().numpy() if S.by_residual else None
    radius = S.median(probes.cpu().numpy(), base)
    res = idx.range_search_probed(q, radius)
    want = S.want(probes.cpu().numpy(), base, radius)
    assert same(res, want) and partial(want[0], scanned)
    Dk, Ik = idx.search(q, 2048)
    for i in small:
        keep = Dk[i] > radius
        assert (Ik[i][keep] >= 0).all()
        d_r, i_r = slices(res, i)
        o_r, o_k = torch.argsort(i_r), torch.argsort(Ik[i][keep])
        assert torch.equal(i_r[o_r], Ik[i][keep][o_k]) and torch.equal(d_r[o_r].view(torch.int32), Dk[i][keep][o_k].view(torch.int32))
    assert errors() == 0


def test_probing_every_cell_is_the_flat_range_search_after_sorting_by_id():
    from lightretriever_amd import FlatIPIndex
    S = store("flat")
    idx = S.index(NLIST)
    flat = FlatIPIndex(S.d)
    flat.add(dev(S.x))
    q = dev(S.q)
    probes = idx.quantizer.search(q, NLIST)[1].cpu().numpy()
    radius = S.median(probes, None)
    lims, D, I = idx.range_search_probed(q, radius)
    want = S.want(probes, None, radius)
    assert same((lims, D, I), want) and partial(want[0], [S.n] * len(S.q))
    fl, fD, fI = flat.range_search(q, radius)
    assert torch.equal(lims, fl)
    ascending = True
    for i in range(len(S.q)):
        d_r, i_r = slices((lims, D, I), i)
        o = torch.argsort(i_r)
        ascending &= bool((o == torch.arange(len(o), device="cuda")).all())
        assert torch.equal(i_r[o], slices((fl, fD, fI), i)[1]) and torch.equal(d_r[o].view(torch.int32), slices((fl, fD, fI), i)[0].view(torch.int32))
    assert not ascending                                                     # segment order is not the flat search's ascending-row order


# ---- 4. the capacity protocol through the C call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_outputs_are_written_only_where_they_fit_and_lims_is_always_exact(fam):
    S = store(fam)
    base = S.base(PROBES.shape)
    radius = S.median(PROBES, base)
    want = S.want(PROBES, base, radius)
    total = int(want[0][-1])
    assert total > 1 and partial(want[0], TOTALS)
    lims, D, I = S.c(PROBES, base, radius, capacity=total - 1)
    assert np.array_equal(lims.cpu().numpy(), want[0]) and (D == FILL_D).all() and (I == FILL_I).all()
    lims, D, I = S.c(PROBES, base, radius, capacity=total)
    assert same((lims, D, I), want)
    lims, D, I = S.c(PROBES, base, radius, capacity=0)
    assert np.array_equal(lims.cpu().numpy(), want[0]) and (D == FILL_D).all() and (I == FILL_I).all()
    lims, D, I = S.c(PROBES, base, np.inf, capacity=0, null_out=True)         # no hits, no room, no output arrays: LRX_OK
    assert (lims == 0).all()
    errors()


# ---- 5. two chunks, the lims carry, batch independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_a_query_gives_the_same_slice_alone_first_of_two_and_inside_two_chunks(fam):
    Q = 1030                                                                 # more than the 1024 queries of a chunk
    S = Store(fam, [260, 1, 0, 300, 250, 513, 130, 546], d=32, Q=Q, seed=5)
    assert S.n == 2000
    rng = np.random.default_rng(3)
    probes = np.stack([rng.permutation(S.nlist)[:3] for _ in range(Q)]).astype(np.int64)
    base = S.base(probes.shape)
    picks = [0, 1, 511, 1023, 1024, 1029]                                    # both sides of the chunk boundary
    sub = lambda a, rows: None if a is None else a[rows]
    radius = S.median(probes[picks], sub(base, picks), q=S.q[picks])
    whole = S.c_trim(probes, base, radius)
    assert int(whole[0][0]) == 0 and (np.diff(whole[0].cpu().numpy()) >= 0).all()
    want = S.want(probes[picks], sub(base, picks), radius, q=S.q[picks])
    assert partial(want[0], R.scanned_rows(probes[picks], S.list_off))
    for j, i in enumerate(picks):
        d_w, i_w = slices(whole, i)
        a, b = int(want[0][j]), int(want[0][j + 1])
        assert np.array_equal(i_w.cpu().numpy(), want[2][a:b]) and np.array_equal(d_w.cpu().numpy().view(np.int32), want[1][a:b].view(np.int32))
        alone = S.c_trim(probes[[i]], sub(base, [i]), radius, q=S.q[[i]])
        pair = S.c_trim(probes[[i, (i + 7) % Q]], sub(base, [i, (i + 7) % Q]), radius, q=S.q[[i, (i + 7) % Q]])
        assert same_slice(alone, 0, whole, i) and same_slice(pair, 0, whole, i)
    # the op and ops.py over both chunks
    assert same(S.op(probes, base, radius), whole) and same(S.ops(probes, base, radius), whole)
    assert errors() == 0


# ---- 6. the index layer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam, by_residual", [("flat", True), ("sq_fp16", True), ("sq_fp16", False), ("sq8", True), ("sq8", False), ("pq", True), ("pq", False)])
def test_probed_equals_preassigned_with_the_quantisers_own_cells(fam, by_residual, tmp_path):
    from lightretriever_amd import _lib
    from lightretriever_amd.retriever import FaissIndex
    S = store(fam, by_residual)
    idx = S.index(2, id_base=500)
    q = dev(S.q)
    for nprobe in (None, 4):                                                 # the index's own nprobe, and this call's
        coarse, probes = idx.quantizer.search(q, nprobe or 2)
        base = coarse.cpu().numpy() if S.by_residual else None
        radius = S.median(probes.cpu().numpy(), base)
        want = S.want(probes.cpu().numpy(), base, radius, id_base=500)
        assert partial(want[0], R.scanned_rows(probes.cpu().numpy(), S.list_off))
        got = idx.range_search_probed(q, radius, nprobe)
        assert same(got, want)
        assert same(idx.range_search_preassigned(q, radius, probes, coarse), got)
        assert same(idx.range_search_preassigned(S.q, radius, probes[:, [1, 0] + list(range(2, probes.shape[1]))], coarse[:, [1, 0] + list(range(2, probes.shape[1]))]),
                    S.want(probes.cpu().numpy()[:, [1, 0] + list(range(2, probes.shape[1]))],
                           None if base is None else base[:, [1, 0] + list(range(2, probes.shape[1]))], radius, id_base=500))
    # row_map replaces id_base; passage ids go through FaissIndex
    rm = dev(np.arange(S.n, dtype=np.int64) * 2 + 1)
    mapped = idx.range_search_probed(q, radius, 4, row_map=rm)
    assert torch.equal(mapped[0], got[0]) and torch.equal(mapped[2], (got[2] - 500) * 2 + 1) and torch.equal(mapped[1].view(torch.int32), got[1].view(torch.int32))
    plain = S.index(4)
    pids = np.arange(S.n, dtype=np.int64)[::-1] * 10
    f = FaissIndex(plain, pids.tolist()).range_search_probed(q, radius)
    assert torch.equal(f[0], got[0]) and torch.equal(f[2], dev(pids)[got[2] - 500]) and torch.equal(f[1].view(torch.int32), got[1].view(torch.int32))
    # a saved file gives the same result
    fname = str(tmp_path / "index.faiss")
    idx.save(fname)
    assert same(type(idx).load(fname, id_base=500).range_search_probed(q, radius, 4), got)
    # refusals: NaN, a residual index without probe_scores, graph capture; empty inputs give the empty triple
    with pytest.raises(ValueError, match="NaN"):
        idx.range_search_probed(q, float("nan"))
    if S.by_residual:
        with pytest.raises(ValueError, match="probe_scores"):
            idx.range_search_preassigned(q, radius, probes)
    else:
        assert same(idx.range_search_preassigned(q, radius, probes), got)      # ignored or not needed
    with pytest.raises(ValueError, match="probes"):
        idx.range_search_preassigned(q, radius, probes.to(torch.int32), coarse)
    for call in (lambda: idx.range_search_probed(q, radius), lambda: idx.range_search_preassigned(q, radius, probes, coarse)):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.LrxError, match="graph capture"):
            with torch.cuda.graph(g):
                call()
        del g
    torch.cuda.synchronize()
    assert same(idx.range_search_probed(q, radius, 4), got)                  # the stream is usable afterwards
    e = idx.range_search_probed(q[:0], radius)
    assert e[0].tolist() == [0] and e[1].numel() == 0 and e[2].numel() == 0
    with pytest.raises(NotImplementedError, match="range_search"):
        idx.range_search(q, radius)
    assert errors() == 0


@pytest.mark.parametrize("fam", FAMILIES)
def test_rows_added_after_a_range_search_are_found_by_the_next(fam):
    import lightretriever_amd as A
    d, nlist, n = 64, 6, 1500
    rng = np.random.default_rng(11)
    centres = 4 * rng.standard_normal((nlist, d))
    x = dev((centres[rng.integers(0, nlist, n)] + rng.standard_normal((n, d))).astype(F32))
    q = x[:5] + 0.5
    make = {"flat": lambda: A.IVFFlatIndex(d, nlist, nprobe=2), "sq_fp16": lambda: A.IVFSQIndex(d, nlist, nprobe=2), "sq8": lambda: A.IVFSQ8Index(d, nlist, nprobe=2),
            "pq": lambda: A.IVFPQIndex(d, nlist, M_PQ, nprobe=2)}[fam]
    pieces, once = make(), make()
    for idx in (pieces, once):
        idx.train(x, niter=2)
    once.add(x)
    Dk, _ = once.search(q, 100)
    radius = float(Dk[:, 50].median())
    pieces.add(x[:700])
    first = pieces.range_search_probed(q, radius)
    pieces.add(x[700:])
    got = pieces.range_search_probed(q, radius)
    want = once.range_search_probed(q, radius)
    assert same(got, want) and int(first[0][-1]) < int(got[0][-1])
    # the yardstick's view of the hit counts: between none and everything scanned
    probes = once.quantizer.search(q, 2)[1].cpu().numpy()
    scanned = R.scanned_rows(probes, once.list_off.cpu().numpy())
    assert partial(got[0], scanned)
    # and what search reports above the radius is in it
    Dk, Ik = once.search(q, 100)
    for i in range(5):
        keep = Dk[i] > radius
        d_r, i_r = slices(got, i)
        assert set(Ik[i][keep].tolist()) <= set(i_r.tolist())
    assert errors() == 0
