"""GPU: the integer machinery every inverted-file search starts with (lrx_search_ivf.h: k_ivf_plan<false / true>, k_ivf_items, k_pairs_scatter, the
binary search of ivf_scan_items; lrx_search_ivfpq.h: the slot table of k_ivf_pq_scan) at the probe and cell counts include/lrx.h allows -- up to
2048 probe entries, thousands of cells -- where the other inverted-file tests stay at 64 entries and a few hundred cells ("The plan at scale").

The observable is the range search at radius -inf: it returns every scanned row in segment order (cells in probe order, rows by stored
position), so a wrong segment offset, a lost pair or a mis-located work item is a wrong lims, a wrong row or a wrong position.  Every comparison
is on bits -- scores as int32 views, ids and lims equal, the device error count exact -- against the numpy yardsticks, over the data recipes of
ivf_store.Store under which they give the library's bits.  A case calls its family's yardstick search ONCE, at k = n
(ivf_plan_cases.CachedSearch): its head is the top k for every k, ivf_range_yardstick.expected over it is every range result."""
import numpy as np
import pytest
import torch

import ivf_plan_cases as PC
import ivf_range_yardstick as R
import ivf_yardstick as IV
from ivf_store import F32, FAMILIES, SEARCH, Store, dev, errors, partial, quarters, same, same_slice

pytestmark = pytest.mark.gpu

CELL_MAJOR = ("flat", "sq_fp16", "sq8")                                      # the families of ivf_cell_major_search (pairs, work items)
Q_BIG = 130
LADDER = (64, 65, 128, 255, 256, 257, 511, 1024, 1025, 2047, 2048)
_STORES = {}


def big(fam):
    """The family's store of 2500 cells (ivf_plan_cases.scale_sizes) with 130 queries; the cases with fewer take the first of them."""
    if fam not in _STORES:
        _STORES[fam] = Store(fam, PC.scale_sizes(), Q=Q_BIG)
        assert _STORES[fam].sizes[0] == 0 and 6000 <= _STORES[fam].n <= 8000
    return _STORES[fam]


def base_for(S, shape, rng):
    """Store.base's recipe from the case's own generator (the store's is shared between tests)."""
    if not S.by_residual:
        return None
    return (3 * rng.standard_normal(shape)).astype(F32) if S.fam == "pq" else quarters(rng, shape)


def reference(S, probes, base, q, max_scan=None):
    return PC.CachedSearch(SEARCH[S.fam], (q,) + S.head, S.list_off, S.row_ids, probes, base, S.by_residual, max_scan_rows=max_scan)


def topk(S, how, probes, base, k, q, max_scan=None):
    """torch.ops.lrx.ivf_*_ip_topk (how = "op") or ops.ivf_*_ip_topk ("ops"): Store's range arguments with k for the radius."""
    a = S._op_args(probes, base, 0.0, max_scan, q, 0, None)
    a = a[:-4] + (int(k),) + a[-3:]
    if how == "op":
        from lightretriever_amd import torch_ops
        torch_ops.load()
        return getattr(torch.ops.lrx, f"ivf_{S.fam}_ip_topk")(*a)
    from lightretriever_amd import ops
    return getattr(ops, f"ivf_{S.fam}_ip_topk")(*a)


def same_topk(got, want):
    D, I = got[0].cpu().numpy(), got[1].cpu().numpy()
    return D.shape == want[0].shape and np.array_equal(D.view(np.int32), want[0].view(np.int32)) and np.array_equal(I, want[1])


def topk_both(S, ref, probes, base, k, q, max_scan=None):
    got = topk(S, "op", probes, base, k, q, max_scan)
    assert same_topk(got, ref.topk(k))
    assert same_topk(topk(S, "ops", probes, base, k, q, max_scan), ref.topk(k))
    return got


def range_all(S, ref, probes, base, radius, q, max_scan=None):
    """The C call, the torch op and ops.py, each against the cached yardstick -> the C call's result."""
    want = ref.range(radius)
    got = S.c_trim(probes, base, radius, q=q, max_scan=max_scan)
    assert same(got, want)
    assert same(S.op(probes, base, radius, q=q, max_scan=max_scan), want)
    assert same(S.ops(probes, base, radius, q=q, max_scan=max_scan), want)
    return got


def range_calls(ref, radius):
    """The library calls range_all makes: the C call, and from the op and from ops.py one call, or two where the result is longer than their
    first guess of 1024 hits per query (index._range_call: the call is repeated with outputs of the size lims reports).  Every call counts
    its bad entries and its queries over the bound."""
    retry = int(ref.range(radius)[0][-1]) > 1024 * len(ref.probes)
    return 1 + 2 * (2 if retry else 1)


# ---- 1. the nprobe ladder: runs of 1 .. 8 entries per thread of k_ivf_plan, one to four waves with entries, one and two trips of the slot-table load ----
@pytest.mark.parametrize("nprobe", LADDER)
@pytest.mark.parametrize("fam", FAMILIES)
def test_the_nprobe_ladder(fam, nprobe):
    S = big(fam)
    rng = np.random.default_rng(1000 + nprobe)
    q = S.q[:6]
    probes = PC.prefix_probes(rng, 6, nprobe, np.arange(S.nlist))
    assert (np.array(S.sizes)[probes] == 0).any()                            # empty cells are named
    base = base_for(S, probes.shape, rng)
    ref = reference(S, probes, base, q)
    errors()
    for k in (10, 2048):
        topk_both(S, ref, probes, base, k, q)
    every = range_all(S, ref, probes, base, -np.inf, q)
    assert np.array_equal(np.diff(every[0].cpu().numpy()), ref.scanned()) and (ref.scanned() > 0).all()
    radius = ref.median()
    range_all(S, ref, probes, base, radius, q)
    assert partial(ref.range(radius)[0], ref.scanned())
    assert errors() == 0


# ---- 2. crafted skip patterns at nprobe = 2048: a thread of the plan owns 8 entries, a wave 512 ------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_crafted_skip_patterns(fam):
    """The rows a .. g of ivf_plan_cases.crafted_probes (tests/test_ivf_plan_scale_host.py states what each holds).  The error count of a call
    is the number of its entries >= nlist; with those entries replaced by -1 the bits are the same and the count is 0."""
    S = big(fam)
    rng = np.random.default_rng(2000)
    probes = PC.crafted_probes(S.sizes)
    q = S.q[:len(probes)]
    nbad = int((probes >= S.nlist).sum())
    assert nbad > 0
    base = base_for(S, probes.shape, rng)
    ref = reference(S, probes, base, q)
    scanned = ref.scanned()
    assert scanned[4] == scanned[5] == 129 and scanned[6] == 0 and (scanned[:4] > 2048).all()
    errors()
    tops = {}
    for k in (10, 2048):
        tops[k] = topk_both(S, ref, probes, base, k, q)
        assert errors() == 2 * nbad
    assert (tops[10][1][6] == -1).all()                                      # g: all padding
    every = range_all(S, ref, probes, base, -np.inf, q)
    assert errors() == range_calls(ref, -np.inf) * nbad
    lims = every[0].cpu().numpy()
    assert np.array_equal(np.diff(lims), scanned) and lims[7] == lims[6]     # g: lims flat
    radius = ref.median()
    got = range_all(S, ref, probes, base, radius, q)
    assert errors() == range_calls(ref, radius) * nbad and partial(ref.range(radius)[0], scanned)
    # the neighbours of the bad entries are what they are without them
    clean = np.where(probes >= S.nlist, -1, probes)
    assert same(S.c_trim(clean, base, radius, q=q), got) and same(S.c_trim(clean, base, -np.inf, q=q), every)
    for k in (10, 2048):
        again = topk(S, "op", clean, base, k, q)
        assert torch.equal(again[1], tops[k][1]) and torch.equal(again[0].view(torch.int32), tops[k][0].view(torch.int32))
    assert errors() == 0


# ---- 3. the scan bound at many probes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_one_row_over_the_scan_bound_at_1500_probes(fam):
    S = big(fam)
    rng = np.random.default_rng(3000)
    q = S.q[:6]
    probes, scanned = PC.largest_first(PC.prefix_probes(rng, 6, 1500, np.arange(S.nlist)), S.list_off)
    bound = int(scanned[0]) - 1                                              # query 0 alone is over it
    base = base_for(S, probes.shape, rng)
    ref, free = reference(S, probes, base, q, max_scan=bound), reference(S, probes, base, q)
    assert ref.scanned().tolist() == [0] + scanned[1:].tolist()
    errors()
    for k in (10, 2048):
        got = topk_both(S, ref, probes, base, k, q, max_scan=bound)
        assert errors() == 2                                                 # query 0, once per call
        assert (got[1][0] == -1).all() and (got[0][0] == -float(IV.FLT_MAX)).all()
        D, I = free.topk(k)
        assert np.array_equal(got[1][1:].cpu().numpy(), I[1:]) and np.array_equal(got[0][1:].cpu().numpy().view(np.int32), D[1:].view(np.int32))
    whole = S.c_trim(probes, base, -np.inf, q=q)
    assert errors() == 0
    for radius in (-np.inf, free.median()):
        got = range_all(S, ref, probes, base, radius, q, max_scan=bound)
        assert errors() == range_calls(ref, radius)                           # query 0, once per call
        assert int(got[0][1]) == 0
    assert partial(got[0], ref.scanned())
    short = S.c_trim(probes, base, -np.inf, q=q, max_scan=bound)
    assert all(same_slice(short, i, whole, i) for i in range(1, 6))          # every other query keeps its bits
    assert errors() == 1


# ---- 4. more than 262 144 pairs in one chunk: the grid-stride loop of k_pairs_scatter ---------------------------------------------------------
@pytest.mark.parametrize("fam", CELL_MAJOR)
def test_more_pairs_than_the_scatter_grid_has_threads(fam):
    """130 queries x 2048 distinct non-empty cells: 266 240 pairs in one chunk, past the 1024 x 256 threads of k_pairs_scatter's grid.  (The
    PQ family is not here: its query-major scan emits no pairs.)  The C call gets a zero-filled workspace: a pair the scatter dropped leaves
    null words -- missing rows, not an earlier call's correct-looking answer -- and no stale slot is ever turned into an address."""
    S = big(fam)
    rng = np.random.default_rng(4000)
    probes = PC.prefix_probes(rng, Q_BIG, 2048, np.flatnonzero(np.diff(S.list_off) > 0))
    assert (np.diff(S.list_off)[probes] > 0).all() and all(len(set(r)) == 2048 for r in probes.tolist()) and probes.size > 262144
    base = base_for(S, probes.shape, rng)
    ref = reference(S, probes, base, S.q)
    errors()
    every = S.c_trim(probes, base, -np.inf, q=S.q, fill=torch.zeros)
    assert same(every, ref.range(-np.inf))
    radius = ref.median()
    whole = S.c_trim(probes, base, radius, q=S.q, fill=torch.zeros)
    assert same(whole, ref.range(radius)) and partial(ref.range(radius)[0], ref.scanned())
    assert same_topk(topk(S, "op", probes, base, 100, S.q), ref.topk(100))
    for i in (0, 63, 64, 128, 129):                                          # a query alone gives its rows of the batch
        alone = S.c_trim(probes[[i]], None if base is None else base[[i]], radius, q=S.q[[i]], fill=torch.zeros)
        assert same_slice(alone, 0, whole, i)
    assert errors() == 0


# ---- 5. the edges of k_ivf_items: 1024 threads over nlist + 1 entries ------------------------------------------------------------------------
@pytest.mark.parametrize("nlist", [1023, 1024, 1025])
@pytest.mark.parametrize("fam", CELL_MAJOR)
def test_the_item_scan_around_1024_cells(fam, nlist):
    """nlist + 1 = 1024 entries are one per thread; 1025 and 1026 are runs of two.  The 129-row (two-item) last cell and the entry c == nlist
    that closes the scans sit on threads 1022 | 1023, on 511 | 512 and together on 512; the threads past them own nothing."""
    S = Store(fam, PC.edge_sizes(nlist), seed=nlist)
    rng = np.random.default_rng(5000 + nlist)
    probes = PC.with_cell(PC.prefix_probes(rng, 6, 300, np.arange(nlist)), nlist - 1, [0, 2, 5], rng)
    base = base_for(S, probes.shape, rng)
    ref = reference(S, probes, base, S.q)
    assert (probes[[0, 2, 5]] == nlist - 1).any(axis=1).all() and (np.array(S.sizes)[probes] == 0).any()
    errors()
    every = range_all(S, ref, probes, base, -np.inf, S.q)
    assert np.array_equal(np.diff(every[0].cpu().numpy()), ref.scanned())
    topk_both(S, ref, probes, base, 50, S.q)
    assert errors() == 0


# ---- 6. the index classes at many probes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_the_index_hands_1500_probes_to_the_op(fam):
    """The Python path up to the kernels and nothing more: the index's search and range_search_probed are the op called with the index
    quantiser's own probe lists and scores, and those lists are the yardstick's.  (The kernels are held to the yardsticks above.)"""
    S = big(fam)
    idx = S.index(nprobe=1500)
    hq = S.q[:6]
    q = dev(hq)
    coarse, probes = idx.quantizer.search(q, 1500)
    assert np.array_equal(probes.cpu().numpy(), IV.probe_lists(hq, S.cent, 1500))
    hp, hb = probes.cpu().numpy(), coarse.cpu().numpy() if S.by_residual else None
    bound = idx.max_scan_rows()
    errors()
    D, I = idx.search(q, 100)
    want = topk(S, "op", hp, hb, 100, hq, max_scan=bound)
    assert torch.equal(I, want[1]) and torch.equal(D.view(torch.int32), want[0].view(torch.int32)) and (I >= 0).all()
    radius = float(D[:, 50].median())
    got = idx.range_search_probed(q, radius)
    assert same(got, S.op(hp, hb, radius, q=hq, max_scan=bound))
    assert partial(got[0], R.scanned_rows(hp, S.list_off))
    assert errors() == 0
