"""GPU: the inverted-file fp16 scalar-quantised index (lrx_ivf_sq_fp16_ip_search, lrx_ivf_sq_fp16_encode_rows, torch.ops.lrx.ivf_sq_fp16_ip_topk,
ops.ivf_sq_fp16_ip_topk, IVFSQIndex, IVFSQFaissSearch) against the numpy yardstick (tests/ivfsq_yardstick.py), SQFp16Index, IVFFlatIndex and
RefineFlatIndex, bit for bit: without residuals and probing every cell it is the fp16 flat search; hand-made cells around the row group of the
scan with every kind of bad probe entry; ties; batch independence; the codes; the life cycle; nesting of the probe sets; persistence, HIP graph,
the searcher and the refine route.  Where the comparison is with the yardstick the data are small integers, centroids included, and hand-given
probe scores are quarters: every fp64 sum is exact in any order.  Observed figures: DESIGN §5.4.12."""
import numpy as np
import pytest
import torch

import ivf_yardstick as IV
import ivfsq_yardstick as Y

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.view(torch.int32)


def bits16(t):
    return t.view(torch.int16)


def assert_same(got, want):
    assert torch.equal(got[1], want[1])
    assert torch.equal(bits(got[0]), bits(want[0]))


def assert_yardstick(got, want):
    D, I = got
    assert np.array_equal(I.cpu().numpy(), want[1])
    assert np.array_equal(D.cpu().numpy().view(np.int32), want[0].view(np.int32))


def errors(reset=True):
    from lightretriever_amd import _lib
    torch.cuda.synchronize()
    return int(_lib.lib().lrx_device_error_count(1 if reset else 0))


def group_rows(d):
    from lightretriever_amd import _lib
    return int(_lib.lib().lrx_ivf_sq_fp16_group_rows(d))


def _args(q, codes, list_off, row_ids, probes, base):
    q, codes, list_off, probes = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, codes, list_off, probes))
    row_ids = row_ids if row_ids is None or isinstance(row_ids, torch.Tensor) else dev(row_ids)
    base = base if base is None or isinstance(base, torch.Tensor) else dev(np.asarray(base, np.float32))
    return q.contiguous(), codes, list_off, row_ids, probes, base


def ivfsq_c(q, codes, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    """lrx_ivf_sq_fp16_ip_search through ctypes with ld_probe = nprobe + 3: the padding entries name cell 0 and carry a score of 1e30 (read,
    they would add that cell's rows or lift a score)."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    q, codes, list_off, row_ids, probes, base = _args(q, codes, list_off, row_ids, probes, base)
    (Q, D), n, npb, nlist = q.shape, codes.shape[0], probes.shape[1], list_off.numel() - 1
    pb = torch.zeros(Q, npb + 3, dtype=torch.int64, device="cuda")
    pb[:, :npb] = probes
    ps = None
    if base is not None:
        ps = torch.full((Q, npb + 3), 1e30, dtype=torch.float32, device="cuda")
        ps[:, :npb] = base
    Do = torch.full((Q, k), 7.5, dtype=torch.float32, device="cuda")
    Io = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(l.lrx_ivf_sq_fp16_ip_workspace_bytes(n, nlist, D, Q, npb, k, max_scan), dtype=torch.uint8, device="cuda")
    _lib.check(l.lrx_ivf_sq_fp16_ip_search(_lib.ptr(codes), n, D, _lib.ptr(list_off), _lib.ptr(row_ids), nlist, _lib.ptr(q), Q, _lib.ptr(pb), _lib.ptr(ps), npb,
                                           npb + 3, int(by_residual), max_scan, k, id_base, _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(row_map), _lib.ptr(ws),
                                           ws.numel(), _lib.current_stream()))
    torch.cuda.synchronize()
    return Do, Io


def ivfsq_op(q, codes, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    from lightretriever_amd import torch_ops
    torch_ops.load()
    q, codes, list_off, row_ids, probes, base = _args(q, codes, list_off, row_ids, probes, base)
    return torch.ops.lrx.ivf_sq_fp16_ip_topk(q, codes, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base, row_map)


def ivfsq_ops(q, codes, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    from lightretriever_amd import ops
    q, codes, list_off, row_ids, probes, base = _args(q, codes, list_off, row_ids, probes, base)
    return ops.ivf_sq_fp16_ip_topk(q, codes, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base, row_map)


def quarters(rng, shape):
    return (rng.integers(-12, 13, shape) / 4.0).astype(np.float32)


# ---- 1. without residuals, probing every cell: the fp16 flat index ---------------------------------------------------------------------
@pytest.mark.parametrize("Q, n, d, nlist, k", [(1, 500, 64, 4, 10), (5, 3000, 128, 16, 100), (130, 4000, 64, 8, 2048), (3, 600, 2112, 5, 50), (2, 40, 8192, 3, 7)])
def test_probing_every_cell_without_residuals_equals_the_fp16_index(Q, n, d, nlist, k):
    from lightretriever_amd import IVFSQIndex, SQFp16Index
    g = torch.Generator(device="cuda").manual_seed(n + d)
    x = torch.randn(n, d, generator=g, device="cuda")
    q = torch.randn(Q, d, generator=g, device="cuda")
    idx = IVFSQIndex(d, nlist, nprobe=nlist, by_residual=False)
    idx.train(x, niter=2)
    idx.add(x)
    sq = SQFp16Index(d)
    sq.add(x)
    assert idx.ntotal == n and int(idx.list_sizes.sum()) == n and idx.max_scan_rows() == n
    errors()
    got = idx.search(q, k)
    assert_same(got, sq.search(q, k))
    assert errors() == 0
    if Q * n <= 20000:       # the yardstick's ordered sum gives these bits on any data
        pr = idx.quantizer.search(q, nlist)[1]
        assert_yardstick(got, Y.search(q.cpu().numpy(), idx.stored_codes().cpu().numpy(), idx.list_off.cpu().numpy(), idx.row_ids.cpu().numpy(), pr.cpu().numpy(),
                                       None, False, k))


# ---- 2. hand-made cells -------------------------------------------------------------------------------------------------------------------
NLIST = 7


def cell_sizes(d):
    G = group_rows(d)
    s = [0, 1, G - 1, G, G + 1, 2 * G + 3]
    return s + [sum(s) + 50]                                                  # ... and one cell with more than half of the rows


class Cells:
    def __init__(self, d):
        rng = np.random.default_rng(d)
        self.sizes = cell_sizes(d)
        n = sum(self.sizes)
        cells = rng.permutation(np.repeat(np.arange(NLIST), self.sizes))
        self.d, self.n, self.rng, self.cells = d, n, rng, cells
        self.cent = rng.integers(-3, 4, (NLIST, d)).astype(np.float32)       # integers everywhere: every sum is exact, in any order
        self.x = rng.integers(-3, 4, (n, d)).astype(np.float32)
        self.q = rng.integers(-3, 4, (6, d)).astype(np.float32)
        self.row_ids, self.list_off = IV.cell_order(cells, NLIST)
        xs, cs = self.x[self.row_ids], cells[self.row_ids]
        self.stored = {False: Y.encode(xs), True: Y.encode(xs, self.cent, cs)}
        assert np.array_equal(Y.decode(self.stored[True], self.cent, cs), xs)
        self.dcodes = {b: dev(c) for b, c in self.stored.items()}
        self.dq, self.doff, self.dids = dev(self.q), dev(self.list_off), dev(self.row_ids)

    def all(self, probes, k, by_residual=True, base=None, max_scan=None, row_ids=True):
        """The C call, the torch op and ops over `probes`, each against the yardstick; returns the C call's result."""
        probes = np.asarray(probes, np.int64)
        if by_residual and base is None:
            base = quarters(self.rng, probes.shape)
        base = base if by_residual else None
        scan = self.n if max_scan is None else max_scan
        want = Y.search(self.q, self.stored[by_residual], self.list_off, self.row_ids if row_ids else None, probes, base, by_residual, k, max_scan_rows=max_scan)
        ids = self.dids if row_ids else None
        a = (self.dq, self.dcodes[by_residual], self.doff, ids, probes, base, by_residual, k, scan)
        got = ivfsq_c(*a)
        assert_yardstick(got, want)
        assert_yardstick(ivfsq_op(*a), want)
        assert_yardstick(ivfsq_ops(*a), want)
        return got, want

    def index(self, nprobe, by_residual, **kw):
        from lightretriever_amd import IVFSQIndex
        idx = IVFSQIndex(self.d, NLIST, nprobe=nprobe, by_residual=by_residual, **kw)
        idx.set_contents(self.cent, self.stored[by_residual], self.list_off, self.row_ids)
        return idx


@pytest.fixture(scope="module", params=[32, 64, 2048])
def cells(request):
    return Cells(request.param)


@pytest.mark.parametrize("by_residual", [True, False])
@pytest.mark.parametrize("nprobe", [1, 3, NLIST])
def test_hand_made_cells_against_the_yardstick(cells, nprobe, by_residual):
    probes = np.stack([cells.rng.permutation(NLIST)[:nprobe] for _ in range(6)])
    if nprobe == 1:
        probes[:, 0] = [6, 0, 1, 2, 4, 5]                                    # the large cell, the empty one, 1 row, G - 1, G + 1, 2 G + 3
    errors()
    got, _ = cells.all(probes, 10, by_residual)
    if nprobe == 1:
        assert (got[1][1] == -1).all() and (got[0][1] == -FLT_MAX).all()     # only the empty cell: all padding
        assert (got[1][2, 1:] == -1).all() and got[1][2, 0] >= 0             # one row, then padding
    # the index: the quantiser's own probe lists and scores (integer centroids: exact)
    idx = cells.index(nprobe, by_residual)
    ps, pr = idx.quantizer.search(cells.dq, nprobe)
    want = Y.search(cells.q, cells.stored[by_residual], cells.list_off, cells.row_ids, pr.cpu().numpy(), ps.cpu().numpy(), by_residual, 10)
    assert_yardstick(idx.search(cells.dq, 10), want)
    assert errors() == 0


# ---- 3. probe-list edges ------------------------------------------------------------------------------------------------------------------
def test_a_cell_named_twice_is_scanned_once_with_its_first_base_and_minus_one_is_skipped(cells):
    errors()
    probes = np.array([[5, 5, 5], [4, 0, 4], [-1, 1, -1], [-1, -1, -1], [6, -1, 6], [1, 5, 1]])
    base = quarters(cells.rng, probes.shape)
    for i in range(6):
        for j in range(3):
            if probes[i, j] >= 0 and probes[i, j] in probes[i, :j]:
                base[i, j] = 1e30                                            # the repeat's base: used, it would lift every score of the cell
    got, _ = cells.all(probes, 12, base=base)
    ids, sc = got[1].cpu().numpy(), got[0].cpu().numpy()
    for i in range(6):
        valid = ids[i][ids[i] >= 0]
        assert len(set(valid.tolist())) == valid.size                        # no row twice
        assert (sc[i][ids[i] >= 0] < 1e20).all()
    assert (ids[0] >= 0).sum() == min(12, cells.sizes[5]) and (ids[2] >= 0).sum() == 1 and (ids[3] >= 0).sum() == 0 and (ids[4] >= 0).sum() == 12
    cells.all(probes, 12, by_residual=False)
    assert errors() == 0


def test_probe_entries_past_nlist_are_skipped_and_counted(cells):
    errors()
    probes = [[NLIST, 5, 1], [2 ** 40, 2 ** 40, 4], [0, 1, 2], [NLIST, NLIST, NLIST], [6, -1, 2 ** 40], [2 ** 62, 0, NLIST + 1]]
    cells.all(probes, 10)                                                    # (three calls: the C entry point, the op, ops)
    assert errors() == 3 * 9
    assert errors() == 0                                                     # the read above reset the count


def test_a_query_over_max_scan_rows_is_padding_and_its_neighbours_are_unchanged(cells):
    probes = [[1, 5], [6, 4], [2, 3], [3, 5], [6, 5], [0, 2]]
    totals = [cells.sizes[a] + cells.sizes[b] for a, b in probes]
    base = quarters(cells.rng, (6, 2))
    errors()
    full, _ = cells.all(probes, 10, base=base)
    assert errors() == 0
    scan = totals[1] - 1                                                     # query 1 holds one row too many; so does query 4 (the two largest cells)
    got, _ = cells.all(probes, 10, base=base, max_scan=scan)
    assert errors() == 3 * 2
    for i in range(6):
        if totals[i] > scan:
            assert (got[1][i] == -1).all() and (got[0][i] == -FLT_MAX).all()
        else:
            assert torch.equal(got[1][i], full[1][i]) and torch.equal(bits(got[0][i]), bits(full[0][i]))
    assert [t > scan for t in totals] == [False, True, False, False, True, False]


def test_positions_are_rows_without_row_ids_and_k_beyond_the_scanned_rows_pads_the_tail(cells):
    got, _ = cells.all([[6, 2], [0, 5], [3, 4], [1, 6], [1, 1], [2, 0]], 10, row_ids=False)
    assert int(got[1].max()) < cells.n
    G = group_rows(cells.d)
    got, _ = cells.all([[1, 0], [2, 1], [0, 0], [1, 2], [3, 1], [1, 1]], 2 * G + 5)
    assert (got[1][0, :1] >= 0).all() and (got[1][0, 1:] == -1).all() and (got[0][0, 1:] == -FLT_MAX).all()
    assert (got[1][1, :G] >= 0).all() and (got[1][1, G:] == -1).all() and (got[1][2] == -1).all()
    every = [list(range(NLIST))] * 6
    got, _ = cells.all(every, min(2048, cells.n), by_residual=False)         # every row of every cell
    assert (got[1] >= 0).all()


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, nlist, k", [(600, 8, 50), (6000, 4, 100), (6000, 4, 2048)])      # a segment under 2048 words (sorted whole); above (radix select)
@pytest.mark.parametrize("by_residual", [True, False])
def test_ties_go_to_the_lower_original_row(n, nlist, k, by_residual):
    rng = np.random.default_rng(n + k)
    d = 32
    proto = rng.integers(0, 2, (12, d)).astype(np.float32)                   # 12 distinct 0/1 rows: identical rows inside and across the cells
    x = proto[rng.integers(0, 12, n)]
    q = rng.integers(0, 2, (5, d)).astype(np.float32)
    q[3] = 0
    cent = rng.integers(0, 2, (nlist, d)).astype(np.float32)
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    stored = Y.encode(x[row_ids], cent, cells[row_ids]) if by_residual else Y.encode(x[row_ids])
    probes = np.stack([rng.permutation(nlist)[:nlist - 1] for _ in range(5)])
    base = quarters(rng, probes.shape) if by_residual else None
    if by_residual:
        base[3] = 0.25                                                       # one base for all cells of the zero query: every score equal
    want = Y.search(q, stored, list_off, row_ids, probes, base, by_residual, k)
    assert np.mean(want[0][:, 1:] == want[0][:, :-1]) > 0.5                  # ties everywhere in the result
    got = ivfsq_c(q, stored, list_off, row_ids, probes, base, by_residual, k, n)
    assert_yardstick(got, want)
    assert_yardstick(ivfsq_op(q, stored, list_off, row_ids, probes, base, by_residual, k, n), want)
    scanned = np.sort(np.flatnonzero(np.isin(cells, probes[3])))
    assert scanned.size > 2048 or n == 600
    kk = min(k, scanned.size)
    assert np.array_equal(got[1][3].cpu().numpy()[:kk], scanned[:kk])        # the all-zero query: the lowest original rows of its cells
    assert (got[0][3][:kk] == (0.25 if by_residual else 0.0)).all()


# ---- 5. batch independence ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    """5000 Gaussian rows of d = 256 dealt to 64 cells at random, coded by residual to Gaussian centroids, nprobe 8; 130 queries."""
    from lightretriever_amd import IVFSQIndex
    rng = np.random.default_rng(11)
    n, d, nlist = 5000, 256, 64
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    x = rng.standard_normal((n, d)).astype(np.float32)
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    codes = Y.encode(x, cent, cells)
    idx = IVFSQIndex(d, nlist, nprobe=8)
    idx.set_contents(cent, codes[row_ids], list_off, row_ids)
    q = torch.randn(130, d, generator=torch.Generator(device="cuda").manual_seed(11), device="cuda")
    idx.search(q[:1], 1)
    return idx, codes, cells, q


def test_a_query_does_not_depend_on_its_batch(mid):
    idx, _, _, q = mid
    K = 100
    whole = idx.search(q, K)                                                 # distinct probe lists: the quantiser's
    for i in range(130):
        alone = idx.search(q[i:i + 1], K)
        assert torch.equal(alone[1][0], whole[1][i]) and torch.equal(bits(alone[0][0]), bits(whole[0][i])), i
    first = idx.search(q[77:79], K)
    assert torch.equal(first[1][0], whole[1][77]) and torch.equal(bits(first[0][0]), bits(whole[0][77]))
    # a different scan bound (another layout of the workspace) changes nothing either
    ps, pr = idx.quantizer.search(q, 8)
    args = (idx.stored_codes(), idx.list_off, idx.row_ids)
    assert_same(ivfsq_op(q, *args, pr, ps, True, K, idx.ntotal), whole)
    held = idx.list_sizes[pr.cpu().numpy()].sum(axis=1)                      # every query reports min(K, the rows of its cells) rows
    assert np.array_equal((whole[1] >= 0).sum(dim=1).cpu().numpy(), np.minimum(held, K))
    # equal probe lists: every query probes the cells of query 0 -- each cell's group is scored against all 130 at once
    pe, se = pr[:1].expand(130, 8).contiguous(), ps[:1].expand(130, 8).contiguous()
    whole = ivfsq_op(q, *args, pe, se, True, K, idx.ntotal)
    for i in (0, 1, 63, 64, 77, 129):
        alone = ivfsq_op(q[i:i + 1], *args, pe[:1], se[:1], True, K, idx.ntotal)
        assert torch.equal(alone[1][0], whole[1][i]) and torch.equal(bits(alone[0][0]), bits(whole[0][i])), i
    first = ivfsq_op(q[77:79], *args, pe[:2], se[:2], True, K, idx.ntotal)
    assert torch.equal(first[1][0], whole[1][77]) and torch.equal(bits(first[0][0]), bits(whole[0][77]))


# ---- 6. the codes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_residual", [True, False])
def test_added_rows_are_coded_as_the_yardstick_codes_them(by_residual):
    from lightretriever_amd import IVFSQIndex
    rng = np.random.default_rng(3)
    n, d, nlist = 700, 64, 6
    scale = (10.0 ** rng.uniform(-7, 5.5, d)).astype(np.float32)             # per column: from far under fp16's subnormals to far over its range
    scale[:4] = [1e5, 3e5, 1e-6, 3e-7]
    x = (rng.standard_normal((n, d)) * scale).astype(np.float32)
    cent = (rng.standard_normal((nlist, d)) * scale).astype(np.float32)
    idx = IVFSQIndex(d, nlist, by_residual=by_residual)
    idx.set_contents(cent, torch.zeros(0, d, dtype=torch.float16), np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64))
    for piece in (x[:1], x[1:300], x[300:]):
        idx.add(dev(piece))
    cells = IV.assign_cells(x, cent)
    assert np.array_equal(idx._assign[:n].cpu().numpy(), cells)
    want = Y.encode(x, cent, cells) if by_residual else Y.encode(x)
    got = idx.stored_codes().cpu().numpy()                                   # (cell order: position p holds original row row_ids[p])
    row_ids = idx.row_ids.cpu().numpy()
    assert np.array_equal(row_ids, IV.cell_order(cells, nlist)[0])
    assert got.dtype == np.float16 and np.array_equal(got.view(np.int16), want[row_ids].view(np.int16))
    v = want.astype(np.float32)
    assert (v == 65504).any() and (v == -65504).any() and not np.isinf(v).any()            # both signs saturate
    assert ((np.abs(v) < 2.0 ** -14) & (v != 0)).any()                                       # fp16 subnormals
    # rows reconstruct as the yardstick decodes them
    recon = Y.decode(want, cent, cells) if by_residual else Y.decode(want)
    assert np.array_equal(idx.reconstruct_n(0, n).cpu().numpy().view(np.int32), recon.view(np.int32))
    assert np.array_equal(idx.reconstruct_n(690, 7).cpu().numpy().view(np.int32), recon[690:697].view(np.int32))
    assert np.array_equal(idx.vectors.cpu().numpy().view(np.int32), recon.view(np.int32))


def test_the_encode_call_writes_zeros_for_a_cell_outside_the_lists_and_counts_it():
    from lightretriever_amd import _lib
    l = _lib.lib()
    rng = np.random.default_rng(4)
    d, nlist = 96, 5
    x = rng.standard_normal((9, d)).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    cells = np.array([0, -1, nlist, 2 ** 40, 4, -2 ** 62, 2, 2, 1], np.int64)
    ok = (cells >= 0) & (cells < nlist)
    dx = torch.full((9, d + 8), 1e30, dtype=torch.float32, device="cuda")    # ldx = d + 8: the padding columns are never read
    dx[:, :d] = dev(x)
    for with_cent in (True, False):
        codes = torch.full((12, d), 7.0, dtype=torch.float16, device="cuda")
        errors()
        _lib.check(l.lrx_ivf_sq_fp16_encode_rows(_lib.ptr(dx), d + 8, 9, d, _lib.ptr(dev(cent)) if with_cent else None, _lib.ptr(dev(cells)), nlist,
                                                 _lib.ptr(codes), 2, _lib.current_stream()))
        assert errors() == int((~ok).sum()) == 4
        want = Y.encode(x, cent, np.where(ok, cells, 0)) if with_cent else Y.encode(x)
        want[~ok] = 0
        got = codes.cpu().numpy()
        assert np.array_equal(got[2:11].view(np.int16), want.view(np.int16)) and (got[:2] == 7).all() and (got[11:] == 7).all()
    codes = torch.zeros(9, d, dtype=torch.float16, device="cuda")             # no residual: the cells may be left out
    _lib.check(l.lrx_ivf_sq_fp16_encode_rows(_lib.ptr(dx), d + 8, 9, d, None, None, nlist, _lib.ptr(codes), 0, _lib.current_stream()))
    assert errors() == 0 and np.array_equal(codes.cpu().numpy().view(np.int16), Y.encode(x).view(np.int16))


# ---- 7. the life cycle ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """4000 x 64 clustered rows, nlist 16, trained with 2 iterations, all rows added."""
    from lightretriever_amd import IVFSQIndex
    x, q = IV.clustered_corpus(n=4000, d=64, n_clusters=40)
    x, q = dev(x), dev(q)
    idx = IVFSQIndex(64, 16, nprobe=4)
    idx.train(x, niter=2)
    idx.add(x)
    return x, q, idx


def empty_like(idx, **kw):
    from lightretriever_amd import IVFSQIndex
    b = IVFSQIndex(idx.d, idx.nlist, nprobe=idx.nprobe, by_residual=idx.by_residual, **kw)
    b.set_contents(idx.centroids, torch.zeros(0, idx.d, dtype=torch.float16), np.zeros(idx.nlist + 1, np.int64), np.zeros(0, np.int64))
    return b


def test_training_is_deterministic_and_is_the_flat_inverted_files(trained):
    from lightretriever_amd import IVFFlatIndex, IVFSQIndex
    x, q, idx = trained
    again = IVFSQIndex(64, 16, by_residual=False)
    again.train(x, niter=2)
    assert torch.equal(bits(again.centroids), bits(idx.centroids))
    flat = IVFFlatIndex(64, 16)
    flat.train(x, niter=2)
    assert torch.equal(bits(idx.centroids), bits(flat.centroids))            # the coarse quantiser is IVFFlatIndex's
    with pytest.raises(ValueError, match="15 training rows"):
        IVFSQIndex(64, 16).train(x[:15])


def test_adds_in_pieces_equal_one_add(trained):
    x, q, idx = trained
    want = idx.search(q, 20)
    b = empty_like(idx)
    for piece in (x[:1], x[1:128], x[128:]):
        b.add(piece)
    assert b.ntotal == 4000
    assert_same(b.search(q, 20), want)
    assert torch.equal(b.list_off, idx.list_off) and torch.equal(b.row_ids, idx.row_ids) and torch.equal(bits16(b.stored_codes()), bits16(idx.stored_codes()))
    assert np.array_equal(b.list_sizes, idx.list_sizes)
    off, ids = b.list_off.cpu().numpy(), b.row_ids.cpu().numpy()
    assert all((np.diff(ids[off[c]:off[c + 1]]) > 0).all() for c in range(16))       # ascending original row inside every cell
    # add -> search -> add -> search equals a fresh index with all rows; a small rebuild chunk changes nothing
    c = empty_like(idx)
    c.rebuild_chunk_rows = 700
    c.add(x[:3000])
    part = c.search(q, 20)
    assert int((part[1] >= 3000).sum()) == 0
    c.add(x[3000:])
    assert_same(c.search(q, 20), want)
    assert torch.equal(c.row_ids, idx.row_ids) and torch.equal(bits16(c.stored_codes()), bits16(idx.stored_codes()))
    # reset() keeps the training
    c.reset()
    assert c.ntotal == 0 and c.is_trained and (c.search(q[:2], 5)[1] == -1).all()
    c.add(x)
    assert_same(c.search(q, 20), want)


def test_append_slot_and_commit_train_an_untrained_index(trained):
    from lightretriever_amd import IVFSQIndex
    x, q, _ = trained
    a = IVFSQIndex(64, 16, nprobe=4)
    a.NITER = 2                                                              # commit() trains with the defaults: two iterations here
    slot = a.append_slot(2000)
    slot.copy_(x[:2000])
    a.commit(2000)
    assert a.is_trained and a.ntotal == 2000
    b = IVFSQIndex(64, 16, nprobe=4)
    b.train(x[:2000], niter=2)
    b.add(x[:2000])
    assert torch.equal(bits(a.centroids), bits(b.centroids))
    assert_same(a.search(q, 10), b.search(q, 10))
    with pytest.raises(ValueError, match="staged"):
        a.commit(5)


def test_refusals(trained):
    from lightretriever_amd import IVFSQIndex
    x, q, idx = trained
    with pytest.raises(RuntimeError, match="not trained"):
        IVFSQIndex(64, 16).add(x[:1])
    with pytest.raises(RuntimeError, match="not trained"):
        IVFSQIndex(64, 16).search(q, 1)
    with pytest.raises(ValueError, match="k=2049"):
        idx.search(q, 2049)
    with pytest.raises(ValueError, match="nprobe=17"):
        idx.search(q, 10, nprobe=17)
    with pytest.raises(ValueError, match="row_map"):
        idx.search(q, 10, row_map=torch.arange(10, device="cuda"))
    with pytest.raises(NotImplementedError, match="range_search"):
        idx.range_search(q, 0.0)
    with pytest.raises(ValueError, match="codes must be fp16"):
        idx.set_contents(idx.centroids, torch.zeros(3, 64), np.zeros(17, np.int64), np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="list_off"):
        idx.set_contents(idx.centroids, torch.zeros(3, 64, dtype=torch.float16), np.zeros(17, np.int64), np.arange(3))
    assert idx.search(q[:0], 10)[0].shape == (0, 10) and idx.ntotal == 4000


# ---- 8. nesting of the probe sets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_residual", [True, False])
def test_overlap_with_the_full_probe_never_falls_with_nprobe(by_residual):
    from lightretriever_amd import IVFSQIndex
    x, q = IV.clustered_corpus(n=20000, d=128)
    idx = IVFSQIndex(128, 32, by_residual=by_residual)
    idx.train(dev(x), niter=2)
    idx.add(dev(x))
    dq = dev(q)
    full = idx.search(dq, 10, nprobe=32)
    last = np.zeros(len(q), np.int64)
    for nprobe in (1, 2, 4, 8, 16, 32):
        D, I = idx.search(dq, 10, nprobe=nprobe)
        ov = IV.overlap(I.cpu().numpy(), full[1].cpu().numpy())
        assert (ov >= last).all(), (nprobe, ov, last)
        last = ov
    assert (last == 10).all()
    assert_same((D, I), full)


# ---- 9. ids and files ---------------------------------------------------------------------------------------------------------------------------
def test_ids_follow_id_base_and_row_map(mid):
    idx, codes, cells, q = mid
    qs = q[:7]
    D, I = idx.search(qs, 20)
    idx.id_base = 5
    assert_same(idx.search(qs, 20), (D, torch.where(I >= 0, I + 5, I)))
    idx.id_base = 0
    rm = torch.arange(5000, device="cuda") * 3 + 7
    assert_same(idx.search(qs, 20, row_map=rm), (D, I * 3 + 7))
    assert torch.equal(bits16(idx.stored_codes().cpu()), bits16(torch.from_numpy(codes)[idx.row_ids.cpu()]))
    assert torch.equal(idx._assign[:5000].cpu(), torch.from_numpy(cells))


def test_save_and_load_round_trip(mid, tmp_path):
    from lightretriever_amd import FlatIPIndex, IVFSQIndex, RefineFlatIndex, index_io
    idx, _, _, q = mid
    D, I = idx.search(q, 10)
    path = str(tmp_path / "i.ivfsq.faiss")
    idx.save(path)
    assert open(path, "rb").read() == Y.file_bytes(idx.centroids.cpu().numpy(), idx.list_sizes, idx.stored_codes().cpu().numpy(), idx.row_ids.cpu().numpy(), 8, True)
    st = index_io.read_ivf_sq(path)
    assert (st["d"], st["nlist"], st["nprobe"], st["ntotal"], st["is_trained"], st["by_residual"]) == (256, 64, 8, 5000, True, True)
    back = IVFSQIndex.load(path, id_base=7)
    assert (back.d, back.nlist, back.nprobe, back.by_residual, back.ntotal, back.id_base, back.is_trained) == (256, 64, 8, True, 5000, 7, True)
    assert_same(back.search(q, 10), (D, I + 7))
    back.add(q[:10])                                                         # a loaded index takes further rows
    assert back.ntotal == 5010 and bool((back.search(q[:1], 3)[1] >= 0).all())
    with pytest.raises(NotImplementedError, match="range_search"):
        back.range_search(q, 0.0)
    # a refine index over it
    x = torch.randn(5000, 256, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    base = IVFSQIndex.load(path)
    store = FlatIPIndex(256)
    store.shadow_f16 = False
    store.add(x)
    ref = RefineFlatIndex(base, store, k_factor=3)
    want = ref.search(q, 10)
    rpath = str(tmp_path / "r.refine.faiss")
    ref.save(rpath)
    st = index_io.read_refine(rpath)
    assert st["base"]["fourcc"] == b"IwSq" and st["k_factor"] == 3.0
    again = RefineFlatIndex.load(rpath)
    assert type(again.base_index) is IVFSQIndex and (again.base_index.nprobe, again.base_index.by_residual, again.k_factor) == (8, True, 3.0)
    assert_same(again.search(q, 10), want)
    plain = IVFSQIndex(256, 64, by_residual=False)
    plain.save(path)                                                         # untrained, no residuals
    back = IVFSQIndex.load(path)
    assert not back.is_trained and not back.by_residual and back.ntotal == 0


# ---- 10. HIP graph -----------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_search_replays_the_eager_bits(mid):
    idx, _, _, q = mid
    qbuf = q[:16].clone()
    eager = tuple(t.clone() for t in idx.search(qbuf, 10))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        idx.search(qbuf, 10)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Dg, Ig = idx.search(qbuf, 10)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert_same((Dg, Ig), eager)
    want = tuple(t.clone() for t in idx.search(q[16:32], 10))
    qbuf.copy_(q[16:32])
    graph.replay()
    torch.cuda.synchronize()
    assert_same((Dg, Ig), want)


# ---- 11. the searcher, the hybrid route, refine ------------------------------------------------------------------------------------------------------
def test_searcher_equals_the_index(trained, tmp_path, monkeypatch):
    from lightretriever_amd import IVFSQIndex
    from lightretriever_amd.retriever import HybridSearch, IVFSQFaissSearch, _to_result_dict
    monkeypatch.setattr(IVFSQIndex, "NITER", 2)                              # the searcher trains with the defaults: two iterations here
    x, q, _ = trained
    x, q = x[:300], q[:9]
    ids = [f"doc{i}" for i in range(300)]
    qids = [f"q{i}" for i in range(9)]
    s = HybridSearch(model=None, batch_size=8, faiss_search_map="ivfsq", nlist=12, nprobe=5, by_residual=False, show_progress_bar=False).dense_search
    assert isinstance(s, IVFSQFaissSearch)
    s.index(x, ids)
    idx = s.faiss_index.index
    assert type(idx) is IVFSQIndex and (idx.nlist, idx.nprobe, idx.by_residual, idx.ntotal, s.dim_size) == (12, 5, False, 300, 64)
    direct = IVFSQIndex(64, 12, nprobe=5, by_residual=False)
    direct.train(x)
    direct.add(x)
    want = _to_result_dict(*direct.search(q, 20), qids, ids)
    got = s.retrieve_with_emb(q, qids, 20)
    assert got == want and all(len(v) == 20 for v in got.values())
    s.save(str(tmp_path), prefix="t")
    assert (tmp_path / "t.ivfsq.faiss").exists() and (tmp_path / "t.ivfsq.tsv").exists()
    c = IVFSQFaissSearch(model=None, batch_size=8, show_progress_bar=False)
    c.load(str(tmp_path), prefix="t")
    assert (c.nlist, c.nprobe, c.by_residual, c.faiss_index.index.ntotal) == (12, 5, False, 300)
    assert c.retrieve_with_emb(q, qids, 20) == want
    # a chunk of fewer rows than nlist: one cell per row at the most
    t = IVFSQFaissSearch(model=None, nlist=1024, nprobe=32, batch_size=8, show_progress_bar=False)
    t.index(x[:280], ids[:280])
    assert (t.faiss_index.index.nlist, t.faiss_index.index.nprobe, t.faiss_index.index.by_residual) == (280, 32, True)
    assert len(t.retrieve_with_emb(q, qids, 5)["q0"]) == 5


@pytest.mark.parametrize("k_factor", [1, 2])
def test_refine_is_the_exact_rerank_of_the_bases_own_candidates(k_factor):
    from lightretriever_amd import FlatIPIndex, IVFSQIndex, RefineFlatIndex
    rng = np.random.default_rng(9)
    n, d, nlist, k = 1500, 64, 8, 10
    x = rng.integers(-3, 4, (n, d)).astype(np.float32) + np.float32(0.25) * rng.integers(-2, 3, (n, d)).astype(np.float32)   # quarters: coded exactly or not,
    q = rng.integers(-3, 4, (5, d)).astype(np.float32)                                                                      # every fp64 sum stays exact
    base = IVFSQIndex(d, nlist, nprobe=3)
    base.train(dev(x), niter=1)
    ref = RefineFlatIndex(base, FlatIPIndex(d), k_factor=k_factor)
    ref.add(dev(x))
    assert base.ntotal == n and ref.ntotal == n
    cand = base.search(dev(q), int(k * k_factor))[1].cpu().numpy()
    assert (cand >= 0).all()
    assert_yardstick(ref.search(dev(q), k), Y.rerank(q, x, cand, k))
    if k_factor == 1:
        assert np.array_equal(np.sort(ref.search(dev(q), k)[1].cpu().numpy(), axis=1), np.sort(cand, axis=1))
