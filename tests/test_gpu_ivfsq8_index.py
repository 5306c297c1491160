"""GPU: the inverted-file 8-bit scalar-quantised index (lrx_ivf_sq8_ip_search, lrx_ivf_sq8_encode_rows, lrx_ivf_sq8_decode_rows,
torch.ops.lrx.ivf_sq8_ip_topk, ops.ivf_sq8_ip_topk, IVFSQ8Index, IVFSQ8FaissSearch) against the numpy yardstick (tests/ivfsq8_yardstick.py),
lrx_ivf_flat_ip_search over the decoded rows, SQ8Index, IVFFlatIndex and RefineFlatIndex, bit for bit, no tolerance anywhere:
  (a) without residuals the result over ANY probe lists is the flat inverted file's over the fp32 rows the decode entry returns (Gaussian data);
  (b) on grid data -- ranges under which every code decodes exactly to a multiple of 1/4 (test_ivfsq8_index_host.py checks them) -- and probing
      every cell it is SQ8Index.search's, whose rescoring adds in another order;
hand-made cells around the row group of the scan with every kind of bad probe entry; ties; batch independence; the codes and their decode; range
training; the life cycle; nesting of the probe sets; persistence, HIP graph, the searcher and the refine route.  Observed figures: DESIGN §5.4.13."""
import numpy as np
import pytest
import torch

import ivf_yardstick as IV
import ivfsq8_yardstick as Y
import sq8_yardstick as S8

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
F32 = np.float32
QT = {"QT_8bit": 0, "QT_8bit_uniform": 2}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.view(torch.int32)


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


@pytest.fixture(autouse=True)
def no_device_error_is_left_behind():
    """Every test ends with the device error count at 0: the tests that provoke a count on purpose read (and so reset) it themselves."""
    errors()                                                                  # (whatever an earlier module left)
    yield
    assert errors() == 0


def group_rows(d):
    from lightretriever_amd import _lib
    return int(_lib.lib().lrx_ivf_sq8_group_rows(d))


def grid_trained(d, qtype, rng):
    """`trained` under which every code decodes to a grid value (Y.GRID_RANGES): the three ranges mixed across the dimensions for QT_8bit, the
    middle one for QT_8bit_uniform; and the grid's step per dimension."""
    if qtype == "QT_8bit_uniform":
        return np.array(Y.GRID_RANGES[1][:2], F32), np.full(d, Y.GRID_RANGES[1][2], F32)
    r = np.array(Y.GRID_RANGES, np.float64)[rng.integers(0, 3, d)]
    return np.concatenate([r[:, 0], r[:, 1]]).astype(F32), r[:, 2].astype(F32)


def _args(q, codes, trained, list_off, row_ids, probes, base):
    q, codes, trained, list_off, probes = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, codes, trained, list_off, probes))
    row_ids = row_ids if row_ids is None or isinstance(row_ids, torch.Tensor) else dev(row_ids)
    base = base if base is None or isinstance(base, torch.Tensor) else dev(np.asarray(base, F32))
    return q.contiguous(), codes, trained, list_off, row_ids, probes, base


def sq8_c(q, codes, trained, qt, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    """lrx_ivf_sq8_ip_search through ctypes with ld_probe = nprobe + 3: the padding entries name cell 0 and carry a score of 1e30 (read, they
    would add that cell's rows or lift a score)."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    q, codes, trained, list_off, row_ids, probes, base = _args(q, codes, trained, list_off, row_ids, probes, base)
    (Q, D), n, npb, nlist = q.shape, codes.shape[0], probes.shape[1], list_off.numel() - 1
    pb = torch.zeros(Q, npb + 3, dtype=torch.int64, device="cuda")
    pb[:, :npb] = probes
    ps = None
    if base is not None:
        ps = torch.full((Q, npb + 3), 1e30, dtype=torch.float32, device="cuda")
        ps[:, :npb] = base
    Do = torch.full((Q, k), 7.5, dtype=torch.float32, device="cuda")
    Io = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(l.lrx_ivf_sq8_ip_workspace_bytes(n, nlist, D, Q, npb, k, max_scan), dtype=torch.uint8, device="cuda")
    _lib.check(l.lrx_ivf_sq8_ip_search(_lib.ptr(codes), n, D, _lib.ptr(trained), qt, _lib.ptr(list_off), _lib.ptr(row_ids), nlist, _lib.ptr(q), Q, _lib.ptr(pb),
                                       _lib.ptr(ps), npb, npb + 3, int(by_residual), max_scan, k, id_base, _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(row_map), _lib.ptr(ws),
                                       ws.numel(), _lib.current_stream()))
    torch.cuda.synchronize()
    return Do, Io


def sq8_op(q, codes, trained, qt, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    from lightretriever_amd import torch_ops
    torch_ops.load()
    q, codes, trained, list_off, row_ids, probes, base = _args(q, codes, trained, list_off, row_ids, probes, base)
    return torch.ops.lrx.ivf_sq8_ip_topk(q, codes, trained, qt, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base, row_map)


def sq8_ops(q, codes, trained, qt, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    from lightretriever_amd import ops
    q, codes, trained, list_off, row_ids, probes, base = _args(q, codes, trained, list_off, row_ids, probes, base)
    return ops.ivf_sq8_ip_topk(q, codes, trained, qt, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base, row_map)


def decode_c(codes, trained, qt, cent=None, cells=None, nlist=1, row0=0, n=None):
    """lrx_ivf_sq8_decode_rows through ctypes -> fp32 [n, d] (ldo = d + 4: the padding columns keep their fill)."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    n = codes.shape[0] - row0 if n is None else n
    d = codes.shape[1]
    out = torch.full((n, d + 4), 9.5, dtype=torch.float32, device="cuda")
    _lib.check(l.lrx_ivf_sq8_decode_rows(_lib.ptr(codes), row0, n, d, _lib.ptr(trained), qt, _lib.ptr(cent), _lib.ptr(cells), nlist, _lib.ptr(out), d + 4,
                                         _lib.current_stream()))
    torch.cuda.synchronize()
    assert (out[:, d:] == 9.5).all()
    return out[:, :d].contiguous()


def quarters(rng, shape):
    return (rng.integers(-12, 13, shape) / 4.0).astype(F32)


# ---- 1. consequence (a): without residuals, the flat inverted file over the decoded rows --------------------------------------------------
@pytest.mark.parametrize("qtype", ["QT_8bit", "QT_8bit_uniform"])
@pytest.mark.parametrize("Q, n, d, nlist, k", [(1, 500, 64, 4, 10), (5, 3000, 128, 16, 100), (130, 4000, 64, 8, 2048), (3, 600, 2112, 5, 50), (2, 40, 8192, 3, 7)])
def test_without_residuals_it_is_the_flat_inverted_file_over_the_decoded_rows(Q, n, d, nlist, k, qtype):
    from lightretriever_amd import IVFSQ8Index, ops
    g = torch.Generator(device="cuda").manual_seed(n + d)
    x = torch.randn(n, d, generator=g, device="cuda")
    q = torch.randn(Q, d, generator=g, device="cuda")
    idx = IVFSQ8Index(d, nlist, qtype, nprobe=nlist, by_residual=False)
    idx.train(x, niter=2)
    idx.add(x)
    assert idx.ntotal == n and int(idx.list_sizes.sum()) == n and idx.max_scan_rows() == n
    codes = idx.stored_codes()
    rows = decode_c(codes, idx.trained, QT[qtype])                            # the fp32 rows the codes stand for, by stored position
    assert rows.abs().max() > 1 and len(torch.unique(codes)) > 200            # a trained range, codes all over it
    errors()
    for nprobe in (1, nlist):
        pr = idx.quantizer.search(q, nprobe)[1]
        scan = idx.max_scan_rows(nprobe)
        got = sq8_c(q, codes, idx.trained, QT[qtype], idx.list_off, idx.row_ids, pr, None, False, k, scan)
        assert_same(got, ops.ivf_flat_ip_topk(q, rows, idx.list_off, idx.row_ids, pr, k, scan))
        assert_same(idx.search(q, k, nprobe=nprobe), got)
        if Q * n <= 20000:   # the yardstick's ordered sum gives these bits on any data
            assert_yardstick(got, Y.search(q.cpu().numpy(), codes.cpu().numpy(), idx.trained.cpu().numpy(), idx.list_off.cpu().numpy(), idx.row_ids.cpu().numpy(),
                                           pr.cpu().numpy(), None, False, k))
    assert errors() == 0


# ---- 2. consequence (b): on grid data, probing every cell, SQ8Index.search ----------------------------------------------------------------
@pytest.mark.parametrize("qtype", ["QT_8bit", "QT_8bit_uniform"])
@pytest.mark.parametrize("Q, n, d, nlist, k", [(5, 700, 64, 6, 50), (3, 300, 2112, 4, 20)])
def test_on_grid_data_probing_every_cell_it_is_the_flat_8_bit_index(Q, n, d, nlist, k, qtype):
    from lightretriever_amd import IVFSQ8Index, SQ8Index
    rng = np.random.default_rng(n + d)
    trained, step = grid_trained(d, qtype, rng)
    codes = rng.integers(0, 256, (n, d)).astype(np.uint8)
    codes[0], codes[1] = 0, 255                                               # the first two rows carry every column's minimum and maximum
    q = quarters(rng, (Q, d))
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    sq = SQ8Index(d, qtype)
    sq.set_contents(trained, torch.from_numpy(codes))
    y = sq.reconstruct_n(0, n).cpu().numpy()
    assert np.array_equal(y / step, np.round(y / step)) and np.abs(y).max() <= 128            # the precondition: the decoded rows are on the grid
    idx = IVFSQ8Index(d, nlist, qtype, nprobe=nlist, by_residual=False)
    idx.set_contents(rng.integers(-3, 4, (nlist, d)).astype(F32), trained, torch.from_numpy(codes[row_ids]), list_off, row_ids)
    assert np.array_equal(idx.reconstruct_n(0, n).cpu().numpy(), y)
    errors()
    got = idx.search(dev(q), k)
    assert_same(got, sq.search(dev(q), k))
    assert_yardstick(got, S8.search(q, codes, trained, k))
    assert errors() == 0


# ---- 3. hand-made cells -------------------------------------------------------------------------------------------------------------------
NLIST = 7


def cell_sizes(d):
    G = group_rows(d)
    s = [0, 1, G - 1, G, G + 1, 2 * G + 3]
    return s + [sum(s) + 50]                                                  # ... and one cell with more than half of the rows


class Cells:
    """Random codes under a grid range, integer centroids, queries and hand-given probe scores in quarters: every fp64 sum is exact."""

    def __init__(self, d, qtype):
        rng = np.random.default_rng(d + QT[qtype])
        self.sizes = cell_sizes(d)
        n = sum(self.sizes)
        cells = rng.permutation(np.repeat(np.arange(NLIST), self.sizes))
        self.d, self.n, self.rng, self.cells, self.qtype, self.qt = d, n, rng, cells, qtype, QT[qtype]
        self.trained, _ = grid_trained(d, qtype, rng)
        self.cent = rng.integers(-3, 4, (NLIST, d)).astype(F32)
        self.q = quarters(rng, (6, d))
        self.row_ids, self.list_off = IV.cell_order(cells, NLIST)
        self.stored = rng.integers(0, 256, (n, d)).astype(np.uint8)           # by stored position
        self.dcodes, self.dtrained = dev(self.stored), dev(self.trained)
        self.dq, self.doff, self.dids = dev(self.q), dev(self.list_off), dev(self.row_ids)

    def all(self, probes, k, by_residual=True, base=None, max_scan=None, row_ids=True):
        """The C call, the torch op and ops over `probes`, each against the yardstick; returns the C call's result."""
        probes = np.asarray(probes, np.int64)
        if by_residual and base is None:
            base = quarters(self.rng, probes.shape)
        base = base if by_residual else None
        scan = self.n if max_scan is None else max_scan
        want = Y.search(self.q, self.stored, self.trained, self.list_off, self.row_ids if row_ids else None, probes, base, by_residual, k, max_scan_rows=max_scan)
        ids = self.dids if row_ids else None
        a = (self.dq, self.dcodes, self.dtrained, self.qt, self.doff, ids, probes, base, by_residual, k, scan)
        got = sq8_c(*a)
        assert_yardstick(got, want)
        assert_yardstick(sq8_op(*a), want)
        assert_yardstick(sq8_ops(*a), want)
        return got, want

    def index(self, nprobe, by_residual, **kw):
        from lightretriever_amd import IVFSQ8Index
        idx = IVFSQ8Index(self.d, NLIST, self.qtype, nprobe=nprobe, by_residual=by_residual, **kw)
        idx.set_contents(self.cent, self.trained, torch.from_numpy(self.stored), self.list_off, self.row_ids)
        return idx


@pytest.fixture(scope="module", params=[(32, "QT_8bit"), (64, "QT_8bit_uniform"), (64, "QT_8bit"), (2048, "QT_8bit"), (2048, "QT_8bit_uniform"), (32, "QT_8bit_uniform")],
                ids=lambda p: f"{p[0]}-{p[1]}")
def cells(request):
    return Cells(*request.param)


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
    # the index: the quantiser's own probe lists and scores (integer centroids, queries in quarters: exact)
    idx = cells.index(nprobe, by_residual)
    ps, pr = idx.quantizer.search(cells.dq, nprobe)
    want = Y.search(cells.q, cells.stored, cells.trained, cells.list_off, cells.row_ids, pr.cpu().numpy(), ps.cpu().numpy(), by_residual, 10)
    assert_yardstick(idx.search(cells.dq, 10), want)
    assert errors() == 0


def test_the_last_partial_group_of_every_cell_is_scored(cells):
    """Every row of every cell comes back once (cells of G - 1, G + 1 and 2 G + 3 rows end in a partial group), with the yardstick's score."""
    every = [list(range(NLIST))] * 6
    k = min(2048, cells.n)
    got, want = cells.all(every, k)
    assert (got[1] >= 0).all() and (want[1] >= 0).all()
    if cells.n <= 2048:
        assert (np.sort(got[1].cpu().numpy(), axis=1) == np.arange(cells.n)[None, :]).all()


# ---- 4. probe-list edges ------------------------------------------------------------------------------------------------------------------
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
    errors()
    got, _ = cells.all([[6, 2], [0, 5], [3, 4], [1, 6], [1, 1], [2, 0]], 10, row_ids=False)
    assert int(got[1].max()) < cells.n
    G = group_rows(cells.d)
    got, _ = cells.all([[1, 0], [2, 1], [0, 0], [1, 2], [3, 1], [1, 1]], 2 * G + 5)
    assert (got[1][0, :1] >= 0).all() and (got[1][0, 1:] == -1).all() and (got[0][0, 1:] == -FLT_MAX).all()
    assert (got[1][1, :G] >= 0).all() and (got[1][1, G:] == -1).all() and (got[1][2] == -1).all()
    assert errors() == 0


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, nlist, k", [(600, 8, 50), (6000, 4, 100), (6000, 4, 2048)])      # a segment under 2048 words (sorted whole); above (radix select)
@pytest.mark.parametrize("by_residual, qtype", [(True, "QT_8bit"), (False, "QT_8bit_uniform")])
def test_ties_go_to_the_lower_original_row(n, nlist, k, by_residual, qtype):
    rng = np.random.default_rng(n + k)
    d = 32
    trained = np.array([-128.5, 255.0], F32) if qtype == "QT_8bit_uniform" else np.concatenate([np.full(d, -128.5), np.full(d, 255.0)]).astype(F32)
    proto = rng.integers(0, 2, (12, d)).astype(np.uint8) + 128               # 12 distinct rows that decode to 0 / 1: identical rows inside and across the cells
    assert set(np.unique(S8.decode(proto, trained)).tolist()) == {0.0, 1.0}
    x = proto[rng.integers(0, 12, n)]
    q = rng.integers(0, 2, (5, d)).astype(F32)
    q[3] = 0
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    stored = x[row_ids]
    probes = np.stack([rng.permutation(nlist)[:nlist - 1] for _ in range(5)])
    base = quarters(rng, probes.shape) if by_residual else None
    if by_residual:
        base[3] = 0.25                                                       # one base for all cells of the zero query: every score equal
    want = Y.search(q, stored, trained, list_off, row_ids, probes, base, by_residual, k)
    assert np.mean(want[0][:, 1:] == want[0][:, :-1]) > 0.5                  # ties everywhere in the result
    got = sq8_c(q, stored, trained, QT[qtype], list_off, row_ids, probes, base, by_residual, k, n)
    assert_yardstick(got, want)
    assert_yardstick(sq8_op(q, stored, trained, QT[qtype], list_off, row_ids, probes, base, by_residual, k, n), want)
    scanned = np.sort(np.flatnonzero(np.isin(cells, probes[3])))
    assert scanned.size > 2048 or n == 600
    kk = min(k, scanned.size)
    assert np.array_equal(got[1][3].cpu().numpy()[:kk], scanned[:kk])        # the all-zero query: the lowest original rows of its cells
    assert (got[0][3][:kk] == (0.25 if by_residual else 0.0)).all()


# ---- 6. batch independence ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    """5000 Gaussian rows of d = 256 in 64 trained cells, coded by residual under the trained per-dimension range, nprobe 8; 130 queries."""
    from lightretriever_amd import IVFSQ8Index
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(5000, 256, generator=g, device="cuda")
    q = torch.randn(130, 256, generator=g, device="cuda")
    idx = IVFSQ8Index(256, 64, nprobe=8)
    idx.train(x, niter=2)
    idx.add(x)
    idx.search(q[:1], 1)
    return idx, x, q


def test_a_query_does_not_depend_on_its_batch(mid):
    idx, _, q = mid
    K = 100
    errors()
    whole = idx.search(q, K)                                                 # distinct probe lists: the quantiser's
    for i in range(130):
        alone = idx.search(q[i:i + 1], K)
        assert torch.equal(alone[1][0], whole[1][i]) and torch.equal(bits(alone[0][0]), bits(whole[0][i])), i
    first = idx.search(q[77:79], K)
    assert torch.equal(first[1][0], whole[1][77]) and torch.equal(bits(first[0][0]), bits(whole[0][77]))
    # a different scan bound (another layout of the workspace) changes nothing either
    ps, pr = idx.quantizer.search(q, 8)
    args = (idx.stored_codes(), idx.trained, 0, idx.list_off, idx.row_ids)
    assert_same(sq8_op(q, *args, pr, ps, True, K, idx.ntotal), whole)
    held = idx.list_sizes[pr.cpu().numpy()].sum(axis=1)                      # every query reports min(K, the rows of its cells) rows
    assert np.array_equal((whole[1] >= 0).sum(dim=1).cpu().numpy(), np.minimum(held, K))
    # equal probe lists: every query probes the cells of query 0 -- each cell's group is scored against all 130 at once
    pe, se = pr[:1].expand(130, 8).contiguous(), ps[:1].expand(130, 8).contiguous()
    whole = sq8_op(q, *args, pe, se, True, K, idx.ntotal)
    for i in (0, 1, 63, 64, 77, 129):
        alone = sq8_op(q[i:i + 1], *args, pe[:1], se[:1], True, K, idx.ntotal)
        assert torch.equal(alone[1][0], whole[1][i]) and torch.equal(bits(alone[0][0]), bits(whole[0][i])), i
    first = sq8_op(q[77:79], *args, pe[:2], se[:2], True, K, idx.ntotal)
    assert torch.equal(first[1][0], whole[1][77]) and torch.equal(bits(first[0][0]), bits(whole[0][77]))
    # with residuals and the quantiser's scores the yardstick's ordered sum gives these bits too (a few queries: it is slow)
    sub = slice(0, 3)
    assert_yardstick((whole[0][sub], whole[1][sub]), Y.search(q[sub].cpu().numpy(), idx.stored_codes().cpu().numpy(), idx.trained.cpu().numpy(), idx.list_off.cpu().numpy(),
                                                              idx.row_ids.cpu().numpy(), pe[sub].cpu().numpy(), se[sub].cpu().numpy(), True, K))
    assert errors() == 0


# ---- 7. the codes and their decode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qtype", ["QT_8bit", "QT_8bit_uniform"])
@pytest.mark.parametrize("by_residual", [True, False])
def test_added_rows_are_coded_as_the_yardstick_codes_them(by_residual, qtype):
    from lightretriever_amd import IVFSQ8Index
    rng = np.random.default_rng(3)
    n, d, nlist = 700, 64, 6
    x = (rng.standard_normal((n, d)) * 4).astype(F32)                        # four times the spread the range was trained on: rows clamp both ways
    cent = rng.standard_normal((nlist, d)).astype(F32)
    trained = S8.train(rng.standard_normal((50, d)).astype(F32), qtype == "QT_8bit_uniform")
    if qtype == "QT_8bit":
        trained[d + 5] = 0                                                   # a dimension without width: every code 0
    idx = IVFSQ8Index(d, nlist, qtype, by_residual=by_residual)
    idx.set_contents(cent, trained, torch.zeros(0, d, dtype=torch.uint8), np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64))
    errors()
    for piece in (x[:1], x[1:300], x[300:]):
        idx.add(dev(piece))
    cells = IV.assign_cells(x, cent)
    assert np.array_equal(idx._assign[:n].cpu().numpy(), cells)
    want = Y.encode(x, trained, cent, cells) if by_residual else Y.encode(x, trained)
    got = idx.stored_codes().cpu().numpy()                                   # (cell order: position p holds original row row_ids[p])
    row_ids = idx.row_ids.cpu().numpy()
    assert np.array_equal(row_ids, IV.cell_order(cells, nlist)[0])
    assert got.dtype == np.uint8 and np.array_equal(got, want[row_ids])
    assert (want == 0).mean() > 0.1 and (want == 255).mean() > 0.1 and len(np.unique(want)) == 256     # both ends clamp, every code occurs
    assert qtype != "QT_8bit" or not want[:, 5].any()
    # rows reconstruct as the yardstick decodes them, through the decode entry
    recon = Y.decode(want, trained, cent, cells) if by_residual else Y.decode(want, trained)
    assert np.array_equal(idx.reconstruct_n(0, n).cpu().numpy().view(np.int32), recon.view(np.int32))
    assert np.array_equal(idx.reconstruct_n(690, 7).cpu().numpy().view(np.int32), recon[690:697].view(np.int32))
    assert np.array_equal(idx.vectors.cpu().numpy().view(np.int32), recon.view(np.int32))
    assert np.array_equal(idx.decode_stored(3, 40, residual=True).cpu().numpy().view(np.int32), Y.decode(want[row_ids][3:43], trained).view(np.int32))
    assert errors() == 0


@pytest.mark.parametrize("qt", [0, 2])
def test_the_encode_and_decode_calls_zero_a_row_of_a_cell_outside_the_lists_and_count_it(qt):
    from lightretriever_amd import _lib
    l = _lib.lib()
    rng = np.random.default_rng(4)
    d, nlist = 96, 5
    x = (rng.standard_normal((9, d)) * 2).astype(F32)
    x[8, 3], x[0, 17] = np.nan, np.nan                                       # NaN codes as 0, with and without a centroid
    cent = rng.standard_normal((nlist, d)).astype(F32)
    trained = S8.train(rng.standard_normal((30, d)).astype(F32), qt == 2)
    cells = np.array([0, -1, nlist, 2 ** 40, 4, -2 ** 62, 2, 2, 1], np.int64)
    ok = (cells >= 0) & (cells < nlist)
    dx = torch.full((9, d + 8), 1e30, dtype=torch.float32, device="cuda")    # ldx = d + 8: the padding columns are never read
    dx[:, :d] = dev(x)
    dt, dcells, dcent = dev(trained), dev(cells), dev(cent)
    for with_cent in (True, False):
        codes = torch.full((12, d), 7, dtype=torch.uint8, device="cuda")
        errors()
        _lib.check(l.lrx_ivf_sq8_encode_rows(_lib.ptr(dx), d + 8, 9, d, _lib.ptr(dcent) if with_cent else None, _lib.ptr(dcells), nlist, _lib.ptr(dt), qt,
                                             _lib.ptr(codes), 2, _lib.current_stream()))
        assert errors() == int((~ok).sum()) == 4
        want = Y.encode(x, trained, cent if with_cent else None, cells, nlist)
        assert not want[~ok].any() and want[8, 3] == 0 and want[0, 17] == 0
        got = codes.cpu().numpy()
        assert np.array_equal(got[2:11], want) and (got[:2] == 7).all() and (got[11:] == 7).all()
        # ... and back: code rows [2, 11) decoded, the rows of the bad cells zeros and counted
        back = decode_c(codes, dt, qt, dcent if with_cent else None, dcells, nlist, row0=2, n=9)
        assert errors() == 4
        assert np.array_equal(back.cpu().numpy().view(np.int32), Y.decode(want, trained, cent if with_cent else None, cells, nlist).view(np.int32))
    codes = torch.zeros(9, d, dtype=torch.uint8, device="cuda")               # no residual: the cells may be left out
    _lib.check(l.lrx_ivf_sq8_encode_rows(_lib.ptr(dx), d + 8, 9, d, None, None, nlist, _lib.ptr(dt), qt, _lib.ptr(codes), 0, _lib.current_stream()))
    assert errors() == 0 and np.array_equal(codes.cpu().numpy(), Y.encode(x, trained))
    assert np.array_equal(decode_c(codes, dt, qt).cpu().numpy().view(np.int32), Y.decode(Y.encode(x, trained), trained).view(np.int32)) and errors() == 0


# ---- 8. training and the life cycle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """4000 x 64 clustered rows, nlist 16, trained with 2 iterations, all rows added."""
    from lightretriever_amd import IVFSQ8Index
    x, q = IV.clustered_corpus(n=4000, d=64, n_clusters=40)
    x, q = dev(x), dev(q)
    idx = IVFSQ8Index(64, 16, nprobe=4)
    idx.train(x, niter=2)
    idx.add(x)
    return x, q, idx


def empty_like(idx, **kw):
    from lightretriever_amd import IVFSQ8Index
    b = IVFSQ8Index(idx.d, idx.nlist, idx.qtype, nprobe=idx.nprobe, by_residual=idx.by_residual, **kw)
    b.set_contents(idx.centroids, idx.trained, torch.zeros(0, idx.d, dtype=torch.uint8), np.zeros(idx.nlist + 1, np.int64), np.zeros(0, np.int64))
    return b


@pytest.mark.parametrize("qtype", ["QT_8bit", "QT_8bit_uniform"])
@pytest.mark.parametrize("by_residual", [True, False])
def test_the_range_is_trained_on_the_residuals_and_the_cells_are_the_flat_inverted_files(trained, by_residual, qtype):
    from lightretriever_amd import IVFFlatIndex, IVFSQ8Index
    x, q, _ = trained
    idx = IVFSQ8Index(64, 16, qtype, by_residual=by_residual)
    idx.train(x, niter=2)
    flat = IVFFlatIndex(64, 16)
    flat.train(x, niter=2)
    assert torch.equal(bits(idx.centroids), bits(flat.centroids))            # the coarse quantiser is IVFFlatIndex's
    cent = idx.centroids.cpu().numpy()
    want = Y.train_range(x.cpu().numpy(), cent, by_residual, qtype == "QT_8bit_uniform")
    assert idx.trained.shape == want.shape and np.array_equal(idx.trained.cpu().numpy().view(np.int32), want.view(np.int32))
    assert (want[len(want) // 2:] > 0).all()
    again = IVFSQ8Index(64, 16, qtype, by_residual=by_residual)
    again.train(x, niter=2)
    assert torch.equal(bits(again.trained), bits(idx.trained)) and torch.equal(bits(again.centroids), bits(idx.centroids))
    with pytest.raises(ValueError, match="15 training rows"):
        IVFSQ8Index(64, 16).train(x[:15])


def test_adds_in_pieces_equal_one_add(trained):
    x, q, idx = trained
    want = idx.search(q, 20)
    b = empty_like(idx)
    for piece in (x[:1], x[1:128], x[128:]):
        b.add(piece)
    assert b.ntotal == 4000
    assert_same(b.search(q, 20), want)
    assert torch.equal(b.list_off, idx.list_off) and torch.equal(b.row_ids, idx.row_ids) and torch.equal(b.stored_codes(), idx.stored_codes())
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
    assert torch.equal(c.row_ids, idx.row_ids) and torch.equal(c.stored_codes(), idx.stored_codes())
    # reset() keeps the training
    c.reset()
    assert c.ntotal == 0 and c.is_trained and (c.search(q[:2], 5)[1] == -1).all() and torch.equal(bits(c.trained), bits(idx.trained))
    c.add(x)
    assert_same(c.search(q, 20), want)
    assert errors() == 0


def test_append_slot_and_commit_train_an_untrained_index(trained):
    from lightretriever_amd import IVFSQ8Index
    x, q, _ = trained
    a = IVFSQ8Index(64, 16, nprobe=4)
    a.NITER = 2                                                              # commit() trains with the defaults: two iterations here
    slot = a.append_slot(2000)
    slot.copy_(x[:2000])
    a.commit(2000)
    assert a.is_trained and a.ntotal == 2000
    b = IVFSQ8Index(64, 16, nprobe=4)
    b.train(x[:2000], niter=2)
    b.add(x[:2000])
    assert torch.equal(bits(a.centroids), bits(b.centroids)) and torch.equal(bits(a.trained), bits(b.trained))
    assert_same(a.search(q, 10), b.search(q, 10))
    with pytest.raises(ValueError, match="staged"):
        a.commit(5)


def test_refusals(trained):
    from lightretriever_amd import IVFSQ8Index
    x, q, idx = trained
    with pytest.raises(RuntimeError, match="not trained"):
        IVFSQ8Index(64, 16).add(x[:1])
    with pytest.raises(RuntimeError, match="not trained"):
        IVFSQ8Index(64, 16).search(q, 1)
    with pytest.raises(ValueError, match="k=2049"):
        idx.search(q, 2049)
    with pytest.raises(ValueError, match="nprobe=17"):
        idx.search(q, 10, nprobe=17)
    with pytest.raises(ValueError, match="row_map"):
        idx.search(q, 10, row_map=torch.arange(10, device="cuda"))
    with pytest.raises(NotImplementedError, match="range_search"):
        idx.range_search(q, 0.0)
    with pytest.raises(ValueError, match="codes must be uint8"):
        idx.set_contents(idx.centroids, idx.trained, torch.zeros(3, 64), np.zeros(17, np.int64), np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="trained must hold 128"):
        idx.set_contents(idx.centroids, idx.trained[:2], torch.zeros(3, 64, dtype=torch.uint8), np.zeros(17, np.int64), np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="list_off"):
        idx.set_contents(idx.centroids, idx.trained, torch.zeros(3, 64, dtype=torch.uint8), np.zeros(17, np.int64), np.arange(3))
    assert idx.search(q[:0], 10)[0].shape == (0, 10) and idx.ntotal == 4000


# ---- 9. nesting of the probe sets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_residual, qtype", [(True, "QT_8bit"), (False, "QT_8bit"), (True, "QT_8bit_uniform")])
def test_overlap_with_the_full_probe_never_falls_with_nprobe(by_residual, qtype):
    from lightretriever_amd import IVFSQ8Index
    x, q = IV.clustered_corpus(n=20000, d=128)
    idx = IVFSQ8Index(128, 32, qtype, by_residual=by_residual)
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


# ---- 10. ids and files ---------------------------------------------------------------------------------------------------------------------------
def test_ids_follow_id_base_and_row_map(mid):
    idx, _, q = mid
    qs = q[:7]
    D, I = idx.search(qs, 20)
    idx.id_base = 5
    assert_same(idx.search(qs, 20), (D, torch.where(I >= 0, I + 5, I)))
    idx.id_base = 0
    rm = torch.arange(5000, device="cuda") * 3 + 7
    assert_same(idx.search(qs, 20, row_map=rm), (D, I * 3 + 7))


@pytest.mark.parametrize("qtype", ["QT_8bit", "QT_8bit_uniform"])
def test_save_and_load_round_trip(mid, tmp_path, qtype):
    from lightretriever_amd import FlatIPIndex, IVFSQ8Index, RefineFlatIndex, index_io
    idx, x, q = mid
    if qtype == "QT_8bit_uniform":
        idx = IVFSQ8Index(256, 64, qtype, nprobe=8)
        idx.set_contents(mid[0].centroids, torch.tensor([-4.0, 8.0]), mid[0].stored_codes(), mid[0].list_off, mid[0].row_ids)
    D, I = idx.search(q, 10)
    path = str(tmp_path / "i.ivfsq8.faiss")
    idx.save(path)
    assert open(path, "rb").read() == Y.file_bytes(idx.centroids.cpu().numpy(), idx.trained.cpu().numpy(), QT[qtype], idx.list_sizes, idx.stored_codes().cpu().numpy(),
                                                   idx.row_ids.cpu().numpy(), 8, True)
    st = index_io.read_ivf_sq8(path)
    assert (st["d"], st["nlist"], st["nprobe"], st["ntotal"], st["is_trained"], st["by_residual"], st["qtype"]) == (256, 64, 8, 5000, True, True, QT[qtype])
    back = IVFSQ8Index.load(path, id_base=7)
    assert (back.d, back.nlist, back.nprobe, back.by_residual, back.ntotal, back.id_base, back.is_trained, back.qtype) == (256, 64, 8, True, 5000, 7, True, qtype)
    assert torch.equal(bits(back.trained), bits(idx.trained))
    assert_same(back.search(q, 10), (D, I + 7))
    back.add(q[:10])                                                         # a loaded index takes further rows
    assert back.ntotal == 5010 and bool((back.search(q[:1], 3)[1] >= 0).all())
    # a refine index over it
    base = IVFSQ8Index.load(path)
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
    assert type(again.base_index) is IVFSQ8Index and (again.base_index.nprobe, again.base_index.by_residual, again.base_index.qtype, again.k_factor) == (8, True, qtype, 3.0)
    assert_same(again.search(q, 10), want)
    plain = IVFSQ8Index(256, 64, qtype, by_residual=False)
    plain.save(path)                                                         # untrained, no residuals
    back = IVFSQ8Index.load(path)
    assert not back.is_trained and not back.by_residual and back.ntotal == 0 and back.qtype == qtype


# ---- 11. HIP graph -----------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_search_replays_the_eager_bits(mid):
    idx, _, q = mid
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
    assert errors() == 0


# ---- 12. the searcher, the hybrid route, refine ------------------------------------------------------------------------------------------------------
def test_searcher_equals_the_index(trained, tmp_path, monkeypatch):
    from lightretriever_amd import IVFSQ8Index
    from lightretriever_amd.retriever import HybridSearch, IVFSQ8FaissSearch, _to_result_dict
    monkeypatch.setattr(IVFSQ8Index, "NITER", 2)                             # the searcher trains with the defaults: two iterations here
    x, q, _ = trained
    x, q = x[:300], q[:9]
    ids = [f"doc{i}" for i in range(300)]
    qids = [f"q{i}" for i in range(9)]
    s = HybridSearch(model=None, batch_size=8, faiss_search_map="ivfsq8", nlist=12, nprobe=5, by_residual=False, quantizer_type="QT_8bit_uniform",
                     show_progress_bar=False).dense_search
    assert isinstance(s, IVFSQ8FaissSearch)
    s.index(x, ids)
    idx = s.faiss_index.index
    assert type(idx) is IVFSQ8Index and (idx.nlist, idx.nprobe, idx.by_residual, idx.qtype, idx.ntotal, s.dim_size) == (12, 5, False, "QT_8bit_uniform", 300, 64)
    direct = IVFSQ8Index(64, 12, "QT_8bit_uniform", nprobe=5, by_residual=False)
    direct.train(x)
    direct.add(x)
    want = _to_result_dict(*direct.search(q, 20), qids, ids)
    got = s.retrieve_with_emb(q, qids, 20)
    assert got == want and all(len(v) == 20 for v in got.values())
    s.save(str(tmp_path), prefix="t")
    assert (tmp_path / "t.ivfsq8.faiss").exists() and (tmp_path / "t.ivfsq8.tsv").exists()
    c = IVFSQ8FaissSearch(model=None, batch_size=8, show_progress_bar=False)
    c.load(str(tmp_path), prefix="t")
    assert (c.nlist, c.nprobe, c.by_residual, c.quantizer_type, c.faiss_index.index.ntotal) == (12, 5, False, "QT_8bit_uniform", 300)
    assert c.retrieve_with_emb(q, qids, 20) == want
    # a chunk of fewer rows than nlist: one cell per row at the most
    t = IVFSQ8FaissSearch(model=None, nlist=1024, nprobe=32, batch_size=8, show_progress_bar=False)
    t.index(x[:280], ids[:280])
    assert (t.faiss_index.index.nlist, t.faiss_index.index.nprobe, t.faiss_index.index.by_residual, t.faiss_index.index.qtype) == (280, 32, True, "QT_8bit")
    assert len(t.retrieve_with_emb(q, qids, 5)["q0"]) == 5
    assert errors() == 0


@pytest.mark.parametrize("k_factor", [1, 2])
def test_refine_is_the_exact_rerank_of_the_bases_own_candidates(k_factor):
    from lightretriever_amd import FlatIPIndex, IVFSQ8Index, RefineFlatIndex
    rng = np.random.default_rng(9)
    n, d, nlist, k = 1500, 64, 8, 10
    x = rng.integers(-3, 4, (n, d)).astype(F32) + F32(0.25) * rng.integers(-2, 3, (n, d)).astype(F32)   # quarters: whatever the codes lose, the rerank's
    q = rng.integers(-3, 4, (5, d)).astype(F32)                                                        # fp64 sums over the fp32 rows stay exact
    base = IVFSQ8Index(d, nlist, nprobe=3)
    base.train(dev(x), niter=1)
    ref = RefineFlatIndex(base, FlatIPIndex(d), k_factor=k_factor)
    ref.add(dev(x))
    assert base.ntotal == n and ref.ntotal == n
    cand = base.search(dev(q), int(k * k_factor))[1].cpu().numpy()
    assert (cand >= 0).all()
    assert_yardstick(ref.search(dev(q), k), Y.rerank(q, x, cand, k))
    if k_factor == 1:
        assert np.array_equal(np.sort(ref.search(dev(q), k)[1].cpu().numpy(), axis=1), np.sort(cand, axis=1))
