"""GPU: the inverted-file product-quantised index (lrx_ivf_pq_ip_search, torch.ops.lrx.ivf_pq_ip_topk, ops.ivf_pq_ip_topk, IVFPQIndex,
IVFPQFaissSearch) against the numpy yardstick (tests/ivfpq_yardstick.py), PQIndex, IVFFlatIndex and RefineFlatIndex, bit for bit: without
residuals and probing every cell it is the PQ search; hand-made cells that start mid-block with every kind of bad probe entry; ties; batch
independence; training, adds in pieces, reconstruction; the refine identity; persistence, HIP graph, the searcher.  Codebooks are random normal
[M, 256, d / M] set through set_contents, except in the training tests (2 iterations).  Observed figures: DESIGN §5.4.11.

One case departs from the issue's text: the hand-made cells run at (d, M) = (64, 8) and (96, 24), not (64, 24) -- 24 does not divide 64, which
the entry point refuses (dim % M == 0); 96 is the smallest multiple of 32 that 24 divides, and M = 24 keeps what the case is for: two
16-sub-space groups, the second one half full."""
import numpy as np
import pytest
import torch

import ivf_yardstick as IV
import ivfpq_yardstick as Y

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


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


def blocked(codes, d):
    """Row-major uint8 [n, M] codes -> the blocked device buffer of the library."""
    from lightretriever_amd import PQIndex
    return PQIndex(d, codes.shape[1]).rows_to_blocked(torch.from_numpy(np.ascontiguousarray(codes)))


def ivfpq_c(q, codes_b, n, C, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    """lrx_ivf_pq_ip_search through ctypes with ld_probe = nprobe + 3: the padding entries name cell 0 and carry a score of 1e30 (read, they
    would add that cell's rows or lift a score)."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    q, C, list_off, probes = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, C, list_off, probes))
    row_ids = row_ids if row_ids is None or isinstance(row_ids, torch.Tensor) else dev(row_ids)
    (Q, D), npb, nlist, M = q.shape, probes.shape[1], list_off.numel() - 1, C.shape[0]
    pb = torch.zeros(Q, npb + 3, dtype=torch.int64, device="cuda")
    pb[:, :npb] = probes
    ps = None
    if base is not None:
        ps = torch.full((Q, npb + 3), 1e30, dtype=torch.float32, device="cuda")
        ps[:, :npb] = base if isinstance(base, torch.Tensor) else dev(np.asarray(base, np.float32))
    Do = torch.full((Q, k), 7.5, dtype=torch.float32, device="cuda")
    Io = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(l.lrx_ivf_pq_ip_workspace_bytes(n, nlist, D, M, Q, npb, k, max_scan), dtype=torch.uint8, device="cuda")
    _lib.check(l.lrx_ivf_pq_ip_search(_lib.ptr(codes_b), n, _lib.ptr(C.contiguous()), D, M, _lib.ptr(list_off), _lib.ptr(row_ids), nlist,
                                      _lib.ptr(q.contiguous()), Q, _lib.ptr(pb), _lib.ptr(ps), npb, npb + 3, int(by_residual), max_scan, k, id_base,
                                      _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    torch.cuda.synchronize()
    return Do, Io


def ivfpq_op(q, codes_b, C, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    from lightretriever_amd import torch_ops
    torch_ops.load()
    q, C, list_off, probes = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, C, list_off, probes))
    row_ids = row_ids if row_ids is None or isinstance(row_ids, torch.Tensor) else dev(row_ids)
    base = base if base is None or isinstance(base, torch.Tensor) else dev(np.asarray(base, np.float32))
    return torch.ops.lrx.ivf_pq_ip_topk(q, codes_b, C, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base, row_map)


def ivfpq_ops(q, codes_b, C, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base=0, row_map=None):
    from lightretriever_amd import ops
    q, C, list_off, probes = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, C, list_off, probes))
    row_ids = row_ids if row_ids is None or isinstance(row_ids, torch.Tensor) else dev(row_ids)
    base = base if base is None or isinstance(base, torch.Tensor) else dev(np.asarray(base, np.float32))
    return ops.ivf_pq_ip_topk(q, codes_b, C, list_off, row_ids, probes, base, by_residual, k, max_scan, id_base, row_map)


def random_index(n, d, M, nlist, nprobe, by_residual, seed, **kw):
    """An IVFPQIndex over random centroids, random codebooks and random codes dealt to the cells at random -> (idx, codes by original row, cells)."""
    from lightretriever_amd import IVFPQIndex
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    idx = IVFPQIndex(d, nlist, M, nprobe=nprobe, by_residual=by_residual, **kw)
    idx.set_contents(cent, C, codes[row_ids], list_off, row_ids)
    return idx, codes, cells


# ---- 1. without residuals, probing every cell: the PQ index -----------------------------------------------------------------------------
@pytest.mark.parametrize("Q, n, d, M, nlist, k", [(1, 5, 32, 4, 1, 5), (3, 300, 96, 6, 7, 10), (4, 700, 288, 144, 16, 10), (130, 5000, 256, 32, 64, 100),
                                                  (5, 3000, 128, 16, 4, 2048)])
def test_probing_every_cell_without_residuals_equals_the_pq_index(Q, n, d, M, nlist, k):
    from lightretriever_amd import PQIndex
    idx, codes, _ = random_index(n, d, M, nlist, nlist, False, n + d)
    pq = PQIndex(d, M)
    pq.set_contents(idx.pq.centroids, torch.from_numpy(codes))
    q = torch.randn(Q, d, generator=torch.Generator(device="cuda").manual_seed(n), device="cuda")
    assert idx.ntotal == n and idx.max_scan_rows() == n
    errors()
    assert_same(idx.search(q, k), pq.search(q, k))
    assert errors() == 0


# ---- 2. hand-made cells -------------------------------------------------------------------------------------------------------------------
NLIST = 12
SIZES = [0, 1, 127, 128, 129, 3, 0, 1500, 2, 64, 700, 5]      # cells start mid-block, one tile spans several cells, cell 7 spans two tiles


class Cells:
    def __init__(self, d, M):
        rng = np.random.default_rng(d + M)
        n = sum(SIZES)
        cells = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
        self.d, self.M, self.n, self.rng, self.cells = d, M, n, rng, cells
        self.C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
        self.codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
        self.q = rng.standard_normal((6, d)).astype(np.float32)
        self.row_ids, self.list_off = IV.cell_order(cells, NLIST)
        self.stored = self.codes[self.row_ids]
        self.dcodes, self.dC, self.dq, self.doff, self.dids = blocked(self.stored, d), dev(self.C), dev(self.q), dev(self.list_off), dev(self.row_ids)

    def all(self, probes, k, base=None, by_residual=True, max_scan=None, row_ids=True):
        """The C call, the torch op and ops over `probes`, each against the yardstick; returns the C call's result."""
        probes = np.asarray(probes, np.int64)
        if base is None and by_residual:
            base = (3 * self.rng.standard_normal(probes.shape)).astype(np.float32)
        scan = self.n if max_scan is None else max_scan
        want = Y.search(self.q, self.C, self.stored, self.list_off, self.row_ids if row_ids else None, probes, base, by_residual, k, max_scan_rows=max_scan)
        ids = self.dids if row_ids else None
        got = ivfpq_c(self.dq, self.dcodes, self.n, self.dC, self.doff, ids, probes, base, by_residual, k, scan)
        assert_yardstick(got, want)
        assert_yardstick(ivfpq_op(self.dq, self.dcodes, self.dC, self.doff, ids, probes, base, by_residual, k, scan), want)
        assert_yardstick(ivfpq_ops(self.dq, self.dcodes, self.dC, self.doff, ids, probes, base, by_residual, k, scan), want)
        return got, want


@pytest.fixture(scope="module", params=[(64, 8), (96, 24)])
def cells(request):
    return Cells(*request.param)


@pytest.mark.parametrize("nprobe", [1, 3, 9])
def test_hand_made_cells_against_the_yardstick(cells, nprobe):
    probes = np.stack([cells.rng.permutation(NLIST)[:nprobe] for _ in range(6)])
    if nprobe == 1:
        probes[:, 0] = [7, 0, 1, 5, 4, 3]                                    # two tiles, the empty cell, 1 row, 3 rows, 129 rows, 128 rows
    errors()
    got, _ = cells.all(probes, 10)
    assert errors() == 0
    if nprobe == 1:
        assert (got[1][1] == -1).all() and (got[0][1] == -FLT_MAX).all()     # only the empty cell: all padding
        assert (got[1][2, 1:] == -1).all() and got[1][2, 0] >= 0             # one row, then padding
        assert (got[1][3, 3:] == -1).all() and (got[1][3, :3] >= 0).all()
    cells.all(probes, 10, by_residual=False)                                 # the same cells without a base term (probe_scores = NULL)


# ---- 3. edges -------------------------------------------------------------------------------------------------------------------------------
def test_k_beyond_the_scanned_rows_pads_the_tail(cells):
    got, _ = cells.all([[5, 8], [1, 0], [0, 6], [8, 1], [11, 5], [5, 1]], 20)
    assert (got[1][0, :5] >= 0).all() and (got[1][0, 5:] == -1).all() and (got[0][0, 5:] == -FLT_MAX).all()
    assert (got[1][2] == -1).all()
    every = [[7, 0, 10, 2, 3, 4, 9, 11, 1, 5, 6, 8]] * 6
    got, _ = cells.all(every, 2048)                                          # every row (2659): the radix-select path at the largest k
    assert (got[1] >= 0).all()


def test_a_cell_named_twice_is_scanned_once_with_its_first_base_and_minus_one_is_skipped(cells):
    errors()
    probes = np.array([[5, 5, 5], [4, 0, 4], [-1, 1, -1], [-1, -1, -1], [7, -1, 7], [1, 5, 1]])
    base = (3 * cells.rng.standard_normal(probes.shape)).astype(np.float32)
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
    assert (ids[0] >= 0).sum() == 3 and (ids[2] >= 0).sum() == 1 and (ids[3] >= 0).sum() == 0 and (ids[4] >= 0).sum() == 12
    assert errors() == 0


def test_probe_entries_past_nlist_are_skipped_and_counted(cells):
    errors()
    probes = [[NLIST, 5, 1], [2 ** 40, 2 ** 40, 4], [0, 1, 2], [NLIST, NLIST, NLIST], [7, -1, 2 ** 40], [2 ** 62, 0, NLIST + 1]]
    cells.all(probes, 10)                                                    # (three calls: the C entry point, the op, ops)
    assert errors() == 3 * 9
    assert errors() == 0                                                     # the read above reset the count


def test_a_query_over_max_scan_rows_is_padding_and_its_neighbours_are_unchanged(cells):
    probes = [[1, 5], [7, 4], [2, 3], [8, 9], [7, 10], [11, 2]]
    totals = [SIZES[a] + SIZES[b] for a, b in probes]
    base = (3 * cells.rng.standard_normal((6, 2))).astype(np.float32)
    errors()
    full, _ = cells.all(probes, 10, base=base)
    assert errors() == 0
    scan = totals[1] - 1                                                     # query 1 holds one row too many (1500 + 129); so does query 4 (1500 + 700)
    got, _ = cells.all(probes, 10, base=base, max_scan=scan)
    assert errors() == 3 * 2
    for i in range(6):
        if totals[i] > scan:
            assert (got[1][i] == -1).all() and (got[0][i] == -FLT_MAX).all()
        else:
            assert torch.equal(got[1][i], full[1][i]) and torch.equal(bits(got[0][i]), bits(full[0][i]))
    assert [t > scan for t in totals] == [False, True, False, False, True, False]


def test_positions_are_rows_without_row_ids(cells):
    got, _ = cells.all([[7, 2], [0, 8], [3, 4], [6, 7], [1, 1], [2, 0]], 10, row_ids=False)
    assert int(got[1].max()) < cells.n


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, nlist, k", [(600, 8, 50), (6000, 4, 100), (6000, 4, 2048)])      # under 2048 scanned rows (sorted whole); above (radix select)
@pytest.mark.parametrize("by_residual", [True, False])
def test_ties_go_to_the_lower_original_row(n, nlist, k, by_residual):
    rng = np.random.default_rng(n + k)
    d, M = 32, 4
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    proto = rng.integers(0, 256, (12, M)).astype(np.uint8)                   # 12 distinct code rows: identical codes inside and across the cells
    codes = proto[rng.integers(0, 12, n)]
    q = rng.standard_normal((5, d)).astype(np.float32)
    q[3] = 0                                                                 # every table entry +0.0
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    stored = codes[row_ids]
    probes = np.stack([rng.permutation(nlist)[:nlist - 1] for _ in range(5)])
    base = rng.integers(-2, 3, probes.shape).astype(np.float32) if by_residual else None
    if by_residual:
        base[3] = 0.25                                                       # one base for all cells of the zero query: every score equal
    want = Y.search(q, C, stored, list_off, row_ids, probes, base, by_residual, k)
    assert np.mean(want[0][:, 1:] == want[0][:, :-1]) > 0.5                  # ties everywhere in the result
    cb = blocked(stored, d)
    got = ivfpq_c(q, cb, n, C, list_off, row_ids, probes, base, by_residual, k, n)
    assert_yardstick(got, want)
    assert_yardstick(ivfpq_op(q, cb, C, list_off, row_ids, probes, base, by_residual, k, n), want)
    scanned = np.sort(np.flatnonzero(np.isin(cells, probes[3])))
    assert scanned.size > 2048 or n == 600
    kk = min(k, scanned.size)
    assert np.array_equal(got[1][3].cpu().numpy()[:kk], scanned[:kk])        # the all-zero query: the lowest original rows of its cells
    assert (got[0][3][:kk] == (0.25 if by_residual else 0.0)).all()


# ---- 5. batch independence ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    """5000 random code rows of M = 32 over d = 256 in 64 cells, by residual, nprobe 8; 130 queries."""
    idx, codes, cells = random_index(5000, 256, 32, 64, 8, True, 11)
    q = torch.randn(130, 256, generator=torch.Generator(device="cuda").manual_seed(11), device="cuda")
    idx.search(q[:1], 1)
    return idx, codes, cells, q


def test_a_query_does_not_depend_on_its_batch(mid):
    idx, _, _, q = mid
    K = 100
    whole = idx.search(q, K)
    for i in range(130):
        alone = idx.search(q[i:i + 1], K)
        assert torch.equal(alone[1][0], whole[1][i]) and torch.equal(bits(alone[0][0]), bits(whole[0][i])), i
    first = idx.search(q[77:79], K)
    assert torch.equal(first[1][0], whole[1][77]) and torch.equal(bits(first[0][0]), bits(whole[0][77]))
    # a different scan bound (another layout of the workspace) changes nothing either
    ps, pr = idx.quantizer.search(q, 8)
    args = (idx.pq._codes, idx.pq.centroids, idx.list_off, idx.row_ids, pr, ps, True, K)
    assert_same(ivfpq_op(q, *args, idx.ntotal), whole)
    assert_same(ivfpq_op(q, *args, idx.max_scan_rows(8)), whole)
    held = idx.list_sizes[pr.cpu().numpy()].sum(axis=1)                      # every query reports min(K, the rows of its cells) rows
    assert np.array_equal((whole[1] >= 0).sum(dim=1).cpu().numpy(), np.minimum(held, K))


def test_the_index_agrees_with_the_yardstick(mid):
    idx, codes, cells, q = mid
    qs = q[:7]
    ps, pr = idx.quantizer.search(qs, 8)
    want = Y.search(qs.cpu().numpy(), idx.pq.centroids.cpu().numpy(), idx.stored_codes().cpu().numpy(), idx.list_off.cpu().numpy(), idx.row_ids.cpu().numpy(),
                    pr.cpu().numpy(), ps.cpu().numpy(), True, 20, id_base=5)
    idx.id_base = 5
    got = idx.search(qs, 20)
    idx.id_base = 0
    assert_yardstick(got, want)
    rm = torch.arange(5000, device="cuda") * 3 + 7
    D, I = idx.search(qs, 20)
    assert_same(idx.search(qs, 20, row_map=rm), (D, I * 3 + 7))
    assert torch.equal(idx.stored_codes().cpu(), torch.from_numpy(codes)[idx.row_ids.cpu()])
    assert torch.equal(idx._assign[:5000].cpu(), torch.from_numpy(cells))


# ---- 6. the class: training, adds, reconstruction ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """4000 x 64 clustered rows, nlist 16, M 8, trained with 2 iterations, all rows added."""
    from lightretriever_amd import IVFPQIndex
    x, q = IV.clustered_corpus(n=4000, d=64, n_clusters=40)
    x, q = dev(x), dev(q)
    idx = IVFPQIndex(64, 16, 8, nprobe=4)
    idx.train(x, niter=2)
    idx.add(x)
    return x, q, idx


def cells_and_residuals(idx, x):
    cells = idx.quantizer.search(x, 1)[1][:, 0]
    return cells, x - idx.centroids[cells]


def test_training_is_deterministic_and_is_the_two_trainings_it_is_made_of(trained):
    from lightretriever_amd import IVFFlatIndex, IVFPQIndex, PQIndex
    x, q, idx = trained
    again = IVFPQIndex(64, 16, 8)
    again.train(x, niter=2)
    assert torch.equal(bits(again.centroids), bits(idx.centroids)) and torch.equal(bits(again.pq.centroids), bits(idx.pq.centroids))
    flat = IVFFlatIndex(64, 16)
    flat.train(x, niter=2)
    assert torch.equal(bits(idx.centroids), bits(flat.centroids))            # the coarse quantiser is IVFFlatIndex's
    _, res = cells_and_residuals(idx, x)
    pq = PQIndex(64, 8)
    pq.train(res, niter=2)
    assert torch.equal(bits(idx.pq.centroids), bits(pq.centroids))           # the codebooks are PQIndex's over the residuals
    plain = IVFPQIndex(64, 16, 8, by_residual=False)
    plain.train(x, niter=2)
    pq.train(x, niter=2)
    assert torch.equal(bits(plain.pq.centroids), bits(pq.centroids)) and torch.equal(bits(plain.centroids), bits(flat.centroids))
    with pytest.raises(ValueError, match="255 training rows"):
        IVFPQIndex(64, 16, 8).train(x[:255])


def test_the_sampled_residuals_train_what_all_residuals_train():
    """More rows than PQIndex samples (65536): the index draws the sample first and takes residuals of those rows only."""
    from lightretriever_amd import IVFPQIndex, PQIndex
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(66000, 32, generator=g, device="cuda")
    idx = IVFPQIndex(32, 4, 4)
    idx.train(x, niter=1)
    _, res = cells_and_residuals(idx, x)
    pq = PQIndex(32, 4)
    pq.train(res, niter=1)
    assert torch.equal(bits(idx.pq.centroids), bits(pq.centroids))


def test_adds_in_pieces_equal_one_add_and_rows_reconstruct(trained):
    from lightretriever_amd import IVFPQIndex, PQIndex
    x, q, idx = trained
    want = idx.search(q, 20)
    b = IVFPQIndex(64, 16, 8, nprobe=4)
    with pytest.raises(RuntimeError, match="not trained"):
        b.add(x[:1])
    b.set_contents(idx.centroids, idx.pq.centroids, torch.zeros(0, 8, dtype=torch.uint8), np.zeros(17, np.int64), np.zeros(0, np.int64))
    for piece in (x[:1], x[1:128], x[128:]):
        b.add(piece)
    assert b.ntotal == 4000
    assert_same(b.search(q, 20), want)
    assert torch.equal(b.list_off, idx.list_off) and torch.equal(b.row_ids, idx.row_ids) and torch.equal(b.stored_codes(), idx.stored_codes())
    assert np.array_equal(b.list_sizes, idx.list_sizes)
    off, ids = b.list_off.cpu().numpy(), b.row_ids.cpu().numpy()
    assert all((np.diff(ids[off[c]:off[c + 1]]) > 0).all() for c in range(16))       # ascending original row inside every cell
    # add -> search -> add -> search equals a fresh index with all rows
    c = IVFPQIndex(64, 16, 8, nprobe=4)
    c.set_contents(idx.centroids, idx.pq.centroids, torch.zeros(0, 8, dtype=torch.uint8), np.zeros(17, np.int64), np.zeros(0, np.int64))
    c.add(x[:3000])
    part = c.search(q, 20)
    assert int((part[1] >= 3000).sum()) == 0
    c.add(x[3000:])
    assert_same(c.search(q, 20), want)
    assert torch.equal(c.row_ids, idx.row_ids) and torch.equal(c.stored_codes(), idx.stored_codes())
    # the codes are PQIndex's codes of the residuals; a row reconstructs as centroid[cell] + their decode (one fp32 add)
    cells, res = cells_and_residuals(idx, x)
    pq = PQIndex(64, 8)
    pq.set_contents(idx.pq.centroids, torch.zeros(0, 8, dtype=torch.uint8))
    pq.add(res)
    back = torch.empty(4000, 8, dtype=torch.uint8, device="cuda")
    back[idx.row_ids] = idx.stored_codes()
    assert torch.equal(back, pq.codes())
    recon = idx.centroids[cells] + pq.reconstruct_n(0, 4000)
    assert torch.equal(bits(idx.reconstruct_n(0, 4000)), bits(recon)) and torch.equal(bits(idx.reconstruct_n(3990, 7)), bits(recon[3990:3997]))
    # reset() keeps the training
    c.reset()
    assert c.ntotal == 0 and c.is_trained and (c.search(q[:2], 5)[1] == -1).all()
    c.add(x)
    assert_same(c.search(q, 20), want)


def test_without_residuals_rows_reconstruct_as_the_decode_alone(trained):
    from lightretriever_amd import IVFPQIndex, PQIndex
    x, q, idx = trained
    plain = IVFPQIndex(64, 16, 8, nprobe=16, by_residual=False)
    plain.set_contents(idx.centroids, idx.pq.centroids, torch.zeros(0, 8, dtype=torch.uint8), np.zeros(17, np.int64), np.zeros(0, np.int64))
    plain.add(x[:1000])
    pq = PQIndex(64, 8)
    pq.set_contents(idx.pq.centroids, torch.zeros(0, 8, dtype=torch.uint8))
    pq.add(x[:1000])
    assert torch.equal(bits(plain.reconstruct_n(0, 1000)), bits(pq.reconstruct_n(0, 1000)))
    assert_same(plain.search(q, 10), pq.search(q, 10))                       # every cell probed: the PQ index


def test_append_slot_and_commit_train_an_untrained_index(trained):
    from lightretriever_amd import IVFPQIndex
    x, q, _ = trained
    a = IVFPQIndex(64, 16, 8, nprobe=4)
    a.NITER = a.pq.NITER = 2                                                 # commit() trains with the defaults: two iterations here
    slot = a.append_slot(2000)
    slot.copy_(x[:2000])
    a.commit(2000)
    assert a.is_trained and a.pq.is_trained and a.ntotal == 2000
    b = IVFPQIndex(64, 16, 8, nprobe=4)
    b.train(x[:2000], niter=2)
    b.add(x[:2000])
    assert torch.equal(bits(a.centroids), bits(b.centroids)) and torch.equal(bits(a.pq.centroids), bits(b.pq.centroids))
    assert_same(a.search(q, 10), b.search(q, 10))
    with pytest.raises(ValueError, match="staged"):
        a.commit(5)


def test_refusals(trained):
    from lightretriever_amd import IVFPQIndex
    x, q, idx = trained
    with pytest.raises(RuntimeError, match="not trained"):
        IVFPQIndex(64, 16, 8).add(x[:1])
    with pytest.raises(RuntimeError, match="not trained"):
        IVFPQIndex(64, 16, 8).search(q, 1)
    with pytest.raises(ValueError, match="k=2049"):
        idx.search(q, 2049)
    with pytest.raises(ValueError, match="nprobe=17"):
        idx.search(q, 10, nprobe=17)
    with pytest.raises(ValueError, match="row_map"):
        idx.search(q, 10, row_map=torch.arange(10, device="cuda"))
    with pytest.raises(NotImplementedError, match="range_search"):
        idx.range_search(q, 0.0)
    with pytest.raises(ValueError, match="codes must be uint8"):
        idx.set_contents(idx.centroids, idx.pq.centroids, torch.zeros(3, 7, dtype=torch.uint8), np.zeros(17, np.int64), np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="list_off"):
        idx.set_contents(idx.centroids, idx.pq.centroids, torch.zeros(3, 8, dtype=torch.uint8), np.zeros(17, np.int64), np.arange(3))
    assert idx.search(q[:0], 10)[0].shape == (0, 10) and idx.ntotal == 4000


# ---- 7. the refine identity ---------------------------------------------------------------------------------------------------------------------
def test_refine_over_every_scanned_row_is_the_ivf_flat_search():
    from lightretriever_amd import IVFFlatIndex, IVFPQIndex, RefineFlatIndex
    x, q = IV.clustered_corpus(n=1500, d=64, n_clusters=20)
    x, q = dev(x), dev(q)
    flat = IVFFlatIndex(64, 8, nprobe=2)
    flat.train(x, niter=2)
    flat.add(x)
    base = IVFPQIndex(64, 8, 8, nprobe=2)
    base.train(x, niter=2)
    assert torch.equal(bits(base.centroids), bits(flat.centroids))
    ref = RefineFlatIndex(base, k_factor=200)
    ref.add(x)
    k = 10
    assert int(k * ref.k_factor) == 2000 and base.max_scan_rows() <= 2000 and base.ntotal == 1500
    assert_same(ref.search(q, k), flat.search(q, k))


# ---- 8. persistence ---------------------------------------------------------------------------------------------------------------------------------
def test_save_and_load_round_trip(mid, tmp_path):
    from lightretriever_amd import FlatIPIndex, IVFPQIndex, RefineFlatIndex, index_io
    idx, _, _, q = mid
    D, I = idx.search(q, 10)
    path = str(tmp_path / "i.ivfpq.faiss")
    idx.save(path)
    assert open(path, "rb").read() == Y.file_bytes(idx.centroids.cpu().numpy(), idx.pq.centroids.cpu().numpy(), idx.list_sizes, idx.stored_codes().cpu().numpy(),
                                                   idx.row_ids.cpu().numpy(), 8, True)
    st = index_io.read_ivf_pq(path)
    assert (st["d"], st["nlist"], st["nprobe"], st["ntotal"], st["is_trained"], st["by_residual"], st["M"]) == (256, 64, 8, 5000, True, True, 32)
    back = IVFPQIndex.load(path, id_base=7)
    assert (back.d, back.nlist, back.nprobe, back.M, back.by_residual, back.ntotal, back.id_base, back.is_trained) == (256, 64, 8, 32, True, 5000, 7, True)
    assert_same(back.search(q, 10), (D, I + 7))
    back.add(q[:10])                                                         # a loaded index takes further rows
    assert back.ntotal == 5010 and bool((back.search(q[:1], 3)[1] >= 0).all())
    # a refine index over it
    x = torch.randn(5000, 256, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    base = IVFPQIndex.load(path)
    store = FlatIPIndex(256)
    store.shadow_f16 = False
    store.add(x)
    ref = RefineFlatIndex(base, store, k_factor=3)
    want = ref.search(q, 10)
    rpath = str(tmp_path / "r.refine.faiss")
    ref.save(rpath)
    st = index_io.read_refine(rpath)
    assert st["base"]["fourcc"] == b"IwPQ" and st["k_factor"] == 3.0
    again = RefineFlatIndex.load(rpath)
    assert type(again.base_index) is IVFPQIndex and (again.base_index.nprobe, again.base_index.by_residual, again.k_factor) == (8, True, 3.0)
    assert_same(again.search(q, 10), want)
    plain = IVFPQIndex(256, 64, 32, by_residual=False)
    plain.save(path)                                                         # untrained, no residuals
    back = IVFPQIndex.load(path)
    assert not back.is_trained and not back.by_residual and back.ntotal == 0


# ---- 9. HIP graph -----------------------------------------------------------------------------------------------------------------------------------
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
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert_same((Dg, Ig), eager)
    want = tuple(t.clone() for t in idx.search(q[16:32], 10))
    qbuf.copy_(q[16:32])
    graph.replay()
    torch.cuda.synchronize()
    assert_same((Dg, Ig), want)


# ---- 10. the searcher -------------------------------------------------------------------------------------------------------------------------------
def test_searcher_equals_the_index(trained, tmp_path, monkeypatch):
    from lightretriever_amd import IVFPQIndex, PQIndex
    from lightretriever_amd.retriever import HybridSearch, IVFPQFaissSearch, _to_result_dict
    monkeypatch.setattr(IVFPQIndex, "NITER", 2)                              # the searcher trains with the defaults: two iterations here
    monkeypatch.setattr(PQIndex, "NITER", 2)
    x, q, _ = trained
    x, q = x[:300], q[:9]
    ids = [f"doc{i}" for i in range(300)]
    qids = [f"q{i}" for i in range(9)]
    s = HybridSearch(model=None, batch_size=8, faiss_search_map="ivfpq", nlist=12, nprobe=5, num_of_centroids=8, by_residual=False,
                     show_progress_bar=False).dense_search
    assert isinstance(s, IVFPQFaissSearch)
    s.index(x, ids)
    idx = s.faiss_index.index
    assert type(idx) is IVFPQIndex and (idx.nlist, idx.nprobe, idx.M, idx.by_residual, idx.ntotal, s.dim_size) == (12, 5, 8, False, 300, 64)
    direct = IVFPQIndex(64, 12, 8, nprobe=5, by_residual=False)
    direct.train(x)
    direct.add(x)
    want = _to_result_dict(*direct.search(q, 20), qids, ids)
    got = s.retrieve_with_emb(q, qids, 20)
    assert got == want and all(len(v) == 20 for v in got.values())
    s.save(str(tmp_path), prefix="t")
    assert (tmp_path / "t.ivfpq.faiss").exists() and (tmp_path / "t.ivfpq.tsv").exists()
    c = IVFPQFaissSearch(model=None, batch_size=8, show_progress_bar=False)
    c.load(str(tmp_path), prefix="t")
    assert (c.nlist, c.nprobe, c.num_of_centroids, c.by_residual, c.faiss_index.index.ntotal) == (12, 5, 8, False, 300)
    assert c.retrieve_with_emb(q, qids, 20) == want
    # a chunk of fewer rows than nlist: one cell per row at the most
    t = IVFPQFaissSearch(model=None, nlist=1024, nprobe=32, num_of_centroids=8, batch_size=8, show_progress_bar=False)
    t.index(x[:280], ids[:280])
    assert (t.faiss_index.index.nlist, t.faiss_index.index.nprobe) == (280, 32)
    assert len(t.retrieve_with_emb(q, qids, 5)["q0"]) == 5
