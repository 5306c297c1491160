"""GPU: the inverted-file flat index (lrx_ivf_flat_ip_search, torch.ops.lrx.ivf_flat_ip_topk, IVFFlatIndex, IVFFaissSearch) against the numpy
yardstick (tests/ivf_yardstick.py), the flat index and lrx_flat_ip_rerank, bit for bit: nprobe == nlist equals the flat search, hand-made
cells with every kind of bad probe entry, ties, batch independence, nesting of the probe sets, adds in pieces, training, and the plumbing
(ids, persistence, HIP graph, the searcher).  Observed figures: DESIGN §5.4.10."""
import numpy as np
import pytest
import torch

import ivf_yardstick as Y

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


def ivf_c(q, X, list_off, row_ids, probes, k, max_scan, id_base=0, row_map=None):
    """lrx_ivf_flat_ip_search through ctypes with ldx = D + 8 (padding columns 1e30: never read into a result) and ld_probe = nprobe + 3 (the
    padding entries name cell 0: read, they would add that cell's rows)."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    q, X, list_off, probes = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, X, list_off, probes))
    row_ids = row_ids if row_ids is None or isinstance(row_ids, torch.Tensor) else dev(row_ids)
    (Q, D), n, npb, nlist = q.shape, X.shape[0], probes.shape[1], list_off.numel() - 1
    xb = torch.full((n, D + 8), 1e30, dtype=torch.float32, device="cuda")
    xb[:, :D] = X
    pb = torch.zeros(Q, npb + 3, dtype=torch.int64, device="cuda")
    pb[:, :npb] = probes
    Do = torch.full((Q, k), 7.5, dtype=torch.float32, device="cuda")
    Io = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(l.lrx_ivf_flat_ip_workspace_bytes(n, nlist, D, Q, npb, k, max_scan), dtype=torch.uint8, device="cuda")
    _lib.check(l.lrx_ivf_flat_ip_search(_lib.ptr(xb), n, D + 8, D, _lib.ptr(list_off), _lib.ptr(row_ids), nlist, _lib.ptr(q.contiguous()), Q, _lib.ptr(pb), npb,
                                        npb + 3, max_scan, k, id_base, _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(),
                                        _lib.current_stream()))
    torch.cuda.synchronize()
    return Do, Io


def ivf_op(q, X, list_off, row_ids, probes, k, max_scan, id_base=0, row_map=None):
    from lightretriever_amd import torch_ops
    torch_ops.load()
    q, X, list_off, probes = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, X, list_off, probes))
    row_ids = row_ids if row_ids is None or isinstance(row_ids, torch.Tensor) else dev(row_ids)
    return torch.ops.lrx.ivf_flat_ip_topk(q, X, list_off, row_ids, probes, k, max_scan, id_base, row_map)


def rerank_flat(q, X, cand, k):
    from lightretriever_amd import _lib
    l = _lib.lib()
    q, X, cand = dev(q), dev(X), dev(cand)
    Q, nc = cand.shape
    Do = torch.empty(Q, k, dtype=torch.float32, device="cuda")
    Io = torch.empty(Q, k, dtype=torch.int64, device="cuda")
    ws = torch.empty(l.lrx_ip_rerank_workspace_bytes(Q, nc, k), dtype=torch.uint8, device="cuda")
    _lib.check(l.lrx_flat_ip_rerank(_lib.ptr(X), X.shape[0], X.shape[1], X.shape[1], _lib.ptr(q), Q, _lib.ptr(cand), nc, nc, k, 0, _lib.ptr(Do), _lib.ptr(Io),
                                    None, _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    torch.cuda.synchronize()
    return Do, Io


def trained(x, nlist, nprobe=1, niter=None, **kw):
    from lightretriever_amd import IVFFlatIndex
    idx = IVFFlatIndex(x.shape[1], nlist, nprobe=nprobe, **kw)
    idx.train(x, niter=niter)
    return idx


# ---- 1. nprobe == nlist is the flat index ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q, n, d, nlist, k", [(1, 5, 32, 1, 5), (3, 300, 96, 7, 10), (4, 600, 2112, 16, 10), (130, 5000, 256, 64, 100), (5, 3000, 2048, 32, 2048)])
def test_probing_every_cell_equals_the_flat_index(Q, n, d, nlist, k):
    from lightretriever_amd import FlatIPIndex
    g = torch.Generator(device="cuda").manual_seed(n + d)
    x = torch.randn(n, d, generator=g, device="cuda")
    q = torch.randn(Q, d, generator=g, device="cuda")
    idx = trained(x, nlist, nprobe=nlist, niter=2)
    idx.add(x)
    flat = FlatIPIndex(d)
    flat.add(x)
    assert idx.ntotal == n and int(idx.list_sizes.sum()) == n and idx.max_scan_rows() == n
    assert_same(idx.search(q, k), flat.search(q, k))


# ---- 2. hand-made cells ----------------------------------------------------------------------------------------------------------------
NLIST = 9
SIZES = [130, 0, 1, 7, 9, 520, 111, 100, 122]         # an empty cell, 1 row, 7 (under a row group at d = 2048), 9, more than half of the 1000 rows


class Cells:
    def __init__(self, d):
        rng = np.random.default_rng(d)
        n = sum(SIZES)
        cells = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
        self.d, self.n = d, n
        self.X = rng.integers(-3, 4, (n, d)).astype(np.float32)              # integers: every partial sum is exact, in any order
        self.q = rng.integers(-3, 4, (6, d)).astype(np.float32)
        self.cells = cells
        self.row_ids, self.list_off = Y.cell_order(cells, NLIST)
        self.stored = self.X[self.row_ids]
        self.rng = rng
        self.dX, self.dq, self.doff, self.dids = dev(self.stored), dev(self.q), dev(self.list_off), dev(self.row_ids)

    def both(self, probes, k, max_scan=None, q=None):
        """The C call and the op over `probes`, each against the yardstick; returns the C call's result."""
        q = self.q if q is None else q
        probes = np.asarray(probes, np.int64)
        scan = self.n if max_scan is None else max_scan
        want = Y.search(q, self.stored, self.list_off, self.row_ids, probes, k, max_scan_rows=max_scan)
        got = ivf_c(q, self.dX, self.doff, self.dids, probes, k, scan)
        assert_yardstick(got, want)
        assert_yardstick(ivf_op(q, self.dX, self.doff, self.dids, probes, k, scan), want)
        return got, want


@pytest.fixture(scope="module", params=[64, 2048])
def cells(request):
    return Cells(request.param)


@pytest.mark.parametrize("nprobe", [1, 3, 9])
def test_hand_made_cells_against_the_yardstick_and_the_rerank(cells, nprobe):
    probes = np.stack([cells.rng.permutation(NLIST)[:nprobe] for _ in range(6)])
    if nprobe == 1:
        probes[:, 0] = [5, 1, 2, 3, 4, 0]                                    # the large cell, the empty one, 1 row, 7 rows, 9 rows
    errors()
    got, want = cells.both(probes, 10)
    assert errors() == 0
    # the rerank fed the same rows as candidates: the same device function scores them
    cand = np.full((6, cells.n), -1, np.int64)
    for i in range(6):
        rows = np.flatnonzero(np.isin(cells.cells, probes[i]))
        cand[i, :rows.size] = rows
    assert_same(got, rerank_flat(cells.q, cells.X, cand, 10))
    if nprobe == 1:
        assert (got[1][1] == -1).all() and (got[0][1] == -FLT_MAX).all()     # only the empty cell: all padding
        assert (got[1][2, 1:] == -1).all() and got[1][2, 0] >= 0             # one row, then padding
        assert (got[1][3, 7:] == -1).all() and (got[1][3, :7] >= 0).all()


def test_k_beyond_the_scanned_rows_pads_the_tail(cells):
    got, _ = cells.both([[3, 4], [2, 1], [1, 1], [4, 2], [0, 3], [3, 2]], 20)
    assert (got[1][0, :16] >= 0).all() and (got[1][0, 16:] == -1).all() and (got[0][0, 16:] == -FLT_MAX).all()
    assert (got[1][2] == -1).all()
    cells.both([[5, 0, 6, 7, 8, 2, 3, 4, 1]] * 6, 1000)                      # every row: the top 1000 of 1000
    cells.both([[5, 0, 6, 7, 8, 2, 3, 4, 1]] * 6, 2048)


def test_a_cell_named_twice_is_scanned_once_and_minus_one_is_skipped(cells):
    errors()
    got, _ = cells.both([[3, 3, 3], [4, 0, 4], [-1, 2, -1], [-1, -1, -1], [5, -1, 5], [2, 3, 2]], 12)
    ids = got[1].cpu().numpy()
    for i in range(6):
        valid = ids[i][ids[i] >= 0]
        assert len(set(valid.tolist())) == valid.size                        # no row twice
    assert (ids[0] >= 0).sum() == 7 and (ids[2] >= 0).sum() == 1 and (ids[3] >= 0).sum() == 0
    assert errors() == 0


def test_probe_entries_past_nlist_are_skipped_and_counted(cells):
    errors()
    probes = [[NLIST, 3, 2], [2 ** 40, 2 ** 40, 4], [0, 1, 2], [NLIST, NLIST, NLIST], [5, -1, 2 ** 40], [2 ** 62, 0, NLIST + 1]]
    cells.both(probes, 10)                                                   # (two calls: the C entry point and the op)
    assert errors() == 2 * 9
    assert errors() == 0                                                     # the read above reset the count


def test_a_query_over_max_scan_rows_is_padding_and_its_neighbours_are_unchanged(cells):
    probes = [[0, 3], [5, 4], [6, 7], [2, 3], [5, 8], [4, 2]]
    totals = [SIZES[a] + SIZES[b] for a, b in probes]
    errors()
    full, _ = cells.both(probes, 10)
    assert errors() == 0
    scan = totals[1] - 1                                                     # query 1 holds one row too many; so does query 4 (520 + 122)
    got, _ = cells.both(probes, 10, max_scan=scan)
    assert errors() == 2 * 2
    for i in range(6):
        if totals[i] > scan:
            assert (got[1][i] == -1).all() and (got[0][i] == -FLT_MAX).all()
        else:
            assert torch.equal(got[1][i], full[1][i]) and torch.equal(bits(got[0][i]), bits(full[0][i]))
    assert [t > scan for t in totals] == [False, True, False, False, True, False]


def test_positions_are_rows_without_row_ids(cells):
    probes = [[5, 2], [0, 8], [3, 4], [6, 7], [1, 1], [2, 0]]
    want = Y.search(cells.q, cells.stored, cells.list_off, None, probes, 10)
    assert_yardstick(ivf_c(cells.q, cells.dX, cells.doff, None, probes, 10, cells.n), want)
    assert_yardstick(ivf_op(cells.q, cells.dX, cells.doff, None, probes, 10, cells.n), want)


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, nlist, k", [(600, 8, 50), (6000, 4, 100), (6000, 4, 2048)])      # under 2048 scanned rows (sorted whole); above (radix select)
def test_ties_go_to_the_lower_original_row(n, nlist, k):
    rng = np.random.default_rng(n + k)
    d = 32
    X = rng.integers(0, 2, (n, d)).astype(np.float32)
    q = rng.integers(0, 2, (5, d)).astype(np.float32)
    q[3] = 0                                                                 # every score +0.0
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = Y.cell_order(cells, nlist)
    stored = X[row_ids]
    probes = np.stack([rng.permutation(nlist)[:nlist - 1] for _ in range(5)])
    S = Y.exact_scores(q[0], X)
    assert np.unique(S).size < 40 and np.mean(S[:, None] == S[None, :]) > 0.05        # a few dozen distinct scores: ties everywhere, across cells
    want = Y.search(q, stored, list_off, row_ids, probes, k)
    got = ivf_c(q, stored, list_off, row_ids, probes, k, n)
    assert_yardstick(got, want)
    assert_yardstick(ivf_op(q, stored, list_off, row_ids, probes, k, n), want)
    scanned = np.sort(np.flatnonzero(np.isin(cells, probes[3])))
    kk = min(k, scanned.size)
    assert np.array_equal(got[1][3].cpu().numpy()[:kk], scanned[:kk])        # the all-zero query: the lowest original rows of its cells
    assert (bits(got[0][3])[:kk] == 0).all()                                 # ... with score +0.0


# ---- 4. batch independence ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    """5000 x 256 Gaussian rows in a trained index of 64 cells, 130 queries."""
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(5000, 256, generator=g, device="cuda")
    q = torch.randn(130, 256, generator=g, device="cuda")
    idx = trained(x, 64, nprobe=8, niter=3)
    idx.add(x)
    idx.search(q[:1], 1)
    return x, q, idx


def test_a_query_does_not_depend_on_its_batch(mid):
    x, q, idx = mid
    K = 100
    whole = idx.search(q, K)
    alone = idx.search(q[77:78], K)
    first = idx.search(q[77:79], K)
    for got in (alone, first):
        assert torch.equal(got[1][0], whole[1][77]) and torch.equal(bits(got[0][0]), bits(whole[0][77]))
    # explicit probe lists: all equal (one hot set of cells) and all distinct
    equal = torch.tensor([3, 9, 27, 41, 5, 60, 0, 33], device="cuda").repeat(130, 1)
    distinct = (torch.arange(130, device="cuda")[:, None] + 7 * torch.arange(8, device="cuda")[None, :]) % 64
    for probes in (equal, distinct):
        args = (idx.stored_rows(), idx.list_off, idx.row_ids)
        whole = ivf_op(q, *args, probes, K, idx.ntotal)
        alone = ivf_op(q[77:78].contiguous(), *args, probes[77:78].contiguous(), K, idx.ntotal)
        first = ivf_op(q[77:79].contiguous(), *args, probes[77:79].contiguous(), K, idx.ntotal)
        for got in (alone, first):
            assert torch.equal(got[1][0], whole[1][77]) and torch.equal(bits(got[0][0]), bits(whole[0][77]))
        # a different scan bound (another chunking of the workspace) changes nothing either
        assert_same(ivf_op(q, *args, probes, K, idx.max_scan_rows(8)), whole)
        held = idx.list_sizes[probes.cpu().numpy()].sum(axis=1)              # every query reports min(K, the rows of its cells) rows
        assert np.array_equal((whole[1] >= 0).sum(dim=1).cpu().numpy(), np.minimum(held, K))


# ---- 5. nesting, training -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clustered():
    x, q = Y.clustered_corpus()
    idx = trained(dev(x), 64)
    return x, q, idx


def test_overlap_with_the_flat_result_never_decreases_with_nprobe(clustered):
    from lightretriever_amd import FlatIPIndex
    x, q, idx = clustered
    idx.reset()
    idx.add(dev(x))
    flat = FlatIPIndex(128)
    flat.add(dev(x))
    ref = flat.search(dev(q), 10)
    prev = np.zeros(len(q), np.int64)
    for nprobe in (1, 2, 4, 8, 16, 32, 64):
        got = idx.search(dev(q), 10, nprobe=nprobe)
        ov = Y.overlap(got[1].cpu().numpy(), ref[1].cpu().numpy())
        assert (ov >= prev).all(), (nprobe, ov, prev)                        # exact: the probe sets nest
        prev = ov
    assert (prev == 10).all()
    assert_same(got, ref)


def test_training_is_deterministic_and_matches_the_yardstick(clustered):
    x, q, idx = clustered
    first = idx.centroids.clone()
    idx.train(dev(x))
    assert torch.equal(bits(idx.centroids), bits(first))                     # two train() calls: the same bits
    idx0 = trained(dev(x), 64, niter=0)
    _, xs, init = Y.sample_and_init(x, 64)
    assert np.array_equal(idx0.centroids.cpu().numpy().view(np.int32), init.view(np.int32))
    # After 10 iterations: the index's fp64 objective against the yardstick's from the same initial centroids.  Assignment ties resolved under
    # different rounding can send the two runs apart, so this is no bit test.  The margin is the yardstick's own spread over the five seeds
    # 1234 .. 1238 on this corpus: objectives 1446405 .. 1471159 on the 16384 sampled rows, largest relative spread 1.72 % (from 2.6e6 at niter=0).
    want = Y.objective(xs, Y.lloyd(xs, init, Y.NITER, np.random.default_rng(0)))
    got = Y.objective(xs, first.cpu().numpy())
    print(f"k-means objective: index {got:.1f}, yardstick {want:.1f}, ratio {got / want:.5f}")
    assert got <= want * 1.0172
    assert got < 0.7 * Y.objective(xs, init)
    with pytest.raises(ValueError, match="nlist"):
        trained(dev(x[:63]), 64)


# ---- 6. adds ---------------------------------------------------------------------------------------------------------------------------------
def test_adds_in_pieces_equal_one_add(mid):
    from lightretriever_amd import IVFFlatIndex
    x, q, idx = mid
    want = idx.search(q, 20)
    b = IVFFlatIndex(256, 64, nprobe=8)
    with pytest.raises(RuntimeError, match="not trained"):
        b.add(x[:1])
    b.set_contents(idx.centroids, x[:0], np.zeros(65, np.int64), np.zeros(0, np.int64))
    for piece in (x[:1], x[1:128], x[128:]):
        b.add(piece)
    assert b.ntotal == 5000
    assert_same(b.search(q, 20), want)
    assert torch.equal(b.list_off, idx.list_off) and torch.equal(b.row_ids, idx.row_ids) and torch.equal(bits(b.stored_rows()), bits(idx.stored_rows()))
    assert np.array_equal(b.list_sizes, idx.list_sizes)
    off = b.list_off.cpu().numpy()
    ids = b.row_ids.cpu().numpy()
    assert all((np.diff(ids[off[c]:off[c + 1]]) > 0).all() for c in range(64))       # ascending original row inside every cell
    # add -> search -> add -> search equals a fresh index with all rows
    c = IVFFlatIndex(256, 64, nprobe=8)
    c.set_contents(idx.centroids, x[:0], np.zeros(65, np.int64), np.zeros(0, np.int64))
    c.add(x[:3000])
    part = c.search(q, 20)
    assert int((part[1] >= 3000).sum()) == 0
    c.add(x[3000:])
    assert_same(c.search(q, 20), want)
    assert torch.equal(c.row_ids, idx.row_ids)
    assert torch.equal(bits(c.reconstruct_n(0, 5000)), bits(x)) and torch.equal(bits(c.reconstruct_n(4990, 7)), bits(x[4990:4997]))
    # reset() keeps the training
    cent = c.centroids.clone()
    c.reset()
    assert c.ntotal == 0 and c.is_trained and torch.equal(bits(c.centroids), bits(cent))
    assert (c.search(q[:2], 5)[1] == -1).all()
    c.add(x)
    assert_same(c.search(q, 20), want)


def test_append_slot_and_commit_train_an_untrained_index(mid):
    from lightretriever_amd import IVFFlatIndex
    x, q, _ = mid
    a = IVFFlatIndex(256, 16, nprobe=4)
    slot = a.append_slot(2000)
    slot.copy_(x[:2000])
    a.commit(2000)
    assert a.is_trained and a.ntotal == 2000
    b = trained(x[:2000], 16, nprobe=4)
    b.add(x[:2000])
    assert torch.equal(bits(a.centroids), bits(b.centroids))
    assert_same(a.search(q, 10), b.search(q, 10))
    with pytest.raises(ValueError, match="staged"):
        a.commit(5)


# ---- 7. plumbing -----------------------------------------------------------------------------------------------------------------------------
def test_ids_persistence_and_refusals(mid, tmp_path):
    from lightretriever_amd import IVFFlatIndex, index_io
    x, q, idx = mid
    D, I = idx.search(q, 10)
    idx.id_base = 1000
    assert_same(idx.search(q, 10), (D, I + 1000))
    idx.id_base = 0
    rm = torch.arange(5000, device="cuda") * 3 + 7
    assert_same(idx.search(q, 10, row_map=rm), (D, I * 3 + 7))
    path = str(tmp_path / "i.ivf.faiss")
    idx.save(path)
    assert open(path, "rb").read() == Y.ivf_file_bytes(idx.centroids.cpu().numpy(), idx.list_sizes, idx.stored_rows().cpu().numpy(), idx.row_ids.cpu().numpy(), 8)
    st = index_io.read_ivf_flat(path)
    assert (st["d"], st["nlist"], st["nprobe"], st["ntotal"], st["is_trained"]) == (256, 64, 8, 5000, True)
    back = IVFFlatIndex.load(path, id_base=7)
    assert (back.d, back.nlist, back.nprobe, back.ntotal, back.id_base, back.is_trained) == (256, 64, 8, 5000, 7, True)
    assert_same(back.search(q, 10), (D, I + 7))
    back.add(x[:10])                                                         # a loaded index takes further rows
    assert back.ntotal == 5010 and bool((back.search(q[:1], 3)[1] >= 0).all())
    with pytest.raises(NotImplementedError, match="range_search"):
        idx.range_search(q, 0.0)
    with pytest.raises(ValueError, match="k=2049"):
        idx.search(q, 2049)
    with pytest.raises(ValueError, match="nprobe=65"):
        idx.search(q, 10, nprobe=65)
    with pytest.raises(ValueError, match="row_map"):
        idx.search(q, 10, row_map=torch.arange(10, device="cuda"))
    assert idx.search(q[:0], 10)[0].shape == (0, 10)


def test_a_captured_search_replays_the_eager_bits(mid):
    x, q, idx = mid
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


def test_searcher_equals_the_index(mid, tmp_path):
    from lightretriever_amd import IVFFlatIndex
    from lightretriever_amd.retriever import HybridSearch, IVFFaissSearch, _to_result_dict
    x, q, _ = mid
    x, q = x[:300], q[:9]
    ids = [f"doc{i}" for i in range(300)]
    qids = [f"q{i}" for i in range(9)]
    s = HybridSearch(model=None, batch_size=8, faiss_search_map="ivf", nlist=12, nprobe=5, show_progress_bar=False).dense_search
    assert isinstance(s, IVFFaissSearch)
    s.index(x, ids)
    idx = s.faiss_index.index
    assert type(idx) is IVFFlatIndex and (idx.nlist, idx.nprobe, idx.ntotal, s.dim_size) == (12, 5, 300, 256)
    direct = trained(x, 12, nprobe=5)
    direct.add(x)
    want = _to_result_dict(*direct.search(q, 20), qids, ids)
    got = s.retrieve_with_emb(q, qids, 20)
    assert got == want and all(len(v) == 20 for v in got.values())
    s.save(str(tmp_path), prefix="t")
    assert (tmp_path / "t.ivf.faiss").exists() and (tmp_path / "t.ivf.tsv").exists()
    c = IVFFaissSearch(model=None, batch_size=8, show_progress_bar=False)
    c.load(str(tmp_path), prefix="t")
    assert (c.nlist, c.nprobe, c.faiss_index.index.ntotal) == (12, 5, 300)
    assert c.retrieve_with_emb(q, qids, 20) == want
    # a chunk of fewer rows than nlist: one cell per row at the most
    t = IVFFaissSearch(model=None, nlist=1024, nprobe=32, batch_size=8, show_progress_bar=False)
    t.index(x[:40], ids[:40])
    assert (t.faiss_index.index.nlist, t.faiss_index.index.nprobe) == (40, 32)
    assert len(t.retrieve_with_emb(q, qids, 5)["q0"]) == 5
