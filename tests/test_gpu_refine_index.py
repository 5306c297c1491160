"""GPU: exact re-ranking over the lossy indexes (lrx_flat_ip_rerank / lrx_sq_fp16_ip_rerank, torch.ops.lrx.*_rerank, RefineFlatIndex,
RefineFaissSearch) against the numpy yardstick (tests/refine_yardstick.py) and against the flat / fp16-SQ searches themselves, bit for bit:
exact integer probes full of ties, the padding / duplicate / id rules, out-of-range candidates, batch independence, full recall at
k_base = ntotal, ordinary k_factor, the plumbing (slots, persistence, HIP graph) and the searchers.  Observed figures: DESIGN §5.4.9."""
import numpy as np
import pytest
import torch

import refine_yardstick as Y

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
SHAPES = [(1, 5, 32, 5, 5), (3, 300, 96, 40, 7), (4, 600, 2112, 64, 10), (130, 5000, 256, 100, 10), (5, 3000, 2048, 2048, 2048)]   # (Q, n_rows, D, n_cand, k)
CODE_SHAPES = [(1, 5, 64, 5, 5), (3, 300, 128, 40, 7)] + [s for s in SHAPES if s[2] % 64 == 0]


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


def rerank_flat(q, X, cand, k, id_base=0, row_map=None, n_rows=None):
    """lrx_flat_ip_rerank through ctypes with ldx = D + 8 (padding columns 1e30: never read into a result) and ld_cand = n_cand + 3 (padding
    entries name row 0: read, they would add hits)."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    q, X, cand = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, X, cand))
    (Q, D), n, nc = q.shape, X.shape[0], cand.shape[1]
    xb = torch.full((n, D + 8), 1e30, dtype=torch.float32, device="cuda")
    xb[:, :D] = X
    cb = torch.zeros(Q, nc + 3, dtype=torch.int64, device="cuda")
    cb[:, :nc] = cand
    Do = torch.full((Q, k), 7.5, dtype=torch.float32, device="cuda")
    Io = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(l.lrx_ip_rerank_workspace_bytes(Q, nc, k), dtype=torch.uint8, device="cuda")
    _lib.check(l.lrx_flat_ip_rerank(_lib.ptr(xb), n if n_rows is None else n_rows, D + 8, D, _lib.ptr(q.contiguous()), Q, _lib.ptr(cb), nc, nc + 3, k, id_base,
                                    _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    torch.cuda.synchronize()
    return Do, Io


def rerank_codes(q, idx, cand, k, id_base=0, row_map=None, n_rows=None):
    """lrx_sq_fp16_ip_rerank through ctypes over the codes of the SQFp16Index idx, ld_cand = n_cand + 3."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    q, cand = (t if isinstance(t, torch.Tensor) else dev(t) for t in (q, cand))
    Q, nc = cand.shape
    cb = torch.zeros(Q, nc + 3, dtype=torch.int64, device="cuda")
    cb[:, :nc] = cand
    Do = torch.full((Q, k), 7.5, dtype=torch.float32, device="cuda")
    Io = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(l.lrx_ip_rerank_workspace_bytes(Q, nc, k), dtype=torch.uint8, device="cuda")
    _lib.check(l.lrx_sq_fp16_ip_rerank(_lib.ptr(idx._xb), idx.ntotal if n_rows is None else n_rows, idx.d, _lib.ptr(q.contiguous()), Q, _lib.ptr(cb), nc, nc + 3, k,
                                       id_base, _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(row_map), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    torch.cuda.synchronize()
    return Do, Io


def codes_index(X):
    from lightretriever_amd import SQFp16Index
    idx = SQFp16Index(X.shape[1])
    idx.add(X if isinstance(X, torch.Tensor) else dev(X))
    return idx


def integer_case(Q, n, D, nc, k):
    rng = np.random.default_rng(Q + n + D)
    X = rng.integers(-3, 4, (n, D)).astype(np.float32)
    q = rng.integers(-3, 4, (Q, D)).astype(np.float32)
    cand = rng.integers(0, n, (Q, nc))
    S = q.astype(np.int64) @ X.astype(np.int64).T                            # every partial sum is an integer below 2^24: exact in any order
    assert np.abs(S).max() < 2 ** 24
    want = Y.rerank(q, X, cand, k)
    for i in (0, Q - 1):                                                     # the yardstick itself against the int64 scores
        rows = want[1][i][want[1][i] >= 0]
        assert np.array_equal(want[0][i][:rows.size], S[i, rows].astype(np.float32))
    return q, X, cand, want


_CASES = {}


def case(shape):
    if shape not in _CASES:
        _CASES[shape] = integer_case(*shape)
    return _CASES[shape]


# ---- 1. integer probe: exact, full of ties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_probe_is_exact_over_fp32_rows(shape):
    """Integers in [-3, 3]: the scores are exact whatever the order of summation, so ids AND scores must be the int64 yardstick's bit for bit;
    scores collide all the time (a few hundred distinct values) and random candidates repeat, so the tie order and the duplicates are in it."""
    q, X, cand, want = case(shape)
    assert_yardstick(rerank_flat(q, X, cand, shape[4]), want)


@pytest.mark.parametrize("shape", CODE_SHAPES)
def test_integer_probe_is_exact_over_fp16_codes(shape):
    q, X, cand, want = case(shape)                                           # (small integers are fp16 numbers: the codes are the rows)
    assert_yardstick(rerank_codes(q, codes_index(X), cand, shape[4]), want)


# ---- 2. the same bits as the searches -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss():
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(20000, 128, generator=g, device="cuda")
    x[7001] = x[12]                                                          # a twin: equal scores
    return x, torch.randn(9, 128, generator=g, device="cuda")


def shuffled(I, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.stack([row[torch.randperm(row.numel(), generator=g, device="cuda")] for row in I])


@pytest.mark.parametrize("n", [3000, 20000])                                 # the plain path of a tiny shard, the two-pass chain
def test_rerank_of_a_search_result_returns_that_search(gauss, n):
    from lightretriever_amd import FlatIPIndex
    x, q = gauss
    idx = FlatIPIndex(128)
    idx.add(x[:n])
    D, I = idx.search(q, 64)
    assert_same(rerank_flat(q, x[:n], shuffled(I), 64), (D, I))
    sq = codes_index(x[:n])
    D, I = sq.search(q, 64)
    assert_same(rerank_codes(q, sq, shuffled(I, 1), 64), (D, I))


# ---- 3. padding and id rules --------------------------------------------------------------------------------------------------------
def test_padding_duplicates_and_ids():
    q, X, cand, _ = case(CODE_SHAPES[1])                                     # Q = 3, 300 rows of 128, 40 candidates
    cand = cand.copy()
    cand[0, ::2] = -1                                                        # padding between the candidates
    cand[1] = -1                                                             # nothing at all
    cand[2, 5:] = -1                                                         # fewer valid candidates than k
    cand[2, :5] = [17, 4, 17, 250, 4]                                        # duplicates
    sq = codes_index(X)
    for k in (7, 40):
        want = Y.rerank(q, X, cand, k)
        assert (want[1][1] == -1).all() and (want[0][1] == -FLT_MAX).all() and (want[1][2, 5:] == -1).all() and (want[1][0] >= 0).sum() == min(k, 20)
        assert sorted(want[1][2, :5].tolist()) == [4, 4, 17, 17, 250]
        assert_yardstick(rerank_flat(q, X, cand, k), want)
        assert_yardstick(rerank_codes(q, sq, cand, k), want)
    row_map = dev(np.arange(300)[::-1] * 5 + 3)
    for run in (lambda **kw: rerank_flat(q, X, cand, 7, **kw), lambda **kw: rerank_codes(q, sq, cand, 7, **kw)):
        assert_yardstick(run(id_base=1000), Y.rerank(q, X, cand, 7, id_base=1000))
        assert_yardstick(run(id_base=1000, row_map=row_map), Y.rerank(q, X, cand, 7, row_map=row_map.cpu().numpy()))   # (row_map wins over id_base)


# ---- 4. out-of-range candidates are not read ----------------------------------------------------------------------------------------
def test_out_of_range_candidates_are_skipped_and_counted():
    """n_rows = 100 of a 200-row tensor whose rows 100..199 hold 1e30: a candidate in 100..199 lies inside the allocation whatever the
    kernel does, but must be absent from the result and counted once in the device error counter."""
    from lightretriever_amd import _lib
    l = _lib.lib()
    rng = np.random.default_rng(4)
    X = rng.integers(-3, 4, (200, 64)).astype(np.float32)
    X[100:] = 1e30
    q = np.abs(rng.integers(-3, 4, (6, 64))).astype(np.float32) + 1          # positive queries: a row of 1e30 would win
    cand = rng.integers(0, 100, (6, 30))
    cand[:, 3::4] = rng.integers(100, 200, cand[:, 3::4].shape)
    cand[4] = rng.integers(100, 200, 30)                                     # a query with nothing valid
    n_bad = int((cand >= 100).sum())
    want = Y.rerank(q, X, cand, 10, n_rows=100)
    assert (want[1][4] == -1).all() and (want[1] < 100).all()
    sq = codes_index(np.where(X > 1e29, 60000.0, X).astype(np.float32))
    for run in (lambda: rerank_flat(q, X, cand, 10, n_rows=100), lambda: rerank_codes(q, sq, cand, 10, n_rows=100)):
        assert l.lrx_device_error_count(1) >= 0 and l.lrx_device_error_count(1) == 0
        got = run()
        assert l.lrx_device_error_count(1) == n_bad and l.lrx_device_error_count(1) == 0
        assert_yardstick(got, want)


# ---- 5. batch independence, the torch ops ---------------------------------------------------------------------------------------------
def test_a_query_alone_gives_the_same_bits_and_the_ops_equal_ctypes():
    from lightretriever_amd import torch_ops  # noqa: F401
    shape = SHAPES[3]                                                        # Q = 130: the split over workgroups differs from a single query's
    q, X, cand, want = case(shape)
    g = torch.Generator(device="cuda").manual_seed(1)
    qg, Xg = torch.randn(130, 256, generator=g, device="cuda"), torch.randn(5000, 256, generator=g, device="cuda")
    full = rerank_flat(qg, Xg, cand, 10)
    sq = codes_index(Xg)
    full16 = rerank_codes(qg, sq, cand, 10)
    for i in (0, 64, 129):
        assert_yardstick(rerank_flat(q[i:i + 1], X, cand[i:i + 1], 10), (want[0][i:i + 1], want[1][i:i + 1]))
        assert_same(rerank_flat(qg[i:i + 1], Xg, cand[i:i + 1], 10), (full[0][i:i + 1], full[1][i:i + 1]))
        assert_same(rerank_codes(qg[i:i + 1], sq, cand[i:i + 1], 10), (full16[0][i:i + 1], full16[1][i:i + 1]))
    c = dev(cand)
    row_map = torch.arange(5000, device="cuda").flip(0).contiguous()
    assert_same(torch.ops.lrx.flat_ip_rerank(qg, Xg, c, 10), full)
    assert_same(torch.ops.lrx.sq_fp16_ip_rerank(qg, sq._xb, 5000, c, 10), full16)
    wide = torch.zeros(130, 107, dtype=torch.int64, device="cuda")           # strided candidates and rows
    wide[:, :100] = c
    xw = torch.full((5000, 264), 1e30, device="cuda")
    xw[:, :256] = Xg
    D, I = torch.ops.lrx.flat_ip_rerank(qg, xw[:, :256], wide[:, :100], 10, 50, row_map)
    assert torch.equal(bits(D), bits(full[0])) and torch.equal(I, row_map[full[1]])
    D, I = torch.ops.lrx.sq_fp16_ip_rerank(qg, sq._xb, 5000, wide[:, :100], 10, 50)
    assert torch.equal(bits(D), bits(full16[0])) and torch.equal(I, full16[1] + 50)
    for bad in (lambda: torch.ops.lrx.flat_ip_rerank(qg, Xg, c, 101), lambda: torch.ops.lrx.flat_ip_rerank(qg, Xg, c, 0),
                lambda: torch.ops.lrx.flat_ip_rerank(qg[:5], Xg, c, 10), lambda: torch.ops.lrx.flat_ip_rerank(qg, Xg[:, :128], c, 10),
                lambda: torch.ops.lrx.flat_ip_rerank(qg, Xg, c.int(), 10), lambda: torch.ops.lrx.sq_fp16_ip_rerank(qg, sq._xb[:100], 5000, c, 10),
                lambda: torch.ops.lrx.flat_ip_rerank(qg, Xg, c, 10, 0, row_map[:10]), lambda: torch.ops.lrx.flat_ip_rerank(qg.cpu(), Xg, c, 10)):
        with pytest.raises(RuntimeError):
            bad()


# ---- 6. / 7. RefineFlatIndex over every base ------------------------------------------------------------------------------------------
N, DIM, K = 600, 128, 20
BASE_KINDS = ["pq", "sq8", "sq8_uniform", "pca_flat", "pca_pq"]


def make_base(kind):
    from lightretriever_amd import FlatIPIndex, PCAMatrix, PQIndex, PreTransformIndex, SQ8Index
    return {"pq": lambda: PQIndex(DIM, 16), "sq8": lambda: SQ8Index(DIM, "QT_8bit"), "sq8_uniform": lambda: SQ8Index(DIM, "QT_8bit_uniform"),
            "pca_flat": lambda: PreTransformIndex(PCAMatrix(DIM, 32), FlatIPIndex(32)),
            "pca_pq": lambda: PreTransformIndex(PCAMatrix(DIM, 32), PQIndex(32, 8))}[kind]()


@pytest.fixture(scope="module")
def rows():
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(N, DIM, generator=g, device="cuda")
    x[N - 10:] = x[:10]                                                      # ten duplicated rows: equal scores, the lower row first
    q = torch.randn(17, DIM, generator=g, device="cuda")
    q[3] = x[4]
    return x, q


@pytest.fixture(scope="module")
def flat_ref(rows):
    from lightretriever_amd import FlatIPIndex
    x, q = rows
    idx = FlatIPIndex(DIM)
    idx.add(x)
    D, I = idx.search(q, K)
    return D.clone(), I.clone()


def refine_over(kind, x, store=None, **kw):
    from lightretriever_amd import RefineFlatIndex
    idx = RefineFlatIndex(make_base(kind), store, **kw)
    assert not idx.is_trained and idx.ntotal == 0 and idx.d == DIM
    with pytest.raises(RuntimeError, match="not trained"):
        idx.add(x)
    idx.train(x)
    assert idx.is_trained
    idx.add(x[:250])
    idx.add(x[250:].cpu().numpy())
    assert idx.ntotal == idx.base_index.ntotal == idx.refine_index.ntotal == N
    return idx


@pytest.mark.parametrize("kind", BASE_KINDS)
def test_full_recall_returns_the_flat_search(kind, rows, flat_ref):
    """k_factor = 30: k_base = 600 = ntotal, every row is a candidate, so the result is FlatIPIndex.search's bit for bit -- whatever the base
    makes of the rows -- and SQFp16Index.search's with an fp16 store."""
    from lightretriever_amd import FlatIPIndex, SQFp16Index
    x, q = rows
    idx = refine_over(kind, x, k_factor=30)
    assert type(idx.refine_index) is FlatIPIndex and idx.refine_index.shadow_f16 is False and idx.refine_index._xb is None   # 4 B/element
    assert_same(idx.search(q, K), flat_ref)
    assert_same(idx.search(q.cpu().numpy(), K, k_factor=30.0), flat_ref)
    sq = SQFp16Index(DIM)
    sq.add(x)
    idx16 = refine_over(kind, x, SQFp16Index(DIM), k_factor=30)
    assert_same(idx16.search(q, K), sq.search(q, K))


@pytest.mark.parametrize("kind", BASE_KINDS)
def test_ordinary_k_factor_equals_the_yardstick(kind, rows, flat_ref):
    x, q = rows
    idx = refine_over(kind, x)
    xn, qn, ref = x.cpu().numpy(), q.cpu().numpy(), flat_ref[1].cpu().numpy()
    base_recall = Y.recall(idx.base_index.search(q, K)[1].cpu().numpy(), ref)
    last = 0.0
    for kf in (1, 2, 4):
        kb = Y.k_base(K, kf)
        cand = idx.base_index.search(q, kb)[1]
        assert cand.shape == (17, kb)
        got = idx.search(q, K, k_factor=kf)
        assert_yardstick(got, Y.rerank(qn, xn, cand.cpu().numpy(), K))
        r = Y.recall(got[1].cpu().numpy(), ref)
        print(f"{kind}: k_factor {kf}: recall@{K} {r:.3f} (base alone {base_recall:.3f})")
        assert r >= base_recall and r >= last                                 # by construction: the candidates hold the base's own top k
        last = r
    idx.k_factor = 4.0
    assert_same(idx.search(q, K), got)                                        # the index's own k_factor is the default


# ---- 8. plumbing ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,store", [("pq", "flat"), ("pca_pq", "flat"), ("sq8", "fp16")])
def test_slot_commit_equals_add_and_trains_an_untrained_base(kind, store, rows):
    from lightretriever_amd import RefineFlatIndex, SQFp16Index
    x, q = rows
    want_idx = refine_over(kind, x, SQFp16Index(DIM) if store == "fp16" else None, k_factor=2)
    want = want_idx.search(q, K)
    idx = RefineFlatIndex(make_base(kind), SQFp16Index(DIM) if store == "fp16" else None, k_factor=2)
    slot = idx.append_slot(N)
    assert slot.shape == (N, DIM) and slot.dtype == torch.float32
    if store == "flat":
        assert slot.data_ptr() == idx.refine_index._x.data_ptr()             # the encoder writes the final fp32 rows
    slot.copy_(x)
    idx.commit(N)                                                            # trains the base on the slot, adds, commits the store
    assert idx.is_trained and idx.ntotal == idx.base_index.ntotal == N
    assert_same(idx.search(q, K), want)
    with pytest.raises(ValueError, match="slot rows"):
        idx.commit(3)
    # reconstruct_n reads the store; reset drops the rows of both and keeps the training
    rec = idx.reconstruct_n(5, 40)
    assert torch.equal(bits(rec), bits(x[5:45] if store == "flat" else x[5:45].half().float()))
    with pytest.raises(ValueError):
        idx.reconstruct_n(N - 5, 10)
    idx.reset()
    assert idx.ntotal == idx.base_index.ntotal == idx.refine_index.ntotal == 0 and idx.is_trained
    D, I = idx.search(q, K)
    assert (I == -1).all() and (D == -FLT_MAX).all()
    idx.append_slot(250).copy_(x[:250])                                      # a second slot continues the first
    idx.commit(250)
    idx.append_slot(N - 250).copy_(x[250:])
    idx.commit(N - 250)
    assert_same(idx.search(q, K), want)
    idx.id_base = 1000
    row_map = torch.arange(N, device="cuda").flip(0).contiguous()
    assert idx.base_index.id_base == 0 and torch.equal(idx.search(q, K)[1], want[1] + 1000)
    assert torch.equal(idx.search(q, K, row_map=row_map)[1], row_map[want[1]])


@pytest.mark.parametrize("kind,store", [("pq", "flat"), ("sq8_uniform", "fp16"), ("pca_flat", "flat"), ("pca_pq", "fp16")])
def test_save_load_round_trip(kind, store, rows, tmp_path):
    from lightretriever_amd import FlatIPIndex, RefineFlatIndex, SQFp16Index, index_io
    x, q = rows
    idx = refine_over(kind, x, SQFp16Index(DIM) if store == "fp16" else None, k_factor=2.5)
    want = idx.search(q, K)
    path = str(tmp_path / "r.refine.faiss")
    idx.save(path)
    st = index_io.read_refine(path)
    assert (st["d"], st["ntotal"], st["is_trained"], st["k_factor"]) == (DIM, N, True, 2.5)
    back = RefineFlatIndex.load(path, id_base=7)
    assert type(back.base_index) is type(idx.base_index) and type(back.refine_index) is (SQFp16Index if store == "fp16" else FlatIPIndex)
    assert back.k_factor == 2.5 and back.ntotal == N and back.id_base == 7 and back.base_index.id_base == 0 and back.is_trained
    if store == "flat":
        assert back.refine_index.shadow_f16 is False and back.refine_index._xb is None
    D, I = back.search(q, K)
    assert torch.equal(bits(D), bits(want[0])) and torch.equal(I, want[1] + 7)
    assert torch.equal(bits(back.reconstruct_n(0, N)), bits(idx.reconstruct_n(0, N)))


def test_refusals_and_graph_capture(rows):
    from lightretriever_amd import PQIndex, RefineFlatIndex, _lib, refine
    x, q = rows
    idx = refine_over("sq8_uniform", x, k_factor=2)
    with pytest.raises(ValueError, match="2048"):
        idx.search(q, 1025)
    with pytest.raises(ValueError, match="2048"):
        idx.search(q, 100, k_factor=20.5)
    with pytest.raises(ValueError, match="k_factor"):
        idx.search(q, 10, k_factor=0.9)
    with pytest.raises(ValueError, match="k_factor"):
        RefineFlatIndex(PQIndex(DIM, 16), k_factor=0.5)
    with pytest.raises(ValueError, match="id_base=3"):
        RefineFlatIndex(PQIndex(DIM, 16, id_base=3))
    idx.base_index.id_base = 3
    with pytest.raises(ValueError, match="id_base=3"):
        idx.search(q, 10)
    idx.base_index.id_base = 0
    with pytest.raises(NotImplementedError):
        idx.range_search(q, 0.0)
    with pytest.raises(ValueError, match="row_map"):
        idx.search(q, 10, row_map=torch.arange(10, device="cuda"))
    with pytest.raises(TypeError):
        RefineFlatIndex(idx.refine_index)
    assert idx.search(q[:0], 10)[0].shape == (0, 10)
    # the rerank captured in a HIP graph and replayed with new queries gives the eager bits
    store, slots = idx.refine_index, {}
    qbuf = q.clone()
    cand = idx.base_index.search(q, 2 * K)[1].clone()
    cold = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.LrxError, match="workspace must exist"):
        with torch.cuda.graph(cold):                                         # the first rerank of this shape under capture: refused, nothing launched
            refine.rerank(qbuf, store, cand, K, ws_slots=slots)
    del cold
    eager = tuple(t.clone() for t in refine.rerank(qbuf, store, cand, K, ws_slots=slots))
    assert_same(eager, idx.search(q, K))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        refine.rerank(qbuf, store, cand, K, ws_slots=slots)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Dg, Ig = refine.rerank(qbuf, store, cand, K, ws_slots=slots)
    graph.replay()
    torch.cuda.synchronize()
    assert_same((Dg, Ig), eager)
    q2 = q.flip(0).contiguous()
    want = tuple(t.clone() for t in refine.rerank(q2, store, cand, K))
    qbuf.copy_(q2)
    graph.replay()
    torch.cuda.synchronize()
    assert_same((Dg, Ig), want)


# ---- 9. the searchers -----------------------------------------------------------------------------------------------------------------
class TableModel:
    """encode_corpus / encode_queries by lookup: the embeddings are the test's own."""

    def __init__(self, table):
        self.table = table

    def _rows(self, texts):
        return torch.stack([self.table[t["text"] if isinstance(t, dict) else t] for t in texts]).cuda()

    def encode_queries(self, queries, **kw):
        return {"dense_reps": self._rows(queries)}

    def encode_corpus(self, corpus, **kw):
        return {"dense_reps": self._rows(corpus)}


SEARCHERS = [("pq", dict(num_of_centroids=16), "pq"), ("sq", dict(quantizer_type="QT_8bit_uniform"), "sq8_uniform"), ("pca", dict(output_dimension=32), "pca_flat")]


@pytest.mark.parametrize("refine_base,kwargs,kind", SEARCHERS)
@pytest.mark.parametrize("refine_type", ["flat", "fp16"])
def test_searcher_equals_the_index(refine_base, kwargs, kind, refine_type, rows, tmp_path):
    from lightretriever_amd import FlatIPIndex, RefineFlatIndex, SQFp16Index
    from lightretriever_amd.retriever import HybridSearch, RefineFaissSearch, _to_result_dict
    x, q = rows
    ids = [f"doc{i}" for i in range(N)]
    qids = [f"q{i}" for i in range(q.shape[0])]
    s = HybridSearch(model=None, batch_size=8, faiss_search_map="refine", refine_base=refine_base, k_factor=3, refine_type=refine_type,
                     show_progress_bar=False, **kwargs).dense_search
    assert isinstance(s, RefineFaissSearch)
    s.index(x, ids)
    idx = s.faiss_index.index
    assert type(idx) is RefineFlatIndex and type(idx.base_index) is type(make_base(kind)) and idx.k_factor == 3.0 and idx.ntotal == N and s.dim_size == DIM
    assert type(idx.refine_index) is (SQFp16Index if refine_type == "fp16" else FlatIPIndex)
    direct = refine_over(kind, x, SQFp16Index(DIM) if refine_type == "fp16" else None, k_factor=3)
    want = _to_result_dict(*direct.search(q, K), qids, ids)
    got = s.retrieve_with_emb(q, qids, K)
    assert got == want and all(len(v) == K for v in got.values())
    with pytest.raises(ValueError, match="2048"):
        s.retrieve_with_emb(q, qids, 700)
    # save -> load: the same hits, k_factor and the shard classes come from the file
    s.save(str(tmp_path), prefix="t")
    assert (tmp_path / "t.refine.faiss").exists() and (tmp_path / "t.refine.tsv").exists()
    c = RefineFaissSearch(model=None, refine_base=refine_base, batch_size=8, show_progress_bar=False, **kwargs)
    c.load(str(tmp_path), prefix="t")
    assert c.k_factor == 3.0 and c.refine_type == refine_type and c.faiss_index.index.ntotal == N
    assert c.retrieve_with_emb(q, qids, K) == want
    if refine_base == "pca":                                                 # the next chunk reuses the first chunk's matrix
        first = s.base_search.pca_matrix
        s._clear()
        s.index(x[:300], ids[:300])
        assert torch.equal(bits(s.faiss_index.index.base_index.transform.A), bits(first.A)) and s.faiss_index.index.ntotal == 300


def test_search_with_a_stand_in_model_end_to_end(rows):
    from lightretriever_amd import SQFp16Index
    from lightretriever_amd.retriever import HybridSearch, RefineFaissSearch, _to_result_dict
    x, q = rows
    x, q = x.cpu(), q[:5].cpu()
    ids = [f"d{i:03d}" for i in range(N)]
    corpus = {pid: {"text": "x" * (N - j) + pid} for j, pid in enumerate(ids)}   # longest first = this order
    qs = {f"q{i}": f"query {i}" for i in range(5)}
    table = {corpus[pid]["text"]: x[j] for j, pid in enumerate(ids)}
    table.update({t: q[i] for i, t in enumerate(qs.values())})
    model = TableModel(table)
    for refine_type in ("flat", "fp16"):
        direct = refine_over("pq", x.cuda(), SQFp16Index(DIM) if refine_type == "fp16" else None, k_factor=4)
        want = _to_result_dict(*direct.search(q.cuda(), K), list(qs), ids)
        s = RefineFaissSearch(model, refine_base="pq", k_factor=4, refine_type=refine_type, num_of_centroids=16, batch_size=64, show_progress_bar=False)
        assert s.search(corpus, qs, top_k=K) == want                          # one chunk: encoded into the slot, the base trained at commit
        h = HybridSearch(model, batch_size=64, faiss_search_map="refine", refine_base="pq", k_factor=4, refine_type=refine_type, num_of_centroids=16,
                         show_progress_bar=False)
        assert h.search(corpus, qs, top_k=K) == want
    with pytest.raises(ValueError, match="2048"):
        s.search(corpus, qs, top_k=600)
