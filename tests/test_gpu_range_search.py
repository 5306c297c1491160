"""GPU: exact inner-product range search (FlatIPIndex.range_search, lrx_flat_ip_range_search, torch.ops.lrx.flat_ip_range_search) against an
fp64 evaluation of every product on the GPU, rounded once: lims, ids and the bits of the scores must be identical."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def range_fp64_gpu(q, X, radius, id_base=0, chunk=32768):
    """(lims, D, I): rows with (float)(fp64 q . x) > radius, ascending row order per query."""
    Q = q.shape[0]
    qd = q.double()
    qi_l, row_l, sc_l = [], [], []
    for s in range(0, X.shape[0], chunk):
        e = min(s + chunk, X.shape[0])
        sc = (qd @ X[s:e].double().T).float()
        qi, r = torch.nonzero(sc > radius, as_tuple=True)
        qi_l.append(qi)
        row_l.append(r + s)
        sc_l.append(sc[qi, r])
    qi, rows, scores = torch.cat(qi_l), torch.cat(row_l), torch.cat(sc_l)
    order = torch.sort(qi, stable=True).indices            # chunks are in row order: a stable sort by query keeps rows ascending
    qi, rows, scores = qi[order], rows[order], scores[order]
    lims = torch.zeros(Q + 1, dtype=torch.int64, device=q.device)
    lims[1:] = torch.cumsum(torch.bincount(qi, minlength=Q), 0)
    return lims, scores, rows + id_base


def assert_same(got, ref):
    lims, D, I = got
    rl, rD, rI = ref
    assert torch.equal(lims.cpu(), rl.cpu()), (lims[:8].tolist(), rl[:8].tolist())
    assert torch.equal(I.cpu(), rI.cpu())
    assert torch.equal(D.view(torch.int32).cpu(), rD.view(torch.int32).cpu())


def make_index(X, id_base=0, **attrs):
    from lightretriever_amd import FlatIPIndex
    idx = FlatIPIndex(X.shape[1], capacity=X.shape[0], id_base=id_base)
    for k, v in attrs.items():
        setattr(idx, k, v)
    slot = idx.append_slot(X.shape[0])
    slot.copy_(X)
    idx.commit(X.shape[0])
    return idx


def unit_rows(n, d, seed, chunk=131072):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty(n, d, device="cuda")
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        X[s:e] = torch.nn.functional.normalize(torch.randn(e - s, d, generator=g, device="cuda"), dim=-1)
    return X


def queries_of(X, Q, seed):
    """Half corpus rows (a self-hit at ~1 plus neighbours), half random unit vectors."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = torch.randint(0, X.shape[0], (Q,), generator=g, device="cuda")
    rnd = torch.nn.functional.normalize(torch.randn(Q, X.shape[1], generator=g, device="cuda"), dim=-1)
    q = torch.where((torch.arange(Q, device="cuda") % 2 == 0)[:, None], X[rows] + 0.01 * rnd, rnd)
    return torch.nn.functional.normalize(q, dim=-1).contiguous()


@pytest.fixture(scope="module")
def corpus_1m():
    X = unit_rows(1_000_000, 2048, seed=11)
    idx = make_index(X)
    yield X, idx
    del idx, X
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", ["200k_x_1024", "1m_x_2048"])
def test_random_unit_rows_exact(shape, corpus_1m):
    if shape == "1m_x_2048":
        X, idx = corpus_1m
    else:
        X = unit_rows(200_000, 1024, seed=5)
        idx = make_index(X)
    N, D = X.shape
    q = queries_of(X, 300, seed=7)
    sigma = D ** -0.5
    # radii: ~0 hits for random queries (4.5 sigma), ~1e-3 N, ~5e-3 N hits; 200 k rows also ~15 % (~30 k rows: past any LDS-resident sort)
    radii = [4.5 * sigma, 3.1 * sigma, 2.58 * sigma] + ([1.04 * sigma] if N <= 200_000 else [])
    for radius in radii:
        ref = range_fp64_gpu(q, X, radius)
        for Q in (1, 37, 256, 300):
            got = idx.range_search(q[:Q], radius)
            rl = ref[0][:Q + 1]
            assert_same(got, (rl, ref[1][:int(rl[-1])], ref[2][:int(rl[-1])]))
        per_q = (ref[0][1:] - ref[0][:-1]).cpu()
        assert int(per_q.max()) <= 70_000
    if N <= 200_000:
        assert int(per_q.max()) > 20_000                  # the last radius: every query well past one LDS sort


def test_strict_boundary_on_an_exact_grid():
    """Entries k / 16 with |k| <= 3: every product and sum is exact in fp16, fp32 and fp64 -- many rows attain the same score exactly."""
    g = torch.Generator(device="cuda").manual_seed(3)
    N, D = 60_000, 128
    X = torch.randint(-3, 4, (N, D), generator=g, device="cuda").float() / 16
    q = (torch.randint(-3, 4, (8, D), generator=g, device="cuda").float() / 16).contiguous()
    idx = make_index(X)
    exact = (q.double() @ X.double().T)
    radius = float(exact[0].median())
    assert (exact[0] == radius).sum() >= 100
    got = idx.range_search(q, radius)
    assert_same(got, range_fp64_gpu(q, X, radius))
    lims, Dv, I = got
    mine = I[int(lims[0]):int(lims[1])]
    at = torch.nonzero(exact[0] == radius).flatten()
    nxt = torch.nonzero(exact[0] == radius + 1 / 256).flatten()      # the next attained score of the grid
    assert len(nxt) > 0
    assert not torch.isin(at, mine).any() and torch.isin(nxt, mine).all()


def test_overflowing_lists_take_the_score_matrix_path_and_stay_complete():
    from lightretriever_amd import _lib
    from lightretriever_amd.synth import clustered_corpus
    N, D = 300_000, 1024
    from lightretriever_amd import FlatIPIndex
    idx = FlatIPIndex(D, capacity=N)
    slot = idx.append_slot(N)
    info = clustered_corpus(slot, n_clusters=4, intra_cos=0.9, dup_frac=0.01, seed=2)
    idx.commit(N)
    X = idx.vectors
    members = torch.stack([torch.nonzero(info["assign"] == c).flatten()[0] for c in range(4)])
    rnd = torch.nn.functional.normalize(torch.randn(4, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)), dim=-1)
    q = torch.cat([info["centres"], X[members], rnd]).contiguous()
    radius = 0.8
    lib = _lib.lib()
    lib.lrx_search_fallback_count(1)
    got = idx.range_search(q, radius)
    fb = int(lib.lrx_search_fallback_count(1))
    ref = range_fp64_gpu(q, X, radius)
    assert_same(got, ref)
    hits = (ref[0][1:] - ref[0][:-1]).cpu()
    big = int((hits > 65536).sum())
    assert big >= 4 and int(hits.max()) > 65536           # more than one candidate list holds -- and far past any LDS-resident sort
    calls = 2 if int(ref[0][-1]) > q.shape[0] * 1024 else 1       # (range_search calls the library again when its first guess was short)
    assert fb % calls == 0 and big <= fb // calls <= q.shape[0]


def test_overflow_in_the_second_query_group_of_a_chunk():
    """200 queries = two 128-query groups of one chunk; the second has 72 queries, so its gated score matrix is the six-product kernel.
    Overflowing queries only in the second group (its gate alone raised), then in both (the first group's matrix is scored again for the
    fill pass)."""
    from lightretriever_amd import FlatIPIndex, _lib
    from lightretriever_amd.synth import clustered_corpus
    N, D = 300_000, 1024
    idx = FlatIPIndex(D, capacity=N)
    slot = idx.append_slot(N)
    info = clustered_corpus(slot, n_clusters=4, intra_cos=0.9, dup_frac=0.01, seed=3)
    idx.commit(N)
    X = idx.vectors
    base = torch.nn.functional.normalize(torch.randn(200, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)), dim=-1)
    qa = base.clone()
    qa[150:154] = info["centres"]
    qb = base.clone()
    qb[5] = info["centres"][0]
    qb[170] = info["centres"][1]
    lib = _lib.lib()
    for q, flagged in ((qa.contiguous(), [150, 151, 152, 153]), (qb.contiguous(), [5, 170])):
        radius = 0.8
        lib.lrx_search_fallback_count(1)
        got = idx.range_search(q, radius)
        fb = int(lib.lrx_search_fallback_count(1))
        ref = range_fp64_gpu(q, X, radius)
        assert_same(got, ref)
        hits = (ref[0][1:] - ref[0][:-1]).cpu()
        assert torch.nonzero(hits > 65536).flatten().tolist() == flagged
        calls = 2 if int(ref[0][-1]) > q.shape[0] * 1024 else 1
        assert fb % calls == 0 and len(flagged) <= fb // calls <= q.shape[0]


def _states_check(X, q, radius):
    ref = range_fp64_gpu(q, X, radius)
    outs = []
    for attrs in ({}, {"shadow_f16": False}, {"two_pass": False}):
        outs.append(make_index(X, **attrs).range_search(q, radius))
    for o in outs:
        assert_same(o, ref)
    # id_base shifts the ids only
    o = make_index(X, id_base=1000).range_search(q, radius)
    assert_same(o, (ref[0], ref[1], ref[2] + 1000))
    return ref


def test_index_states_shadow_two_pass_width_and_tiny_shard():
    X = unit_rows(60_000, 128, seed=21)
    q = queries_of(X, 40, seed=22)
    _states_check(X, q, 2.3 * 128 ** -0.5)
    X96 = unit_rows(60_000, 96, seed=23)                  # d % 64 != 0: no shadow, score-matrix path
    _states_check(X96, queries_of(X96, 40, seed=24), 2.3 * 96 ** -0.5)
    Xs = X[:4096].contiguous()                            # <= REF_CAND rows: score-matrix path even with a shadow
    _states_check(Xs, q, 1.5 * 128 ** -0.5)


def test_consistency_with_topk(corpus_1m):
    X, idx = corpus_1m
    q = queries_of(X, 100, seed=31)
    Ds, Is = idx.search(q, 100)
    for i in range(100):
        kth = Ds[i, 99:100]
        r = float(torch.nextafter(kth, torch.tensor([-float("inf")], device="cuda")).item())
        lims, Dr, Ir = idx.range_search(q[i:i + 1], r)
        assert int(lims[1]) >= 100
        assert torch.isin(Is[i], Ir).all()
        pos = torch.searchsorted(Ir, Is[i].sort().values)
        sc = dict(zip(Is[i].tolist(), Ds[i].view(torch.int32).tolist()))
        assert Dr.view(torch.int32)[pos].tolist() == [sc[j] for j in Is[i].sort().values.tolist()]
        assert bool((Dr >= kth).all())


def test_edge_cases_and_capacity_contract():
    from lightretriever_amd import FlatIPIndex, _lib
    lib = _lib.lib()
    errs0 = int(lib.lrx_device_error_count(0))
    empty = FlatIPIndex(128)
    lims, Dv, I = empty.range_search(torch.randn(3, 128, device="cuda"), 0.0)
    assert lims.tolist() == [0, 0, 0, 0] and Dv.numel() == 0 and I.numel() == 0
    X = unit_rows(50_000, 128, seed=41)
    idx = make_index(X)
    lims, Dv, I = idx.range_search(torch.empty(0, 128, device="cuda"), 0.0)
    assert lims.tolist() == [0]
    q = queries_of(X, 3, seed=42)
    lims, Dv, I = idx.range_search(q, 10.0)
    assert lims.tolist() == [0, 0, 0, 0]
    for radius in (-10.0, -float("inf")):
        got = idx.range_search(q, radius)
        assert int(got[0][-1]) == 3 * 50_000
        assert_same(got, range_fp64_gpu(q, X, radius))
    # C level: one short of the result leaves sentinel outputs untouched, returns OK and still gives the exact lims
    radius = 2.0 * 128 ** -0.5
    ref = range_fp64_gpu(q, X, radius)
    n = int(ref[0][-1])
    assert n > 1
    ws = torch.empty(int(lib.lrx_flat_ip_range_workspace_bytes(50_000, 128, 3, 1)), dtype=torch.uint8, device="cuda")

    def call(cap, Do, Io, lims):
        return lib.lrx_flat_ip_range_search(_lib.ptr(idx._x), 50_000, idx._x.stride(0), 128, _lib.ptr(idx._xb), _lib.ptr(idx._bounds), _lib.ptr(q), 3,
                                            radius, 0, _lib.ptr(lims), _lib.ptr(Do), _lib.ptr(Io), cap, _lib.ptr(ws), ws.numel(), _lib.current_stream())
    Do = torch.full((n,), 12345.0, device="cuda")
    Io = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    lims = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    assert call(n - 1, Do, Io, lims) == 0
    assert torch.equal(lims.cpu(), ref[0].cpu())
    assert bool((Do == 12345.0).all()) and bool((Io == -7).all())
    assert call(n, Do, Io, lims) == 0
    assert_same((lims, Do, Io), ref)
    torch.cuda.synchronize()
    assert int(lib.lrx_device_error_count(0)) == errs0


def test_faiss_index_and_torch_op():
    from lightretriever_amd import torch_ops
    from lightretriever_amd.retriever import FaissIndex
    lrx = torch_ops.load()
    X = unit_rows(60_000, 256, seed=51)
    idx = make_index(X)
    q = queries_of(X, 20, seed=52)
    radius = 2.2 * 256 ** -0.5
    want = idx.range_search(q, radius)
    pids = np.arange(60_000, dtype=np.int64) * 3 + 17
    fi = FaissIndex(idx, list(pids))
    lims, Dv, I = fi.range_search(q, radius)
    assert torch.equal(lims, want[0]) and torch.equal(Dv, want[1]) and torch.equal(I.cpu(), torch.from_numpy(pids)[want[2].cpu()])
    got = lrx.flat_ip_range_search(q, idx.vectors, idx._xb, idx._bounds, radius, 0)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    got = lrx.flat_ip_range_search(q, idx.vectors, None, idx._bounds, radius, 5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2] + 5)
