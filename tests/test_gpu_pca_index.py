"""GPU: the PCA pre-transform index (lrx_linear_transform, torch.ops.lrx.linear_transform, PCAMatrix, PreTransformIndex, PCAFaissSearch) --
the kernel against exact integer probes and a derived fp32 error bound, its determinism and batch independence, the training against the
numpy fp64 yardstick (tests/pca_yardstick.py) under bounds that follow from the fp32 arithmetic, and the composition with every base index
bit for bit against the base fed the transformed rows.  Observed figures: DESIGN §5.4.8."""
import numpy as np
import pytest
import torch

import pca_yardstick as Y

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
SHAPES = [(1, 8, 1), (33, 72, 33), (129, 64, 96), (300, 2048, 256), (257, 4096, 40)]      # (n, d_in, d_out)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_padded(x, A, b, fill=-7.5):
    """lrx_linear_transform with ldx = d_in + 8 and ldo = d_out + 4 -> (out [n, d_out], the padding columns of out)."""
    from lightretriever_amd.transform import linear_transform
    n, d_in = x.shape
    d_out = A.shape[0]
    xb = torch.full((n, d_in + 8), 1e30, dtype=torch.float32, device="cuda")               # (the padding must never be read into a result)
    xb[:, :d_in] = dev(x)
    ob = torch.full((n, d_out + 4), fill, dtype=torch.float32, device="cuda")
    linear_transform(xb[:, :d_in], dev(A), None if b is None else dev(b), out=ob[:, :d_out])
    torch.cuda.synchronize()
    return ob[:, :d_out].cpu().numpy(), ob[:, d_out:].cpu().numpy()


# ---- 1. exact probe ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d_in,d_out", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_integer_probe_is_exact(n, d_in, d_out, bias):
    """Integers in [-3, 3] (b in [-100, 100]): every partial sum stays below 2^24, so any order of summation is exact and the result must be
    the int64 one bit for bit; an operand on the wrong lane, a dropped k or a row / column swap cannot hide (x, A are not symmetric)."""
    rng = np.random.default_rng(n + d_in)
    x = rng.integers(-3, 4, (n, d_in)).astype(np.float32)
    A = rng.integers(-3, 4, (d_out, d_in)).astype(np.float32)
    b = rng.integers(-100, 101, d_out).astype(np.float32) if bias else None
    want = x.astype(np.int64) @ A.astype(np.int64).T + (b.astype(np.int64) if bias else 0)
    assert np.abs(want).max() < 2 ** 24
    got, pad = run_padded(x, A, b)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))
    assert (pad == -7.5).all()


@pytest.mark.parametrize("d_out", [40, 96])
def test_the_tile_rule_does_not_show(d_out):
    """Fewer than 128 tiles of 128 rows run on 64 x 64 tiles, anything larger on 128 x 64 (d_out <= 64) or 128 x 128: 16 256 rows are the
    last call of the first kind, 16 257 the first of the second.  Both are exact on integers, and on Gaussian rows they agree bit for bit."""
    from lightretriever_amd.transform import linear_transform
    rng = np.random.default_rng(d_out)
    n, d_in = 16257, 72
    x = rng.integers(-3, 4, (n, d_in)).astype(np.float32)
    A = rng.integers(-3, 4, (d_out, d_in)).astype(np.float32)
    b = rng.integers(-100, 101, d_out).astype(np.float32)
    want = (x.astype(np.int64) @ A.astype(np.int64).T + b.astype(np.int64)).astype(np.float32)
    for rows in (n, n - 1):
        got, pad = run_padded(x[:rows], A, b)
        assert np.array_equal(got, want[:rows]) and (pad == -7.5).all(), rows
    g = torch.Generator(device="cuda").manual_seed(d_out)
    xg, Ag, bg = (torch.randn(*s, device="cuda", generator=g) for s in ((n, d_in), (d_out, d_in), (d_out,)))
    large, small = linear_transform(xg, Ag, bg), linear_transform(xg[:n - 1], Ag, bg)
    assert torch.equal(large[:n - 1].view(torch.int32), small.view(torch.int32))
    assert torch.equal(linear_transform(xg[n - 1:], Ag, bg).view(torch.int32), large[n - 1:].view(torch.int32))


def test_integer_probe_on_the_large_tile_at_full_depth():
    """8192 x 2048 -> 256: 128 tiles of 128 x 128, 64 k-slices each (the reference in fp64: exact for these integers)."""
    rng = np.random.default_rng(11)
    x = rng.integers(-3, 4, (8192, 2048)).astype(np.float32)
    A = rng.integers(-3, 4, (256, 2048)).astype(np.float32)
    b = rng.integers(-100, 101, 256).astype(np.float32)
    got, pad = run_padded(x, A, b)
    assert np.array_equal(got, (x.astype(np.float64) @ A.astype(np.float64).T + b).astype(np.float32)) and (pad == -7.5).all()


def test_zero_rows_and_torch_op_shapes():
    from lightretriever_amd import torch_ops  # noqa: F401
    from lightretriever_amd.transform import linear_transform
    A = torch.ones(5, 16, device="cuda")
    x0 = torch.empty(0, 16, device="cuda")
    assert linear_transform(x0, A).shape == (0, 5) and torch.ops.lrx.linear_transform(x0, A, None).shape == (0, 5)
    with pytest.raises(Exception, match="d_in=12"):
        linear_transform(torch.ones(3, 12, device="cuda"), torch.ones(5, 12, device="cuda"))
    with pytest.raises(RuntimeError, match="d_in=12"):
        torch.ops.lrx.linear_transform(torch.ones(3, 12, device="cuda"), torch.ones(5, 12, device="cuda"), None)


# ---- 2. precision bound -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d_in,d_out", SHAPES)
def test_error_stays_inside_the_fp32_chain_bound(n, d_in, d_out):
    """|y - y64| <= (d_in + 1) 2^-23 (|A| |x| + |b|) elementwise (pca_yardstick.apply_bound: at most two roundings per step of an fp32 chain,
    in any order).  An fp32 chain sits at a few percent of it; a 16-bit operand anywhere is at 2^-9 relative and fails it."""
    rng = np.random.default_rng(d_in + d_out)
    x = rng.standard_normal((n, d_in))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    # orthonormal rows (orthonormal columns where d_out > d_in: no 96 rows of 64 elements are orthonormal)
    A = (np.linalg.qr(rng.standard_normal((d_in, d_out)))[0].T if d_out <= d_in else np.linalg.qr(rng.standard_normal((d_out, d_in)))[0]).astype(np.float32)
    assert A.shape == (d_out, d_in)
    b = (0.1 * rng.standard_normal(d_out)).astype(np.float32)
    got, _ = run_padded(x, A, b)
    err, bound = np.abs(got.astype(np.float64) - Y.apply(x, A, b)), Y.apply_bound(x, A, b)
    print(f"precision {n}x{d_in}->{d_out}: worst |err| / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all()


# ---- 3. determinism and batch independence -----------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch():
    from lightretriever_amd import torch_ops  # noqa: F401
    from lightretriever_amd.transform import linear_transform
    g = torch.Generator(device="cuda").manual_seed(3)
    n, d_in, d_out = 1000, 256, 64
    x = torch.randn(n, d_in, device="cuda", generator=g)
    A = torch.randn(d_out, d_in, device="cuda", generator=g)
    b = torch.randn(d_out, device="cuda", generator=g)
    whole = linear_transform(x, A, b)
    same = lambda a, c: torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert same(linear_transform(x, A, b), whole)                                           # twice
    for piece in (1, 127, 128, 129):
        parts = [linear_transform(x[s:s + piece], A, b) for s in range(0, n if piece > 1 else 140, piece)]
        assert same(torch.cat(parts), whole[:sum(p.shape[0] for p in parts)]), piece
    assert same(linear_transform(x[3:], A, b), whole[3:])                                   # an offset view: other rows share a tile
    wide = torch.zeros(n, d_in + 9, device="cuda")
    wide[:, 1:d_in + 1] = x
    assert same(linear_transform(wide[:, 1:d_in + 1], A, b), whole)                         # rows that are not 16-byte aligned
    assert same(torch.ops.lrx.linear_transform(x, A, b), whole)
    assert same(torch.ops.lrx.linear_transform(x[5:], A, None), linear_transform(x[5:], A))
    # a wider A: the columns a row shares its tile with do not matter either
    A2 = torch.cat([A, torch.randn(70, d_in, device="cuda", generator=g)])
    b2 = torch.cat([b, torch.randn(70, device="cuda", generator=g)])
    assert same(linear_transform(x, A2, b2)[:, :d_out].contiguous(), whole)


# ---- 4. training --------------------------------------------------------------------------------------------------------------------
D_IN, D_OUT = 256, 64


@pytest.fixture(scope="module")
def planted():
    return Y.planted(20_000, D_IN, D_OUT, seed=0)


@pytest.fixture(scope="module")
def yard(planted):
    return Y.train(planted, D_OUT)


@pytest.fixture(scope="module")
def trained(planted):
    from lightretriever_amd import PCAMatrix
    pca = PCAMatrix(D_IN, D_OUT)
    pca.train(planted)
    return pca


STATE = ("mean", "eigenvalues", "PCAMat", "A", "b")


def test_training_is_deterministic_and_callable_again(planted, trained):
    from lightretriever_amd import PCAMatrix
    again = PCAMatrix(D_IN, D_OUT)
    again.train(torch.from_numpy(planted).cuda())                                           # (device rows or host rows: the same bits)
    for k in STATE:
        a, c = getattr(trained, k), getattr(again, k)
        assert a.dtype == torch.float32 and a.is_cuda and torch.equal(a.view(torch.int32), c.view(torch.int32)), k
    again.train(planted[:5000])                                                             # replaces the previous state
    assert again.is_trained and not torch.equal(again.A, trained.A)
    again.train(planted)
    assert torch.equal(again.A.view(torch.int32), trained.A.view(torch.int32)) and torch.equal(again.b, trained.b)
    assert trained.mean.shape == (D_IN,) and trained.eigenvalues.shape == (D_IN,) and trained.PCAMat.shape == (D_IN, D_IN)
    assert trained.A.shape == (D_OUT, D_IN) and trained.b.shape == (D_OUT,) and torch.equal(trained.A, trained.PCAMat[:D_OUT])


def test_trained_matrix_against_the_fp64_yardstick(planted, trained, yard):
    lam = trained.eigenvalues.double().cpu().numpy()
    P = trained.PCAMat.double().cpu().numpy()
    A = trained.A.double().cpu().numpy()
    b = trained.b.double().cpu().numpy()
    n = planted.shape[0]
    assert (np.diff(lam) <= 0).all()
    assert (P[np.arange(D_IN), np.argmax(np.abs(P), axis=1)] > 0).all()                     # the sign rule
    # the fp32 rounding of fp64 unit eigenvectors: |delta| <= 2^-24 |v| per component, so |<a_i, a_j> - delta_ij| <= 2 2^-24 (1 + o(1))
    ortho = np.abs(A @ A.T - np.eye(D_OUT)).max()
    C, lam64 = yard["C"], yard["eigenvalues"]
    diag = np.abs(A @ C @ A.T - np.diag(lam[:D_OUT])).max()
    print(f"training: |A A^T - I| = {ortho:.3e} (bound {2.0 ** -22:.3e}), |A C A^T - diag| = {diag:.3e} (bound {2.0 ** -21 * lam64[0]:.3e})")
    assert ortho <= 2.0 ** -22
    assert diag <= 2.0 ** -21 * lam64[0]
    absA = np.abs(A)
    for mean in (yard["mean"], trained.mean.double().cpu().numpy()):                        # b = -A mean in fp64, rounded once
        assert (np.abs(b + A @ mean) <= (D_IN + 1) * 2.0 ** -24 * (absA @ np.abs(mean))).all()
    assert (np.abs(trained.mean.double().cpu().numpy() - yard["mean"]) <= 2.0 ** -24 * np.abs(yard["mean"]) + 1e-15).all()
    # the covariance: every Gram chunk is an fp32 chain of K <= 4096 products -> (K + 1) 2^-23 |X|^T |X| over the chunks; fp64 beyond that
    s, G = trained.gram(torch.from_numpy(planted).cuda())
    mean_g = (s / n).cpu().numpy()
    C_gpu = G.cpu().numpy() / n - np.outer(mean_g, mean_g)
    assert np.array_equal(C_gpu, C_gpu.T)                                                   # (i, j) and (j, i) take the same products in the same order
    ax = np.abs(planted.astype(np.float64))
    bound = 4097 * 2.0 ** -23 * (ax.T @ ax) / n
    cov = (np.abs(C_gpu - C) / bound).max()
    print(f"training: worst |C - C64| / bound = {cov:.3e}")
    assert cov <= 1
    fro = np.linalg.norm(bound)
    assert np.abs(lam - lam64).max() <= fro + 2.0 ** -24 * lam64[0]                         # Weyl (+ the fp32 rounding of the stored eigenvalues)
    gap = lam64[D_OUT - 1] - lam64[D_OUT]
    assert 3.0 < gap < 4.5
    P64 = yard["PCAMat"][:D_OUT]
    dist = np.linalg.norm(A.T @ A - P64.T @ P64, 2)                                         # distance of the two top-64 subspaces (projectors)
    print(f"training: eigenvalue error {np.abs(lam - lam64).max():.3e} (bound {fro:.3e}), subspace distance {dist:.3e} (bound {2 * fro / gap:.3e}), gap {gap:.3f}")
    assert dist <= 2 * fro / gap + 2.0 ** -22                                               # Davis-Kahan (+ the rounding of A)


def test_subsample_and_eigen_power(planted, trained, yard):
    from lightretriever_amd import PCAMatrix
    sub = PCAMatrix(D_IN, D_OUT)
    sub.max_points_per_d = 2
    rows = Y.subsample(planted.shape[0], D_IN, 2)
    assert rows.size == 512 and np.array_equal(sub.sample_rows(planted.shape[0]), rows) and trained.sample_rows(planted.shape[0]) is None
    sub.train(planted)
    ys = Y.train(planted, D_OUT, max_points_per_d=2)
    assert np.array_equal(ys["rows"], rows)
    assert (np.abs(sub.mean.double().cpu().numpy() - ys["mean"]) <= 2.0 ** -24 * np.abs(ys["mean"]) + 1e-15).all()
    As = sub.A.double().cpu().numpy()
    assert np.abs(As @ As.T - np.eye(D_OUT)).max() <= 2.0 ** -22
    assert np.abs(As @ ys["C"] @ As.T - np.diag(sub.eigenvalues.double().cpu().numpy()[:D_OUT])).max() <= 2.0 ** -21 * ys["eigenvalues"][0]
    # whitening: the same eigenvectors, each row of A scaled by eigenvalue^-0.5 in fp64 and rounded once
    white = PCAMatrix(D_IN, D_OUT, eigen_power=-0.5)
    white.train(planted)
    assert torch.equal(white.PCAMat, trained.PCAMat) and torch.equal(white.eigenvalues, trained.eigenvalues)
    want = trained.PCAMat[:D_OUT].double().cpu().numpy() * (trained.eigenvalues[:D_OUT].double().cpu().numpy() ** -0.5)[:, None]
    Aw = white.A.double().cpu().numpy()
    assert (np.abs(Aw - want) <= 2.0 ** -23 * np.abs(want)).all()                          # (one fp32 rounding; the pow of two libraries may differ in its last fp64 bit)
    assert (np.abs(white.b.double().cpu().numpy() + Aw @ yard["mean"]) <= (D_IN + 1) * 2.0 ** -24 * (np.abs(Aw) @ np.abs(yard["mean"]))).all()
    y = white.apply(planted[:4000]).double().cpu().numpy()
    cov = y.T @ y / 4000 - np.outer(y.mean(0), y.mean(0))
    assert np.abs(cov - np.eye(D_OUT)).max() < 0.15                                         # whitened: sampling noise of 4000 rows only
    with pytest.raises(ValueError, match="eigen_power"):
        white.reverse_transform(y[:2].astype(np.float32))


# ---- 5. composition -----------------------------------------------------------------------------------------------------------------
def fp64_topk(q, c, k):
    """(q.double() @ c.double().T).float(); the best k per query, ties to the lower row."""
    S = (q.double() @ c.double().T).float()
    v, j = torch.sort(S, dim=1, descending=True, stable=True)
    return v[:, :k].contiguous(), j[:, :k].contiguous()


def assert_same(got, want):
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


def make_base(kind, capacity=0):
    from lightretriever_amd import FlatIPIndex, PQIndex, SQ8Index, SQFp16Index
    return {"flat": lambda: FlatIPIndex(D_OUT, capacity=capacity), "sq_fp16": lambda: SQFp16Index(D_OUT), "sq8": lambda: SQ8Index(D_OUT, "QT_8bit_uniform"),
            "pq": lambda: PQIndex(D_OUT, 8)}[kind]()


@pytest.fixture(scope="module")
def corpus(planted):
    return torch.from_numpy(planted[:5000]).cuda(), torch.from_numpy(planted[5000:5009]).cuda()


@pytest.mark.parametrize("kind", ["flat", "sq_fp16", "sq8", "pq"])
def test_composition_equals_the_base_fed_the_transformed_rows(kind, trained, corpus):
    from lightretriever_amd import PreTransformIndex
    x, q = corpus
    k = 10
    y, yq = trained.apply(x), trained.apply(q)
    direct = make_base(kind)
    if not getattr(direct, "is_trained", True):
        direct.train(y)
    direct.add(y)
    want = direct.search(yq, k)
    idx = PreTransformIndex(trained, make_base(kind))
    assert idx.d == D_IN and idx.ntotal == 0 and idx.device == direct.device and idx.is_trained == (kind in ("flat", "sq_fp16"))
    if not idx.is_trained:
        with pytest.raises(RuntimeError, match="not trained"):
            idx.add(x)
        idx.train(x)                                                                        # trains the base on apply(x); the transform is left alone
        assert idx.is_trained and idx.transform is trained
    idx.add(x[:2000])                                                                       # two pieces, the second from the host
    idx.add(x[2000:].cpu().numpy())
    assert idx.ntotal == 5000
    assert_same(idx.search(q, k), want)
    assert_same(idx.search(q.cpu().numpy(), k), want)
    if kind == "flat":
        assert_same(want, fp64_topk(yq, y, k))                                              # the flat index's own contract over the reduced rows
        assert torch.equal(idx.index.vectors.view(torch.int32), y.view(torch.int32))       # the kernel wrote the slot itself
    # id_base is the base's
    idx.id_base = 100
    assert direct.id_base == 0 and idx.index.id_base == 100
    D, I = idx.search(q, k)
    assert torch.equal(I, want[1] + 100) and torch.equal(D, want[0])
    idx.id_base = 0
    # reconstruct_n: the base's rows through reverse_transform, within the fp32 chain bound of A^T (one more rounding: y - b)
    rows = idx.index.reconstruct_n(7, 50) if kind != "flat" else idx.index.vectors[7:57]
    rec = idx.reconstruct_n(7, 50).double().cpu().numpy()
    A, b = trained.A.double().cpu().numpy(), trained.b.double().cpu().numpy()
    z = rows.double().cpu().numpy() - b
    assert rec.shape == (50, D_IN) and (np.abs(rec - z @ A) <= (D_OUT + 1) * 2.0 ** -23 * (np.abs(z) @ np.abs(A))).all()
    with pytest.raises(ValueError):
        idx.reconstruct_n(4990, 20)
    # reset keeps the training of both parts; append_slot / commit is what the encoder path uses
    idx.reset()
    assert idx.ntotal == 0 and idx.is_trained
    slot = idx.append_slot(5000)
    assert slot.shape == (5000, D_IN) and slot.dtype == torch.float32
    slot.copy_(x)
    idx.commit(5000)
    assert idx.ntotal == 5000 and idx._stage is None
    assert_same(idx.search(q, k), want)
    # range search: a pass-through to the base; a base without it raises its own error
    radius = float(want[0][:, 4].min())
    if kind == "sq8":
        with pytest.raises(NotImplementedError, match="band rescoring"):
            idx.range_search(q, radius)
    else:
        got, ref = idx.range_search(q, radius), direct.range_search(yq, radius)
        assert all(torch.equal(a, c) for a, c in zip(got, ref)) and int(got[0][-1]) >= 4 * q.shape[0]


@pytest.mark.parametrize("kind", ["flat", "pq"])
def test_commit_trains_an_untrained_index(kind, planted, corpus):
    """append_slot / commit with nothing trained: commit trains the transform on the staged rows, the base on their image, then adds them."""
    from lightretriever_amd import PCAMatrix, PreTransformIndex
    x, q = corpus
    idx = PreTransformIndex(PCAMatrix(D_IN, D_OUT), make_base(kind))
    assert not idx.is_trained
    idx.append_slot(5000).copy_(x)
    idx.commit(5000)
    assert idx.is_trained and idx.ntotal == 5000
    ref = PCAMatrix(D_IN, D_OUT)
    ref.train(x)
    assert torch.equal(idx.transform.A.view(torch.int32), ref.A.view(torch.int32))
    direct = make_base(kind)
    y = ref.apply(x)
    if kind == "pq":
        direct.train(y)
    direct.add(y)
    assert_same(idx.search(q, 10), direct.search(ref.apply(q), 10))
    with pytest.raises(ValueError, match="staged"):
        idx.commit(3)


# ---- 6. searcher and persistence ----------------------------------------------------------------------------------------------------
def test_searcher_indexes_reuses_the_matrix_and_reloads(tmp_path, planted, corpus):
    from lightretriever_amd import FlatIPIndex, PCAMatrix, PreTransformIndex, SQFp16Index
    from lightretriever_amd.retriever import HybridSearch, PCAFaissSearch, _to_result_dict
    x, q = corpus
    ids = [f"doc{i}" for i in range(5000)]
    qids = [f"q{i}" for i in range(q.shape[0])]
    s = HybridSearch(model=None, batch_size=8, faiss_search_map="pca", output_dimension=D_OUT, show_progress_bar=False).dense_search
    assert isinstance(s, PCAFaissSearch)
    s.index(x, ids)
    assert isinstance(s.faiss_index.index, PreTransformIndex) and isinstance(s.faiss_index.index.index, FlatIPIndex) and s.dim_size == D_IN
    first = s.pca_matrix
    assert first is s.faiss_index.index.transform and first.is_trained
    ref = PCAMatrix(D_IN, D_OUT)
    ref.train(x)
    assert torch.equal(first.A.view(torch.int32), ref.A.view(torch.int32))
    direct = PreTransformIndex(ref, FlatIPIndex(D_OUT))
    direct.add(x)
    Dd, Id = direct.search(q, 10)
    want = _to_result_dict(Dd, Id, qids, ids)
    got = s.retrieve_with_emb(q, qids, 10)
    assert got == want and all(len(v) == 10 for v in got.values())
    # a second index() call (the next corpus chunk) reuses the matrix: no second training, comparable scores
    x2 = torch.from_numpy(planted[10_000:12_000]).cuda()
    s._clear()
    s.index(x2, [f"doc{i}" for i in range(10_000, 12_000)])
    second = s.pca_matrix
    assert second is not first and second is s.faiss_index.index.transform
    assert torch.equal(second.A.view(torch.int32), first.A.view(torch.int32)) and torch.equal(second.b.view(torch.int32), first.b.view(torch.int32))
    assert s.faiss_index.index.ntotal == 2000
    # save -> load: bit-equal hits, flat base and fp16-SQ base
    for base in (None, SQFp16Index(D_OUT)):
        a = PCAFaissSearch(model=None, base_index=base, output_dimension=D_OUT, batch_size=8, show_progress_bar=False)
        a.index(x, ids)
        hits = a.retrieve_with_emb(q, qids, 10)
        a.save(str(tmp_path), prefix="t")
        assert (tmp_path / "t.pca.faiss").exists() and (tmp_path / "t.pca.tsv").exists()
        c = PCAFaissSearch(model=None, output_dimension=D_OUT, batch_size=8, show_progress_bar=False)
        c.load(str(tmp_path), prefix="t")
        assert type(c.faiss_index.index.index) is (FlatIPIndex if base is None else SQFp16Index) and c.faiss_index.index.ntotal == 5000
        for k in STATE:
            assert torch.equal(getattr(c.pca_matrix, k).view(torch.int32), getattr(a.pca_matrix, k).view(torch.int32)), k
        assert c.retrieve_with_emb(q, qids, 10) == hits
        if base is None:
            assert hits == want
