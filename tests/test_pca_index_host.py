"""CPU side of the PCA pre-transform index: the self-checks of the numpy yardstick (tests/pca_yardstick.py), the 'IxPT' / 'PcAm' file layout
(index_io), the refusals and routes that need no GPU, the ABI of lrx_linear_transform with its argument checks, and the scratch-free ISA of
the new kernels."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from lightretriever_amd import _lib, build, index_io

import pca_yardstick as Y

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "lightretriever_amd", "csrc", "lrx_transform.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- the yardstick against double loops on 50 rows ------------------------------------------------------------------------------
def test_yardstick_agrees_with_double_loops_on_50_rows():
    rng = np.random.default_rng(5)
    n, d, d_out = 50, 8, 3
    x = (rng.standard_normal((n, d)) * np.linspace(3, 0.2, d) + rng.standard_normal(d)).astype(np.float32)
    mean = [sum(float(x[r, i]) for r in range(n)) / n for i in range(d)]
    C = [[sum(float(x[r, i]) * float(x[r, j]) for r in range(n)) / n - mean[i] * mean[j] for j in range(d)] for i in range(d)]
    t = Y.train(x, d_out)
    assert np.array_equal(t["rows"], np.arange(n))
    assert np.allclose(t["mean"], mean, rtol=0, atol=1e-14) and np.allclose(t["C"], C, rtol=0, atol=1e-13)
    lam, P, A, b = t["eigenvalues"], t["PCAMat"], t["A"], t["b"]
    assert (np.diff(lam) <= 0).all() and P.shape == (d, d) and A.shape == (d_out, d) and np.array_equal(A, P[:d_out])
    for i in range(d):                                                       # C v = lambda v, unit length, the sign rule
        v = P[i]
        Cv = [sum(C[a][c] * v[c] for c in range(d)) for a in range(d)]
        assert np.allclose(Cv, lam[i] * v, rtol=0, atol=1e-12)
        assert abs(sum(c * c for c in v) - 1) < 1e-14
        assert v[int(np.argmax(np.abs(v)))] > 0
    for o in range(d_out):                                                   # b = -A mean; apply / reverse, element by element
        assert abs(b[o] + sum(A[o, i] * mean[i] for i in range(d))) < 1e-14
    y = Y.apply(x, A, b)
    for r in (0, 17, n - 1):
        for o in range(d_out):
            assert abs(y[r, o] - (b[o] + sum(A[o, i] * float(x[r, i]) for i in range(d)))) < 1e-13
    back = Y.reverse(y, A, b)
    for r in (0, n - 1):
        for i in range(d):
            assert abs(back[r, i] - sum((y[r, o] - b[o]) * A[o, i] for o in range(d_out))) < 1e-13
    # the reduced rows are centred and decorrelated, their variances are the eigenvalues
    assert np.allclose(y.mean(axis=0), 0, atol=1e-13) and np.allclose(y.T @ y / n, np.diag(lam[:d_out]), rtol=0, atol=1e-12)
    # whitening scales the rows
    tw = Y.train(x, d_out, eigen_power=-0.5)
    assert np.allclose(tw["A"], A / np.sqrt(lam[:d_out])[:, None], rtol=1e-15, atol=0)
    yw = Y.apply(x, tw["A"], tw["b"])
    assert np.allclose(yw.T @ yw / n, np.eye(d_out), rtol=0, atol=1e-12)
    # composition: the top-k of the double loop over the reduced rows
    q = rng.standard_normal((3, d)).astype(np.float32)
    D, I = Y.pre_transform_search(q, x, A, b, 5)
    yq = Y.apply(q, A, b)
    for qi in range(3):
        sc = [sum(yq[qi, o] * y[r, o] for o in range(d_out)) for r in range(n)]
        order = sorted(range(n), key=lambda r: (-sc[r], r))[:5]
        assert I[qi].tolist() == order and np.allclose(D[qi], [sc[r] for r in order], rtol=1e-6)
    D, I = Y.topk(np.array([[1.0, 2.0, 2.0]], np.float32), 5, id_base=10)   # ties to the lower row, padding
    assert I.tolist() == [[11, 12, 10, -1, -1]] and (D[0, 3:] == -np.finfo(np.float32).max).all()


def test_yardstick_subsample_fix_signs_and_bound():
    assert np.array_equal(Y.subsample(100, 8), np.arange(100))
    rows = Y.subsample(100, 8, max_points_per_d=2)
    assert rows.size == 16 and (np.diff(rows) > 0).all() and rows.max() < 100
    assert np.array_equal(rows, np.sort(np.random.default_rng(Y.SEED).permutation(100)[:16]))
    assert np.array_equal(Y.fix_signs(np.array([[1.0, -2.0], [-2.0, 2.0], [0.5, 0.25]])), [[-1.0, 2.0], [2.0, -2.0], [0.5, 0.25]])
    # an fp32 chain sits far inside the bound -- its K roundings add up like a random walk, about sqrt(K) of them against the bound's 2 K, so
    # 1 / sqrt(K) is asked for here -- and operands rounded to 16 bits break it
    rng = np.random.default_rng(1)
    K = 256
    x = rng.standard_normal((40, K))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    A = np.linalg.qr(rng.standard_normal((K, K)))[0][:24].astype(np.float32)
    b = rng.standard_normal(24).astype(np.float32)
    bound = Y.apply_bound(x, A, b)
    acc = np.broadcast_to(b, (40, 24)).copy()
    for k in range(K):
        acc = (acc + (x[:, k:k + 1] * A[:, k][None, :]).astype(np.float32)).astype(np.float32)
    r32 = (np.abs(acc - Y.apply(x, A, b)) / bound).max()
    r16 = (np.abs(Y.apply(x.astype(np.float16), A.astype(np.float16), b) - Y.apply(x, A, b)) / bound).max()
    print("fp32 chain / bound:", r32, " fp16 operands / bound:", r16)
    assert r32 <= 1 / np.sqrt(K) and r16 > 1
    assert Y.planted(10).shape == (10, 256) and Y.planted(10).dtype == np.float32


# ---- the 'IxPT' / 'PcAm' file layout --------------------------------------------------------------------------------------------
def pca_state(d_in=16, d_out=8, eigen_power=0.0, seed=0):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(d_in=d_in, d_out=d_out, eigen_power=eigen_power, random_rotation=False, is_trained=True, mean=f(d_in), eigenvalues=f(d_in),
                PCAMat=f(d_in, d_in), A=f(d_out, d_in), b=f(d_out))


def write_flat(path, st, rows):
    n, d = rows.shape
    index_io.write_pre_transform(str(path), st, n, True, lambda f, prefix: index_io.write_flat_ip(f, [rows[:2], rows[2:]], d, n, prefix=prefix))


def test_ixpt_bytes_and_field_order(tmp_path):
    d_in, d_out, n = 16, 8, 5
    st = pca_state(d_in, d_out, eigen_power=-0.5)
    rows = np.random.default_rng(1).standard_normal((n, d_out)).astype(np.float32)
    path = tmp_path / "a.pca.faiss"
    write_flat(path, st, rows)
    b = path.read_bytes()
    assert b[:4] == b"IxPT"
    assert struct.unpack_from("<iqqqBi", b, 4) == (d_in, n, 1 << 20, 1 << 20, 1, 0)    # the IxFI index header, d = d_in
    assert struct.unpack_from("<i", b, 37) == (1,)                                      # nchain
    assert b[41:45] == b"PcAm"
    assert struct.unpack_from("<ffBi", b, 45) == (-0.5, 0.0, 0, 0)                      # eigen_power, epsilon, random_rotation, balanced_bins
    off = 58
    for name, size in (("mean", d_in), ("eigenvalues", d_in), ("PCAMat", d_in * d_in)):
        assert struct.unpack_from("<Q", b, off) == (size,), name
        assert np.array_equal(np.frombuffer(b[off + 8:off + 8 + 4 * size], "<f4"), st[name].reshape(-1)), name
        off += 8 + 4 * size
    assert b[off] == 1                                                                  # have_bias
    off += 1
    for name, size in (("A", d_out * d_in), ("b", d_out)):
        assert struct.unpack_from("<Q", b, off) == (size,), name
        assert np.array_equal(np.frombuffer(b[off + 8:off + 8 + 4 * size], "<f4"), st[name].reshape(-1)), name
        off += 8 + 4 * size
    assert struct.unpack_from("<iiB", b, off) == (d_in, d_out, 1)                       # d_in, d_out, is_trained
    off += 9
    assert b[off:off + 4] == b"IxFI" and struct.unpack_from("<iq", b, off + 4) == (d_out, n)
    assert len(b) == off + index_io.HEADER_BYTES + 4 * n * d_out
    flat = tmp_path / "flat"                                                            # the sub-record is the flat writer's own record
    index_io.write_flat_ip(str(flat), [rows], d_out, n)
    assert b[off:] == flat.read_bytes()
    got, base = index_io.read_pre_transform(str(path))
    assert base == dict(offset=off, fourcc=b"IxFI", qtype=None, d=d_in, ntotal=n, is_trained=True)
    assert got["d_in"] == d_in and got["d_out"] == d_out and got["eigen_power"] == -0.5 and got["random_rotation"] is False and got["is_trained"] is True
    for name in ("mean", "eigenvalues", "PCAMat", "A", "b"):
        assert got[name].shape == st[name].shape and np.array_equal(got[name], st[name]), name
    assert np.array_equal(index_io.read_flat_ip(str(path), off), rows)


def test_ixpt_round_trip_over_an_fp16_sq_sub_record_and_untrained(tmp_path):
    d_in, d_out, n = 128, 64, 7
    st = pca_state(d_in, d_out)
    codes = np.random.default_rng(2).standard_normal((n, d_out)).astype(np.float16)
    path = tmp_path / "b.pca.faiss"
    index_io.write_pre_transform(str(path), st, n, True, lambda f, prefix: index_io.write_sq_fp16(f, [codes], d_out, n, prefix=prefix))
    got, base = index_io.read_pre_transform(str(path))
    assert base["fourcc"] == b"IxSQ" and base["qtype"] == index_io.QT_FP16 and base["ntotal"] == n
    assert np.array_equal(got["A"], st["A"]) and np.array_equal(index_io.read_sq_fp16(str(path), base["offset"]), codes)
    assert index_io.sq_qtype(str(path), base["offset"]) == index_io.QT_FP16
    # the readers of the other classes refuse the sub-record; without the offset the file is no base index at all
    with pytest.raises(ValueError, match="IxFI"):
        index_io.read_flat_ip(str(path), base["offset"])
    with pytest.raises(ValueError):
        index_io.read_sq_fp16(str(path))
    # 8-bit and PQ sub-records
    trained = np.arange(2, dtype=np.float32)
    c8 = np.random.default_rng(3).integers(0, 256, (n, d_out)).astype(np.uint8)
    index_io.write_pre_transform(str(path), st, n, True, lambda f, prefix: index_io.write_sq8(f, trained, [c8], d_out, n, 2, prefix=prefix))
    _, base = index_io.read_pre_transform(str(path))
    assert base["qtype"] == 2
    qt, t2, codes2, tr = index_io.read_sq8(str(path), base["offset"])
    assert qt == 2 and tr and np.array_equal(t2, trained) and np.array_equal(codes2, c8)
    cent = np.random.default_rng(4).standard_normal((8, 256, 8)).astype(np.float32)
    cpq = c8[:, :8].copy()
    index_io.write_pre_transform(str(path), st, n, True, lambda f, prefix: index_io.write_pq(f, cent, [cpq], d_out, 8, n, prefix=prefix))
    _, base = index_io.read_pre_transform(str(path))
    assert base["fourcc"] == b"IxPq"
    cent2, codes2, tr = index_io.read_pq(str(path), base["offset"])
    assert tr and np.array_equal(cent2, cent) and np.array_equal(codes2, cpq)
    # an untrained transform: empty vectors, is_trained = 0 in both places
    un = dict(d_in=d_in, d_out=d_out, eigen_power=0.0, random_rotation=False, is_trained=False,
              **{k: np.zeros(0, np.float32) for k in ("mean", "eigenvalues", "PCAMat", "A", "b")})
    index_io.write_pre_transform(str(path), un, 0, False, lambda f, prefix: index_io.write_flat_ip(f, [], d_out, 0, prefix=prefix))
    got, base = index_io.read_pre_transform(str(path))
    assert got["is_trained"] is False and base["is_trained"] is False and base["ntotal"] == 0 and got["A"].size == 0
    with pytest.raises(ValueError, match="mean"):
        index_io.pre_transform_prefix(dict(st, mean=st["mean"][:3]), n)


def test_ixpt_rejects_bad_files(tmp_path):
    d_in, d_out, n = 16, 8, 4
    st = pca_state(d_in, d_out)
    rows = np.random.default_rng(1).standard_normal((n, d_out)).astype(np.float32)
    path = tmp_path / "a"
    write_flat(path, st, rows)
    b = path.read_bytes()
    base_off = index_io.read_pre_transform(str(path))[1]["offset"]
    bad = tmp_path / "b"

    def refused(blob, match=None):
        bad.write_bytes(bytes(blob))
        with pytest.raises(ValueError, match=match):
            pca, base = index_io.read_pre_transform(str(bad))
            index_io.read_flat_ip(str(bad), base["offset"])

    for cut in (b[:-1], b[:base_off + 10], b[:base_off + 2], b[:base_off], b[:base_off - 3], b[:200], b[:60], b[:50], b[:39], b[:20], b""):
        refused(cut)
    refused(b"IxFI" + b[4:], "IxPT")
    for nchain in (0, 2):
        b2 = bytearray(b)
        struct.pack_into("<i", b2, 37, nchain)
        refused(b2, "chain")
    for tcc in (b"PCAm", b"rrot", b"LTra"):                                             # the legacy PCA record, other transforms
        refused(b[:41] + tcc + b[45:], "PcAm")
    b2 = bytearray(b)
    struct.pack_into("<f", b2, 49, 1e-3)                                                # epsilon
    refused(b2, "epsilon")
    b2 = bytearray(b)
    struct.pack_into("<Q", b2, 58, d_in - 1)                                            # a vector of the wrong length shifts everything after it
    refused(b2)
    b2 = bytearray(b)
    struct.pack_into("<Q", b2, 58, 1 << 40)
    refused(b2, "truncated")
    b2 = bytearray(b)
    struct.pack_into("<i", b2, base_off - 9, d_in + 8)                                  # d_in of the transform against the header's d
    refused(b2, "inconsistent")
    b2 = bytearray(b)
    struct.pack_into("<i", b2, base_off - 5, d_out - 1)
    refused(b2, "inconsistent")
    refused(b[:base_off] + b"IBxF" + b[base_off + 4:], "base index")
    # the plain readers are unchanged: no offset, whole file
    flat = tmp_path / "flat"
    index_io.write_flat_ip(str(flat), [rows], d_out, n)
    assert np.array_equal(index_io.read_flat_ip(str(flat)), rows)
    with pytest.raises(ValueError):
        index_io.read_flat_ip(str(flat), 4)


# ---- refusals and routes, without a GPU -------------------------------------------------------------------------------------------
def test_refusals_need_no_gpu():
    from lightretriever_amd import BinaryFlatIndex, FlatIPIndex, PCAMatrix, PreTransformIndex
    with pytest.raises(NotImplementedError, match="random_rotation"):
        PCAMatrix(64, 16, 0.0, True)
    with pytest.raises(ValueError, match="d_out=65"):
        PCAMatrix(64, 65)
    with pytest.raises(ValueError, match="multiple of 8"):
        PCAMatrix(36, 16)
    pca = PCAMatrix(64, 16, eigen_power=-0.5)
    assert (pca.d_in, pca.d_out, pca.eigen_power, pca.random_rotation, pca.is_trained) == (64, 16, -0.5, False, False)
    with pytest.raises(ValueError, match="15 training rows"):
        pca.train(np.zeros((15, 64), np.float32))
    with pytest.raises(ValueError, match=r"\[n,64\]"):
        pca.train(np.zeros((100, 32), np.float32))
    for call in (pca.apply, pca.reverse_transform):
        with pytest.raises(RuntimeError, match="not trained"):
            call(np.zeros((1, 64), np.float32))
    other = PCAMatrix(64, 16)
    assert other.copy_from(pca) is other and other.eigen_power == -0.5                  # the reference uses the return value
    with pytest.raises(ValueError, match="copy_from"):
        PCAMatrix(64, 8).copy_from(pca)
    binary = BinaryFlatIndex.__new__(BinaryFlatIndex)                                   # (no GPU here: the refusal needs no state)
    with pytest.raises(TypeError, match="BinaryFlatIndex"):
        PreTransformIndex(pca, binary)
    with pytest.raises(TypeError, match="PCAMatrix"):
        PreTransformIndex(object(), binary)
    flat = FlatIPIndex.__new__(FlatIPIndex)
    flat.d = 32
    with pytest.raises(ValueError, match="d_out=16"):
        PreTransformIndex(pca, flat)


def test_routes_and_searcher_arguments():
    import lightretriever.retriever.faiss_search as shim
    from lightretriever_amd import BinaryFlatIndex, PreTransformIndex
    from lightretriever_amd.retriever import FlatIPFaissSearch, HybridSearch, PCAFaissSearch
    assert shim.PCAFaissSearch is PCAFaissSearch
    h = HybridSearch(model=None, batch_size=8, faiss_search_map="pca", output_dimension=64, show_progress_bar=False)
    s = h.dense_search
    assert type(s) is PCAFaissSearch and s.output_dim == 64 and s.base_index is None and s.pca_matrix is None and s.eigen_power == 0.0
    assert s.get_index_name() == "pca_faiss_index" and s.index_ext == "pca" and s.serves_rpc_shards is False and s.index_cls is PreTransformIndex
    assert HybridSearch(model=None, faiss_search_map="pca", output_dimension=32, eigen_power=-0.5).dense_search.eigen_power == -0.5
    with pytest.raises(ValueError, match="output_dimension"):
        HybridSearch(model=None, faiss_search_map="pca")
    with pytest.raises(ValueError, match="output_dimension"):
        PCAFaissSearch(model=None)
    with pytest.raises(NotImplementedError, match="random_rotation"):
        HybridSearch(model=None, faiss_search_map="pca", output_dimension=64, random_rotation=True)
    with pytest.raises(TypeError, match="BinaryFlatIndex"):
        PCAFaissSearch(model=None, base_index=BinaryFlatIndex.__new__(BinaryFlatIndex), output_dimension=64)
    assert type(HybridSearch(model=None, faiss_search_map="hnsw").dense_search) is FlatIPFaissSearch      # unknown maps: still flat
    assert type(HybridSearch(model=None, faiss_search_map="hnswsq", output_dimension=64).dense_search) is FlatIPFaissSearch


# ---- ABI and argument checks --------------------------------------------------------------------------------------------------------
def test_symbol_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "lrx.h")).read()
    l = ctypes.CDLL(build.build(verbose=False))
    assert "lrx_linear_transform(" in hdr and hasattr(l, "lrx_linear_transform") and "lrx_linear_transform" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["lrx_linear_transform"][1]) == 10
    assert "#define LRX_ABI_VERSION 9" in hdr and _lib.lib().lrx_abi_version() == _lib.ABI_VERSION == 9
    assert "lrx_transform.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "lightretriever_amd", "csrc", "lrx_search.hip")).read()
    assert "k_lt_" not in src and "lrx_transform" not in src                            # (tests count that file's kernels by prefix)
    assert os.path.exists(build.build_torch_ops(verbose=False))
    import torch
    from lightretriever_amd import torch_ops
    assert "linear_transform" in torch_ops.OPS
    assert str(torch.ops.lrx.linear_transform.default._schema) == "lrx::linear_transform(Tensor x, Tensor A, Tensor? b=None) -> Tensor"


FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work


def _lt(l, *, x=FAKE, n_rows=10, ldx=64, A=FAKE, b=FAKE, d_in=64, d_out=16, out=FAKE, ldo=16):
    return l.lrx_linear_transform(x, n_rows, ldx, A, b, d_in, d_out, out, ldo, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(d_in=12, ldx=12), b"d_in=12"), (dict(d_in=0), b"d_in=0"), (dict(d_in=8200, ldx=8200), b"d_in=8200"), (dict(d_in=4), b"d_in=4"),
    (dict(ldx=63), b"ldx=63"), (dict(ldo=15), b"ldo=15"), (dict(d_out=0), b"d_out=0"), (dict(n_rows=-1), b"n_rows=-1"),
    (dict(x=None), b"null"), (dict(A=None), b"null"), (dict(out=None), b"null"),
])
def test_argument_errors_are_reported_without_a_gpu(kw, msg):
    l = _lib.lib()
    assert _lt(l, **kw) == -1, kw                    # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())


def test_zero_rows_launch_nothing():
    assert _lt(_lib.lib(), n_rows=0, x=None, out=None) == 0


# ---- the kernels' descriptors ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def transform_isa():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "t.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def test_transform_kernels_have_no_scratch_and_use_the_f32_mfma(transform_isa):
    """The kernel descriptors (the metadata hipcc emits) say: no private segment, no spilled register; the kernels' text holds the f32-input
    MFMA."""
    desc = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", transform_isa, re.S):
        name = re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)
        desc[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(0)).group(1))
                      for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    assert len(desc) == 3 and all("k_lt_" in n for n in desc), sorted(desc)            # 128 x 128, 128 x 64 and 64 x 64 tiles; the file holds nothing else
    for name, d in desc.items():
        assert d == {"private_segment_fixed_size": 0, "vgpr_spill_count": 0, "sgpr_spill_count": 0}, (name, d)
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), transform_isa, re.S | re.M).group(0)
        assert "v_mfma_f32_32x32x2_f32" in body, name
