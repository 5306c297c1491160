"""CPU side of the exact re-ranking (RefineFlatIndex, faiss IndexRefineFlat): the ABI of lrx_flat_ip_rerank / lrx_sq_fp16_ip_rerank with their
argument checks, the 'IxRF' file layout (index_io) and the end bound of the older readers, the refusals and routes that need no GPU, and the
self-checks of the numpy yardstick (tests/refine_yardstick.py)."""
import ctypes
import os
import struct

import numpy as np
import pytest

from lightretriever_amd import _lib, build, index_io

import refine_yardstick as Y

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLT_MAX = np.finfo(np.float32).max


# ---- the yardstick against double loops on 50 rows ------------------------------------------------------------------------------
def test_yardstick_agrees_with_double_loops_on_50_rows():
    rng = np.random.default_rng(3)
    n, d, Q, k = 50, 12, 4, 6
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[7] = X[3]                                                              # equal scores: the lower row first
    q = rng.standard_normal((Q, d)).astype(np.float32)
    cand = rng.integers(0, n, (Q, 15))
    cand[0] = [7, 3, -1, 3] + [-1] * 11                                      # a tie, padding, a duplicate
    cand[1, :3] = [n, n + 5, -1]                                             # rows that do not exist
    cand[2] = -1                                                             # nothing at all
    cand[3, 4:] = -1                                                         # fewer than k valid
    D, I = Y.rerank(q, X, cand, k, id_base=100)
    for i in range(Q):
        rows = [int(r) for r in cand[i] if 0 <= r < n]
        sc = {r: np.float32(sum(float(q[i, c]) * float(X[r, c]) for c in range(d))) for r in rows}
        order = sorted(rows, key=lambda r: (-float(sc[r]), r))[:k]
        assert I[i, :len(order)].tolist() == [100 + r for r in order], i
        assert np.allclose(D[i, :len(order)], [sc[r] for r in order], rtol=1e-6, atol=0), i
        assert (I[i, len(order):] == -1).all() and (D[i, len(order):] == -FLT_MAX).all()
    assert I[0].tolist() == [103, 103, 107, -1, -1, -1]                      # 3 twice, then its twin 7
    assert (I[2] == -1).all() and (I[3, 4:] == -1).all() and (I[3, :4] >= 100).all()
    row_map = np.arange(n)[::-1] * 3
    assert np.array_equal(Y.rerank(q, X, cand, k, row_map=row_map)[1], np.where(I >= 0, row_map[np.maximum(I - 100, 0)], -1))
    assert np.array_equal(Y.rerank(q, X, cand, k, n_rows=10)[1][1] >= 10, np.zeros(k, bool))
    s = Y.exact_score(q[0], X[5])
    assert s.dtype == np.float32 and s == np.float32(sum(float(a) * float(b) for a, b in zip(q[0], X[5])))
    assert np.array_equal(Y.exact_scores(q[0], X, [5, 5, 9]), [s, s, Y.exact_score(q[0], X[9])])


def test_yardstick_k_base_and_recall():
    assert [Y.k_base(10, f) for f in (1, 1.0, 1.5, 2.99, 30)] == [10, 10, 15, 29, 300]
    assert Y.k_base(7, 1.1) == 7 and Y.k_base(100, 20.48) == 2048 and Y.k_base(100, 20.49) == 2049 > Y.MAX_K_BASE
    assert Y.recall(np.array([[1, 2, 3, -1]]), np.array([[3, 4, -1, -1]])) == 0.5


# ---- ABI and argument checks --------------------------------------------------------------------------------------------------------
NAMES = ("lrx_ip_rerank_workspace_bytes", "lrx_flat_ip_rerank", "lrx_sq_fp16_ip_rerank")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "lrx.h")).read()
    l = ctypes.CDLL(build.build(verbose=False))
    for name in NAMES:
        assert name + "(" in hdr and hasattr(l, name) and name in _lib.SIGNATURES, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 17, 16]
    assert "#define LRX_ABI_VERSION 9" in hdr and _lib.lib().lrx_abi_version() == _lib.ABI_VERSION == 9
    assert '#include "lrx_search_rerank.h"' in open(os.path.join(ROOT, "lightretriever_amd", "csrc", "lrx_search.hip")).read()
    assert os.path.exists(build.build_torch_ops(verbose=False))
    import torch
    from lightretriever_amd import torch_ops
    assert "flat_ip_rerank" in torch_ops.OPS and "sq_fp16_ip_rerank" in torch_ops.OPS
    assert str(torch.ops.lrx.flat_ip_rerank.default._schema) == \
        "lrx::flat_ip_rerank(Tensor q, Tensor x, Tensor cand, int k, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)"
    assert str(torch.ops.lrx.sq_fp16_ip_rerank.default._schema) == \
        "lrx::sq_fp16_ip_rerank(Tensor q, Tensor codes, int n_rows, Tensor cand, int k, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)"


FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work
BIG = 1 << 30


def _flat(l, *, X=FAKE, n_rows=1000, ldx=64, dim=64, q=FAKE, nq=3, cand=FAKE, n_cand=40, ld_cand=40, k=10, out=FAKE, ws=FAKE, ws_bytes=BIG):
    return l.lrx_flat_ip_rerank(X, n_rows, ldx, dim, q, nq, cand, n_cand, ld_cand, k, 0, out, out, None, ws, ws_bytes, None)


def _codes(l, *, X=FAKE, n_rows=1000, dim=64, q=FAKE, nq=3, cand=FAKE, n_cand=40, ld_cand=40, k=10, out=FAKE, ws=FAKE, ws_bytes=BIG):
    return l.lrx_sq_fp16_ip_rerank(X, n_rows, dim, q, nq, cand, n_cand, ld_cand, k, 0, out, out, None, ws, ws_bytes, None)


COMMON = [(dict(k=0), b"k=0"), (dict(k=41), b"k=41"), (dict(n_cand=2049, ld_cand=2049), b"n_cand=2049"), (dict(n_cand=0, k=0), b"n_cand=0"),
          (dict(ld_cand=39), b"ld_cand=39"), (dict(n_rows=-1), b"rows=-1"), (dict(n_rows=1 << 32), b"rows=4294967296"), (dict(nq=-1), b"n_queries=-1"),
          (dict(q=None), b"null"), (dict(cand=None), b"null"), (dict(out=None), b"null"), (dict(X=None), b"null"),
          (dict(q=ctypes.c_void_p(260)), b"16-byte")]


@pytest.mark.parametrize("kw,msg", COMMON + [(dict(dim=62, ldx=62), b"dim=62"), (dict(dim=0), b"dim=0"), (dict(ldx=60), b"ldx=60"), (dict(ldx=66), b"ldx=66"),
                                             (dict(X=ctypes.c_void_p(264)), b"16-byte")])
def test_flat_rerank_argument_errors_need_no_gpu(kw, msg):
    l = _lib.lib()
    assert _flat(l, **kw) == -1, kw               # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())


@pytest.mark.parametrize("kw,msg", COMMON + [(dict(dim=32), b"dim=32"), (dict(dim=96), b"dim=96"), (dict(dim=0), b"dim=0")])
def test_codes_rerank_argument_errors_need_no_gpu(kw, msg):
    l = _lib.lib()
    assert _codes(l, **kw) == -1, kw
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())


def test_short_workspace_and_zero_queries():
    l = _lib.lib()
    need = l.lrx_ip_rerank_workspace_bytes(3, 40, 10)
    assert need >= 3 * 40 * 8 and need % 256 == 0
    assert l.lrx_ip_rerank_workspace_bytes(6, 40, 10) > need and l.lrx_ip_rerank_workspace_bytes(3, 80, 10) > need
    for call in (_flat, _codes):
        assert call(l, ws_bytes=need - 1) == -3 and b"workspace" in l.lrx_last_error()      # LRX_ERR_WORKSPACE
        assert call(l, ws=None) == -3
        assert call(l, nq=0, q=None, cand=None, out=None, ws=None, ws_bytes=0) == 0         # nothing is launched
    assert _flat(l, n_cand=2048, ld_cand=2048, k=2048, ws_bytes=l.lrx_ip_rerank_workspace_bytes(3, 2048, 2048) - 1) == -3


# ---- the 'IxRF' file layout ---------------------------------------------------------------------------------------------------------
D, M, N = 64, 8, 5


def parts(seed=0):
    rng = np.random.default_rng(seed)
    return dict(cent=rng.standard_normal((M, 256, D // M)).astype(np.float32), codes=rng.integers(0, 256, (N, M)).astype(np.uint8),
                rows=rng.standard_normal((N, D)).astype(np.float32))


def write_pq_flat(path, p, k_factor=4.0, d=D, n=N, trained=True):
    index_io.write_refine(str(path), d, n, trained, k_factor,
                          lambda f, prefix: index_io.write_pq(f, p["cent"], [p["codes"][:2], p["codes"][2:]], D, M, N, prefix=prefix),
                          lambda f: index_io.write_flat_ip(f, [p["rows"]], D, N, append=True))


def test_ixrf_bytes_field_by_field(tmp_path):
    p = parts()
    path = tmp_path / "a.refine.faiss"
    write_pq_flat(path, p)
    assert not (tmp_path / "a.refine.faiss.tmp").exists()
    b = path.read_bytes()
    assert b[:4] == b"IxRF"
    assert struct.unpack_from("<iqqqBi", b, 4) == (D, N, 1 << 20, 1 << 20, 1, 0)        # the common index header
    pq, flat = tmp_path / "pq", tmp_path / "flat"                                       # the two records are the writers' own files
    index_io.write_pq(str(pq), p["cent"], [p["codes"]], D, M, N)
    index_io.write_flat_ip(str(flat), [p["rows"]], D, N)
    pb, fb = pq.read_bytes(), flat.read_bytes()
    assert b[37:41] == b"IxPq" and b[37:37 + len(pb)] == pb
    off = 37 + len(pb)
    assert b[off:off + 4] == b"IxFI" and b[off:off + len(fb)] == fb
    assert len(b) == off + len(fb) + 4 and struct.unpack_from("<f", b, off + len(fb)) == (4.0,)
    st = index_io.read_refine(str(path))
    assert st == dict(d=D, ntotal=N, is_trained=True, k_factor=4.0, base=dict(offset=37, end=off, fourcc=b"IxPq", qtype=None),
                      store=dict(offset=off, end=off + len(fb), fourcc=b"IxFI", qtype=None))
    cent, codes, tr = index_io.read_pq(str(path), 37, off)
    assert tr and np.array_equal(cent, p["cent"]) and np.array_equal(codes, p["codes"])
    assert np.array_equal(index_io.read_flat_ip(str(path), off, off + len(fb)), p["rows"])
    assert index_io.index_record_end(str(path), 37) == off and index_io.index_record_end(str(path), off, len(b) - 4) == len(b) - 4
    # a record is followed by more: without the end bound the readers refuse it, as they refuse any file with trailing bytes
    with pytest.raises(ValueError):
        index_io.read_pq(str(path), 37)
    with pytest.raises(ValueError):
        index_io.read_flat_ip(str(path), off)
    with pytest.raises(ValueError):
        index_io.read_flat_ip(str(path), off, len(b) + 1)


def pca_state(d_in=D, d_out=16):
    rng = np.random.default_rng(9)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(d_in=d_in, d_out=d_out, eigen_power=0.0, random_rotation=False, is_trained=True, mean=f(d_in), eigenvalues=f(d_in),
                PCAMat=f(d_in, d_in), A=f(d_out, d_in), b=f(d_out))


def test_ixrf_round_trips_over_every_record_type(tmp_path):
    p = parts(1)
    path = str(tmp_path / "r")
    codes16 = p["rows"].astype(np.float16)
    c8 = np.random.default_rng(2).integers(0, 256, (N, D)).astype(np.uint8)
    t8 = np.arange(2 * D, dtype=np.float32)
    # 8-bit SQ base, fp16 store
    index_io.write_refine(path, D, N, True, 1.5, lambda f, prefix: index_io.write_sq8(f, t8, [c8], D, N, 0, prefix=prefix),
                          lambda f: index_io.write_sq_fp16(f, [codes16], D, N, append=True))
    st = index_io.read_refine(path)
    assert st["k_factor"] == 1.5 and st["base"]["fourcc"] == b"IxSQ" and st["base"]["qtype"] == 0
    assert st["store"]["fourcc"] == b"IxSQ" and st["store"]["qtype"] == index_io.QT_FP16 and st["store"]["end"] == os.path.getsize(path) - 4
    qt, t2, codes2, tr = index_io.read_sq8(path, st["base"]["offset"], st["base"]["end"])
    assert qt == 0 and tr and np.array_equal(t2, t8) and np.array_equal(codes2, c8)
    assert np.array_equal(index_io.read_sq_fp16(path, st["store"]["offset"], st["store"]["end"]), codes16)
    assert index_io.sq_qtype(path, st["store"]["offset"], st["store"]["end"]) == index_io.QT_FP16
    # fp16 SQ base (the same record type twice)
    index_io.write_refine(path, D, N, True, 1.0, lambda f, prefix: index_io.write_sq_fp16(f, [codes16], D, N, prefix=prefix),
                          lambda f: index_io.write_flat_ip(f, [p["rows"]], D, N, append=True))
    st = index_io.read_refine(path)
    assert st["base"]["qtype"] == index_io.QT_FP16 and np.array_equal(index_io.read_sq_fp16(path, st["base"]["offset"], st["base"]["end"]), codes16)
    # PCA base over a PQ sub-record: a record inside a record inside a record
    pst = pca_state()
    cent = np.random.default_rng(4).standard_normal((4, 256, 4)).astype(np.float32)
    cpq = c8[:, :4].copy()
    index_io.write_refine(path, D, N, True, 10.0,
                          lambda f, prefix: index_io.write_pre_transform(f, pst, N, True, lambda g, pre: index_io.write_pq(g, cent, [cpq], 16, 4, N, prefix=pre),
                                                                         prefix=prefix),
                          lambda f: index_io.write_flat_ip(f, [p["rows"]], D, N, append=True))
    st = index_io.read_refine(path)
    assert st["base"]["fourcc"] == b"IxPT" and st["k_factor"] == 10.0
    pca, base = index_io.read_pre_transform(path, st["base"]["offset"], st["base"]["end"])
    assert base["fourcc"] == b"IxPq" and base["d"] == D and np.array_equal(pca["A"], pst["A"])
    cent2, codes2, _ = index_io.read_pq(path, base["offset"], st["base"]["end"])
    assert np.array_equal(cent2, cent) and np.array_equal(codes2, cpq)
    assert np.array_equal(index_io.read_flat_ip(path, st["store"]["offset"], st["store"]["end"]), p["rows"])
    # an empty, untrained index
    index_io.write_refine(path, D, 0, False, 2.0, lambda f, prefix: index_io.write_pq(f, p["cent"], [], D, M, 0, False, prefix=prefix),
                          lambda f: index_io.write_flat_ip(f, [], D, 0, append=True))
    st = index_io.read_refine(path)
    assert st["ntotal"] == 0 and st["is_trained"] is False and index_io.read_flat_ip(path, st["store"]["offset"], st["store"]["end"]).shape == (0, D)


def test_ixrf_rejects_bad_files(tmp_path):
    p = parts(2)
    path = tmp_path / "a"
    write_pq_flat(path, p)
    b = path.read_bytes()
    st = index_io.read_refine(str(path))
    base_off, store_off = st["base"]["offset"], st["store"]["offset"]
    bad = tmp_path / "b"

    def refused(blob, match=None):
        bad.write_bytes(bytes(blob))
        with pytest.raises(ValueError, match=match):
            s = index_io.read_refine(str(bad))
            index_io.read_pq(str(bad), s["base"]["offset"], s["base"]["end"])
            index_io.read_flat_ip(str(bad), s["store"]["offset"], s["store"]["end"])

    for cut in (b[:-1], b[:-4], b[:-5], b[:store_off + 40], b[:store_off + 3], b[:store_off], b[:store_off - 5], b[:base_off + 60], b[:base_off + 2],
                b[:base_off], b[:20], b""):
        refused(cut)
    refused(b + b"\0")                                                                  # bytes between the refine index and k_factor
    refused(b"IxFI" + b[4:], "IxRF")
    for field, off in (("d", 4), ("ntotal", 8)):                                        # the header against its two records
        b2 = bytearray(b)
        struct.pack_into("<i" if field == "d" else "<q", b2, off, (D if field == "d" else N) + 1)
        refused(b2, "base index")
    for field, off in (("d", store_off + 4), ("ntotal", store_off + 8)):
        b2 = bytearray(b)
        struct.pack_into("<i" if field == "d" else "<q", b2, off, (D if field == "d" else N) + 1)
        refused(b2, "refine index")
    b2 = bytearray(b)
    struct.pack_into("<i", b2, 33, 1)                                                   # metric_type
    refused(b2, "inconsistent")
    refused(b[:base_off] + b"IxFI" + b[base_off + 4:], "base index")                    # record types that are not served in that place
    refused(b[:base_off] + b"IBxF" + b[base_off + 4:], "base index")
    refused(b[:store_off] + b"IxPq" + b[store_off + 4:], "refine index")
    refused(b[:store_off] + b"IxRF" + b[store_off + 4:], "refine index")
    b2 = bytearray(b)
    struct.pack_into("<Q", b2, store_off + 37, 1 << 40)                                 # a size word that points past the file
    refused(b2, "truncated")
    # an 8-bit store is not a refine store
    c8 = np.zeros((N, D), np.uint8)
    index_io.write_refine(str(bad), D, N, True, 1.0, lambda f, prefix: index_io.write_pq(f, p["cent"], [p["codes"]], D, M, N, prefix=prefix),
                          lambda f: index_io.write_sq8(f, np.zeros(2, np.float32), [c8], D, N, 2, append=True))
    with pytest.raises(ValueError, match="QT_fp16"):
        index_io.read_refine(str(bad))


def test_older_readers_accept_their_files_with_no_end_bound(tmp_path):
    p = parts(3)
    f = str(tmp_path / "f")
    index_io.write_flat_ip(f, [p["rows"]], D, N)
    size = os.path.getsize(f)
    assert np.array_equal(index_io.read_flat_ip(f), p["rows"]) and np.array_equal(index_io.read_flat_ip(f, 0, size), p["rows"])
    assert index_io.index_record_end(f) == size
    with pytest.raises(ValueError):
        index_io.read_flat_ip(f, 0, size - 1)
    index_io.write_sq_fp16(f, [p["rows"].astype(np.float16)], D, N)
    assert np.array_equal(index_io.read_sq_fp16(f), p["rows"].astype(np.float16)) and index_io.sq_qtype(f) == index_io.QT_FP16
    assert index_io.index_record_end(f) == os.path.getsize(f)
    index_io.write_sq8(f, np.arange(2, dtype=np.float32), [np.ones((N, D), np.uint8)], D, N, 2)
    assert index_io.read_sq8(f)[0] == 2 and index_io.index_record_end(f) == os.path.getsize(f)
    index_io.write_pq(f, p["cent"], [p["codes"]], D, M, N)
    assert np.array_equal(index_io.read_pq(f)[1], p["codes"]) and index_io.index_record_end(f) == os.path.getsize(f)
    with pytest.raises(ValueError):
        index_io.read_pq(f, 0, os.path.getsize(f) - 1)
    pst = pca_state()
    index_io.write_pre_transform(f, pst, N, True, lambda g, prefix: index_io.write_flat_ip(g, [p["rows"][:, :16]], 16, N, prefix=prefix))
    pca, base = index_io.read_pre_transform(f)
    assert np.array_equal(pca["A"], pst["A"]) and np.array_equal(index_io.read_flat_ip(f, base["offset"]), p["rows"][:, :16])
    assert index_io.index_record_end(f) == os.path.getsize(f)
    # append continues a file; without it a writer replaces the file
    index_io.write_flat_ip(f, [p["rows"]], D, N)
    index_io.write_flat_ip(f, [p["rows"][:2]], D, 2, append=True)
    assert os.path.getsize(f) == size + index_io.HEADER_BYTES + 2 * D * 4 and np.array_equal(index_io.read_flat_ip(f, size), p["rows"][:2])
    assert index_io.index_record_end(f) == size
    index_io.write_flat_ip(f, [p["rows"]], D, N)
    assert os.path.getsize(f) == size


# ---- refusals and routes, without a GPU -------------------------------------------------------------------------------------------
def fake(cls, **attrs):
    idx = cls.__new__(cls)                                                              # (no GPU here: the refusals need no device state)
    for k, v in attrs.items():
        setattr(idx, k, v)
    return idx


def test_refine_index_refusals_need_no_gpu():
    from lightretriever_amd import BinaryFlatIndex, FlatIPIndex, PQIndex, RefineFlatIndex, SQ8Index, SQFp16Index
    from lightretriever_amd import refine
    assert refine.MAX_K_BASE == Y.MAX_K_BASE == 2048
    assert [refine.k_base_of(10, f) for f in (1, 1.5, 2.99)] == [Y.k_base(10, f) for f in (1, 1.5, 2.99)]
    for base in (fake(FlatIPIndex), fake(BinaryFlatIndex), object()):
        with pytest.raises(TypeError, match="base index"):
            RefineFlatIndex(base)
    pq = fake(PQIndex, d=64, id_base=0, ntotal=0, device="cuda:0")
    for store in (fake(PQIndex), fake(SQ8Index), fake(BinaryFlatIndex), object()):
        with pytest.raises(TypeError, match="refine index"):
            RefineFlatIndex(pq, store)
    store = fake(FlatIPIndex, d=64, ntotal=0, device="cuda:0")
    for kf in (0.99, 0, -1, float("nan")):
        with pytest.raises(ValueError, match="k_factor"):
            RefineFlatIndex(pq, store, k_factor=kf)
    with pytest.raises(ValueError, match="id_base=5"):
        RefineFlatIndex(fake(PQIndex, d=64, id_base=5, ntotal=0), store)
    with pytest.raises(ValueError, match="d=128"):
        RefineFlatIndex(pq, fake(SQFp16Index, d=128, ntotal=0))
    with pytest.raises(ValueError, match="the refine index 3"):
        RefineFlatIndex(pq, fake(FlatIPIndex, d=64, ntotal=3))
    idx = RefineFlatIndex(pq, store, k_factor=4)
    pq.is_trained = False
    assert (idx.d, idx.ntotal, idx.device, idx.is_trained, idx.id_base, idx.k_factor) == (64, 0, "cuda:0", False, 0, 4.0)
    assert idx.base_index is pq and idx.refine_index is store
    idx.id_base = 7
    assert idx.id_base == 7 and pq.id_base == 0
    with pytest.raises(RuntimeError, match="not trained"):
        idx.add(np.zeros((1, 64), np.float32))
    with pytest.raises(NotImplementedError, match="IndexRefine"):
        idx.range_search(np.zeros((1, 64), np.float32), 0.0)
    with pytest.raises(ValueError, match="2048"):
        idx.search(np.zeros((1, 64), np.float32), 513)                                  # 513 * 4 = 2052
    with pytest.raises(ValueError, match="2048"):
        idx.search(np.zeros((1, 64), np.float32), 100, k_factor=20.49)
    with pytest.raises(ValueError, match="k_factor"):
        idx.search(np.zeros((1, 64), np.float32), 10, k_factor=0.5)
    with pytest.raises(ValueError, match="k=0"):
        idx.search(np.zeros((1, 64), np.float32), 0)


def test_routes_and_searcher_arguments():
    import lightretriever.retriever.faiss_search as shim
    from lightretriever_amd import RefineFlatIndex
    from lightretriever_amd.retriever import (FlatIPFaissSearch, HybridSearch, PCAFaissSearch, PQFaissSearch, RefineFaissSearch, SQFaissSearch)
    assert shim.RefineFaissSearch is RefineFaissSearch and issubclass(RefineFaissSearch, FlatIPFaissSearch)
    s = RefineFaissSearch(model=None, refine_base="pq", batch_size=8, show_progress_bar=False)
    assert (s.index_ext, s.serves_rpc_shards, s.get_index_name(), s.index_cls) == ("refine", False, "refine_faiss_index", RefineFlatIndex)
    assert (s.refine_base, s.k_factor, s.refine_type) == ("pq", 1.0, "flat") and type(s.base_search) is PQFaissSearch
    assert s.base_search.num_of_centroids == 96 and s.base_search.batch_size == 8 and s.show_progress_bar is False
    for bad in (None, "flat", "binary", "hnsw", "refine"):
        with pytest.raises(ValueError, match="refine_base"):
            RefineFaissSearch(model=None, refine_base=bad)
    with pytest.raises(ValueError, match="refine_type"):
        RefineFaissSearch(model=None, refine_base="pq", refine_type="bf16")
    with pytest.raises(ValueError, match="k_factor"):
        RefineFaissSearch(model=None, refine_base="pq", k_factor=0.5)
    # the base searcher's own arguments pass through unchanged, and so do its refusals
    s = RefineFaissSearch(model=None, refine_base="pq", k_factor=4, refine_type="fp16", num_of_centroids=16)
    assert s.base_search.num_of_centroids == 16 and s.k_factor == 4.0 and s.refine_type == "fp16"
    assert type(RefineFaissSearch(model=None, refine_base="sq", quantizer_type="QT_8bit_uniform").base_search) is SQFaissSearch
    p = RefineFaissSearch(model=None, refine_base="pca", output_dimension=32, eigen_power=-0.5)
    assert type(p.base_search) is PCAFaissSearch and p.base_search.output_dim == 32 and p.base_search.eigen_power == -0.5
    with pytest.raises(NotImplementedError, match="use_rotation"):
        RefineFaissSearch(model=None, refine_base="pq", use_rotation=True)
    with pytest.raises(NotImplementedError, match="QT_8bit"):
        RefineFaissSearch(model=None, refine_base="sq", quantizer_type="QT_8bit")
    with pytest.raises(ValueError, match="output_dimension"):
        RefineFaissSearch(model=None, refine_base="pca")
    with pytest.raises(NotImplementedError, match="random_rotation"):
        RefineFaissSearch(model=None, refine_base="pca", output_dimension=32, random_rotation=True)
    # top_k * k_factor past the rerank's limit is refused before anything is encoded
    with pytest.raises(ValueError, match="2048"):
        RefineFaissSearch(model=None, refine_base="pq", k_factor=3).search({}, {}, top_k=1000)
    with pytest.raises(ValueError, match="2048"):
        RefineFaissSearch(model=None, refine_base="pq", k_factor=3).retrieve_with_emb(None, [], 700)
    # the HybridSearch route
    h = HybridSearch(model=None, batch_size=8, faiss_search_map="refine", refine_base="pq", k_factor=10, refine_type="fp16", num_of_centroids=32,
                     show_progress_bar=False)
    d = h.dense_search
    assert type(d) is RefineFaissSearch and (d.refine_base, d.k_factor, d.refine_type, d.base_search.num_of_centroids) == ("pq", 10.0, "fp16", 32)
    d = HybridSearch(model=None, faiss_search_map="refine", refine_base="pca", output_dimension=64, num_of_centroids=32).dense_search
    assert type(d.base_search) is PCAFaissSearch and d.base_search.output_dim == 64        # (a PQ argument does not reach the PCA searcher)
    d = HybridSearch(model=None, faiss_search_map="refine", refine_base="sq", quantizer_type="QT_8bit_uniform").dense_search
    assert d.base_search.qname == "QT_8bit_uniform"
    with pytest.raises(ValueError, match="refine_base"):
        HybridSearch(model=None, faiss_search_map="refine")
    with pytest.raises(NotImplementedError, match="use_rotation"):
        HybridSearch(model=None, faiss_search_map="refine", refine_base="pq", use_rotation=True)
    # no other map changes
    assert type(HybridSearch(model=None, faiss_search_map="hnsw").dense_search) is FlatIPFaissSearch
    assert type(HybridSearch(model=None, faiss_search_map="hnswsq", refine_base="pq").dense_search) is FlatIPFaissSearch
    assert type(HybridSearch(model=None, faiss_search_map="pq", k_factor=4).dense_search) is PQFaissSearch
    assert type(HybridSearch(model=None).dense_search) is FlatIPFaissSearch
