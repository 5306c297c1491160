"""CPU side of the 8-bit scalar-quantised index: the IxSQ file layout for QT_8bit / QT_8bit_uniform (index_io), SQFaissSearch's and
HybridSearch's arguments, the self-checks of the numpy yardstick (tests/sq8_yardstick.py) and the scratch-free ISA of the new kernels."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from lightretriever_amd import index_io

import sq8_yardstick as Y

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "lightretriever_amd", "csrc", "lrx_search.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def sample(d=64, n=5, uniform=False, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n + 20, d)).astype(np.float32)
    trained = Y.train(x, uniform)
    return trained, Y.encode(x[:n], trained)


@pytest.mark.parametrize("uniform", [False, True])
def test_ixsq_8bit_bytes_and_field_order(tmp_path, uniform):
    d, n = 64, 5
    qt = 2 if uniform else 0
    trained, codes = sample(d, n, uniform)
    nt = 2 if uniform else 2 * d
    assert trained.size == nt
    path = tmp_path / "a.sq.faiss"
    index_io.write_sq8(str(path), trained, [codes[:2], codes[2:]], d, n, qt)
    b = path.read_bytes()
    assert b[:4] == b"IxSQ"
    assert struct.unpack_from("<iqqqBi", b, 4) == (d, n, 1 << 20, 1 << 20, 1, 0)       # the IxFI index header
    assert struct.unpack_from("<iifQQ", b, 37) == (qt, 0, 0.0, d, d)                   # qtype, rangestat, arg, d, code_size
    assert struct.unpack_from("<Q", b, 65) == (nt,)
    assert np.array_equal(np.frombuffer(b[73:73 + 4 * nt], dtype="<f4"), trained)
    assert struct.unpack_from("<Q", b, 73 + 4 * nt) == (n * d,)
    assert len(b) == 37 + 28 + 8 + 4 * nt + 8 + n * d
    assert np.array_equal(np.frombuffer(b[81 + 4 * nt:], dtype=np.uint8).reshape(n, d), codes)
    q2, t2, c2, is_trained = index_io.read_sq8(str(path))
    assert q2 == qt and is_trained and np.array_equal(t2, trained) and np.array_equal(c2, codes)
    assert index_io.sq_qtype(str(path)) == qt
    index_io.write_sq8(str(path), trained, [codes], d, n, qt, is_trained=False)
    assert index_io.read_sq8(str(path))[3] is False                                     # header is_trained honoured


def test_ixsq_8bit_rejects_bad_files(tmp_path):
    d, n = 64, 4
    trained, codes = sample(d, n)
    path = tmp_path / "a"
    index_io.write_sq8(str(path), trained, [codes], d, n, 0)
    b = path.read_bytes()
    bad = tmp_path / "b"
    for cut in (b[:-1], b[:70], b[:40], b[:73 + 8 * d + 3]):
        bad.write_bytes(cut)
        with pytest.raises(ValueError):
            index_io.read_sq8(str(bad))
    bad.write_bytes(b"IxFI" + b[4:])
    with pytest.raises(ValueError, match="IxSQ"):
        index_io.read_sq8(str(bad))
    with pytest.raises(ValueError, match="IxSQ"):
        index_io.sq_qtype(str(bad))
    for qt in (1, 3, 4):                                                               # 4-bit, 4-bit uniform, fp16
        b2 = bytearray(b)
        struct.pack_into("<i", b2, 37, qt)
        bad.write_bytes(bytes(b2))
        with pytest.raises(ValueError, match="qtype"):
            index_io.read_sq8(str(bad))
        assert index_io.sq_qtype(str(bad)) == qt
    b2 = bytearray(b)
    struct.pack_into("<i", b2, 37, 2)                                                  # uniform header over a per-dimension `trained`
    bad.write_bytes(bytes(b2))
    with pytest.raises(ValueError):
        index_io.read_sq8(str(bad))
    with pytest.raises(ValueError, match="qtype"):                                     # the fp16 reader keeps refusing 8-bit files
        index_io.read_sq_fp16(str(path))
    with pytest.raises(ValueError):
        index_io.write_sq8(str(bad), trained[:5], [codes], d, n, 0)
    with pytest.raises(ValueError):
        index_io.write_sq8(str(bad), trained, [codes], d, n, 1)
    # a QT_fp16 file is told apart by sq_qtype
    index_io.write_sq_fp16(str(bad), [np.ones((2, d), np.float16)], d, 2)
    assert index_io.sq_qtype(str(bad)) == index_io.QT_FP16


def test_sq_faiss_search_accepts_the_uniform_8bit_quantizer():
    from lightretriever_amd import SQ8Index, SQFp16Index
    from lightretriever_amd.retriever import HybridSearch, SQFaissSearch
    s = SQFaissSearch(model=None, batch_size=8, quantizer_type="QT_8bit_uniform")
    assert s.qname == "QT_8bit_uniform" and s.get_index_name() == "sq_faiss_index" and s.index_ext == "sq" and s.index_cls is SQ8Index
    assert SQFaissSearch(model=None).index_cls is SQFp16Index
    with pytest.raises(NotImplementedError, match="QT_4bit"):
        SQFaissSearch(model=None, quantizer_type="QT_4bit")
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        SQFaissSearch(model=None, quantizer_type="QT_8bit_uniform", similarity_metric=1)
    h = HybridSearch(model=None, batch_size=8, faiss_search_map="sq", quantizer_type="QT_8bit_uniform", show_progress_bar=False)
    assert isinstance(h.dense_search, SQFaissSearch) and h.dense_search.qname == "QT_8bit_uniform" and h.dense_search.index_cls is SQ8Index
    assert HybridSearch(model=None, batch_size=8, faiss_search_map="sq").dense_search.qname == "QT_fp16"
    with pytest.raises(NotImplementedError, match="QT_6bit"):
        HybridSearch(model=None, faiss_search_map="sq", quantizer_type="QT_6bit")


def test_sq8_index_arguments_need_no_gpu_to_be_refused():
    from lightretriever_amd import SQ8Index
    with pytest.raises(NotImplementedError, match="QT_4bit"):
        SQ8Index(64, "QT_4bit")
    with pytest.raises(ValueError, match="multiple of 64"):
        SQ8Index(96)


def normalised(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("uniform", [False, True])
def test_yardstick_reconstruction_error_bound(uniform):
    """Truncation to 255 levels, reconstruction at the cell centre: for rows inside the trained range
    |x - decode(encode(x))| <= vdiff (1 / 510 + 2^-20) + 2^-22 max |x| per dimension."""
    x = normalised(20_000, 256, 1)
    trained = Y.train(x, uniform)
    vmin, vdiff = Y._split(trained, 256)
    assert np.array_equal(vmin, np.broadcast_to(x.min() if uniform else x.min(axis=0), (256,)))
    assert np.array_equal(vdiff, np.broadcast_to((x.max() - x.min()) if uniform else (x.max(axis=0) - x.min(axis=0)), (256,)).astype(np.float32))
    codes = Y.encode(x, trained)
    assert codes.dtype == np.uint8 and codes.min() == 0 and codes.max() == 255
    err = np.abs(x.astype(np.float64) - Y.decode(codes, trained).astype(np.float64)).max(axis=0)
    bound = vdiff.astype(np.float64) * (1 / 510 + 2.0 ** -20) + 2.0 ** -22 * np.abs(x).max()
    print("worst error / bound:", float((err / bound).max()))
    assert (err <= bound).all()


def test_yardstick_edge_cases():
    d = 64
    x = normalised(100, d, 2)
    x[:, 3] = 0.25                                                                     # a constant dimension: vdiff = 0
    x[5, 7] = np.nan                                                                   # ignored by train, code 0
    trained = Y.train(x)
    assert not np.isnan(trained).any() and trained[d + 3] == 0
    clean = np.delete(x[:, 7], 5)
    assert trained[7] == clean.min() and trained[d + 7] == np.float32(clean.max() - clean.min())
    codes = Y.encode(x, trained)
    assert (codes[:, 3] == 0).all() and codes[5, 7] == 0
    assert (Y.decode(codes, trained)[:, 3] == np.float32(0.25)).all()                  # exact reconstruction
    out = np.stack([trained[:d] - 1.0, trained[:d] + trained[d:] + 1.0]).astype(np.float32)
    c = Y.encode(out, trained)
    assert (c[0] == 0).all() and (np.delete(c[1], 3) == 255).all() and c[1, 3] == 0    # clamping outside the range
    # the order of the rows does not matter, and neither does the sign of a zero
    assert np.array_equal(Y.train(x[::-1]), trained)
    z = np.zeros((2, d), np.float32)
    z[1] = -0.0
    assert not np.signbit(Y.train(z)).any()
    nan_col = x.copy()
    nan_col[:, 9] = np.nan                                                             # no training value: vmin = vdiff = 0, code 0, decoded 0
    t9 = Y.train(nan_col)
    assert t9[9] == 0 and t9[d + 9] == 0 and (Y.encode(x, t9)[:, 9] == 0).all() and (Y.decode(Y.encode(x, t9), t9)[:, 9] == 0).all()
    assert (Y.train(np.full((2, d), np.nan, np.float32), True) == 0).all()
    with pytest.raises(ValueError):
        Y.train(np.zeros((0, d), np.float32))
    # scores and top-k: ties to the lower row, padding
    q = normalised(3, d, 3)
    dup = np.concatenate([codes[:4], codes[:4]])
    D, I = Y.search(q, dup, trained, 10)
    assert (I[:, 8:] == -1).all() and (D[:, 8:] == -np.finfo(np.float32).max).all()
    assert (I[:, 0:8:2] + 4 == I[:, 1:8:2]).all() and (D[:, 0:8:2] == D[:, 1:8:2]).all()


@pytest.fixture(scope="module")
def search_isa():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "s.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def test_sq8_kernels_have_no_scratch_and_use_the_i8_mfma(search_isa):
    """The kernel descriptors (the metadata hipcc emits) say: no private segment, no spilled register; the scan's text holds the i8 MFMA."""
    desc = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", search_isa, re.S):
        name = re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)
        if "k_sq8_" in name:
            desc[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(0)).group(1))
                          for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    for k in ("k_sq8_minmax", "k_sq8_encode", "k_sq8_decode", "k_sq8_prep", "k_sq8_select_rescore"):
        assert sum(k in n for n in desc) == 1, (k, sorted(desc))
    scans = [n for n in desc if "k_sq8_scan" in n]
    assert len(scans) == 4 and len(desc) == 9                                          # 1, 2, 4, 8 query tiles
    for name, d in desc.items():
        assert d == {"private_segment_fixed_size": 0, "vgpr_spill_count": 0, "sgpr_spill_count": 0}, (name, d)
    for name in scans:
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), search_isa, re.S | re.M).group(0)
        assert "v_mfma_i32_16x16x64_i8" in body and "scratch_" not in body, name
