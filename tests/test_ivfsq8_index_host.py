"""CPU: the inverted-file 8-bit scalar-quantised index (IVFSQ8Index / IVFSQ8FaissSearch / lrx_ivf_sq8_ip_search) as far as no
GPU is needed -- the numpy yardstick against ivf_yardstick, against fp64 and against a plain loop, the grid precondition of the GPU tests, the
'IwSq' 8-bit file layout, the argument refusals, the HybridSearch and refine routes, the exported symbols, the argument checks of the four C
entry points, the workspace and the group size."""
import ctypes
import struct

import numpy as np
import pytest

from lightretriever_amd import _lib, index_io

import ivf_yardstick as IV
import ivfsq8_yardstick as Y
import sq8_yardstick as S8

FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work
F32 = np.float32


def grid_trained(d, uniform, rng=None):
    """`trained` whose decoded values lie on a grid (Y.GRID_RANGES): the three ranges mixed across the dimensions, or the middle one for all."""
    if uniform:
        return np.array(Y.GRID_RANGES[1][:2], F32), np.full(d, Y.GRID_RANGES[1][2], F32)
    pick = (np.arange(d) if rng is None else rng.integers(0, 3, d)) % 3
    r = np.array(Y.GRID_RANGES, np.float64)[pick]
    return np.concatenate([r[:, 0], r[:, 1]]).astype(F32), r[:, 2].astype(F32)


def _fixture(n=300, d=64, nlist=5, Q=4, seed=0, uniform=False):
    """Codes at random under a grid range, integer centroids, queries in quarters: every decoded value is a multiple of 1/4 below 2^8, every
    fp64 sum exact in any order."""
    rng = np.random.default_rng(seed)
    trained, _ = grid_trained(d, uniform, rng)
    cent = rng.integers(-3, 4, (nlist, d)).astype(F32)
    codes = rng.integers(0, 256, (n, d)).astype(np.uint8)
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    q = (rng.integers(-12, 13, (Q, d)) / 4.0).astype(F32)
    return rng, trained, cent, codes, cells, row_ids, list_off, q


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [False, True])
def test_without_residuals_it_is_the_ivf_yardstick_over_the_decoded_rows(uniform):
    rng, trained, cent, codes, cells, row_ids, list_off, q = _fixture(uniform=uniform)
    stored = codes[row_ids]
    y = Y.decode(stored, trained)
    probes = np.array([[0, 3, 3], [4, -1, 9], [2, 1, 0], [1, 1, 1]])
    got = Y.search(q, stored, trained, list_off, row_ids, probes, None, False, 20, id_base=7)
    assert same(got, IV.search(q, y, list_off, row_ids, probes, 20, id_base=7))
    rm = np.arange(len(codes)) * 3 + 1
    assert same(Y.search(q, stored, trained, list_off, row_ids, probes, None, False, 500, row_map=rm), IV.search(q, y, list_off, row_ids, probes, 500, row_map=rm))
    assert same(Y.search(q, stored, trained, list_off, None, probes, None, False, 9), IV.search(q, y, list_off, None, probes, 9))
    assert (Y.search(q, stored, trained, list_off, row_ids, probes, None, False, 8, max_scan_rows=1)[1] == -1).all()
    # Gaussian rows under a trained range (sums that are NOT exact), d past one 2048-element block and a d that fills no block
    for d in (2112, 32):
        g = np.random.default_rng(d)
        x, qq = g.standard_normal((40, d)).astype(F32), g.standard_normal((2, d)).astype(F32)
        tr = S8.train(x, uniform)
        cl = g.integers(0, 3, 40)
        ri, lo = IV.cell_order(cl, 3)
        st = Y.encode(x[ri], tr)
        probes = np.array([[0, 1, 2], [2, 2, 0]])
        assert same(Y.search(qq, st, tr, lo, ri, probes, None, False, 15), IV.search(qq, Y.decode(st, tr), lo, ri, probes, 15))


@pytest.mark.parametrize("uniform", [False, True])
def test_residual_scores_are_the_fp64_base_plus_product_rounded_once_on_grid_data(uniform):
    rng, trained, cent, codes, cells, row_ids, list_off, q = _fixture(uniform=uniform)
    n, nlist = len(codes), len(cent)
    stored = codes[row_ids]
    y = Y.decode(stored, trained).astype(np.float64)
    probes = IV.probe_lists(q, cent, nlist)
    base = np.stack([IV.exact_scores(q[i], cent)[probes[i]] for i in range(len(q))])
    D, I = Y.search(q, stored, trained, list_off, row_ids, probes, base, True, n)
    assert (np.sort(I, axis=1) == np.arange(n)[None, :]).all()                   # every row once
    pos_of = np.argsort(row_ids)
    for i in range(len(q)):
        b_of = dict(zip(probes[i].tolist(), base[i].astype(np.float64).tolist()))
        for r, s in zip(I[i], D[i]):
            assert s == F32(b_of[int(cells[r])] + np.dot(q[i].astype(np.float64), y[pos_of[r]])), (i, r)
    # hand-given probe scores in quarters stay exact too, and a repeat keeps the base of its first occurrence
    probes = np.array([[2, 2], [1, -1], [9, 3], [0, 4]])
    base = np.array([[1.5, 1e30], [0.25, 1e30], [1e30, -2.75], [0.0, 3.5]], F32)
    D, I = Y.search(q, stored, trained, list_off, row_ids, probes, base, True, 500)
    one = Y.search(q, stored, trained, list_off, row_ids, probes[:, :1], base[:, :1], True, 500)
    assert np.array_equal(I[0], one[1][0]) and np.array_equal(D[0], one[0][0]) and np.array_equal(I[1], one[1][1])
    assert D[0, 0] < 1e20 and I[2][I[2] >= 0].size == (cells == 3).sum()
    r = I[3, 0]
    assert D[3, 0] == F32((0.0 if cells[r] == 0 else 3.5) + np.dot(q[3].astype(np.float64), y[pos_of[r]]))


def test_the_ordered_sum_is_exact_dots_order():
    """On Gaussian data, whose sums are NOT exact, the order shows: lane sub = (e % 128) / 4, blocks of 2048, then the xor tree."""
    rng = np.random.default_rng(5)
    d = 2112
    q = rng.standard_normal(d).astype(F32)
    y = rng.standard_normal((3, d)).astype(F32)
    p = y.astype(np.float64) * q.astype(np.float64)[None, :]
    for r in range(3):
        lanes = []
        for sub in range(32):
            acc = 0.0
            for b in range(0, d, 2048):
                for u in range(16):
                    i = b + 128 * u + 4 * sub
                    if i < d:
                        acc += ((p[r, i] + p[r, i + 1]) + p[r, i + 2]) + p[r, i + 3]
            lanes.append(acc)
        for o in (16, 8, 4, 2, 1):
            lanes = [lanes[i] + lanes[i ^ o] for i in range(32)]
        assert Y.ordered_sums(q, y)[r] == lanes[0]
        assert Y.row_scores(q, y[r:r + 1], 0.75)[0] == F32(0.75 + lanes[0])
    assert abs(Y.ordered_sums(q, y)[0] - p[0].sum()) < 1e-10
    assert IV.exact_scores(q, y).view(np.int32).tolist() == Y.row_scores(q, y).view(np.int32).tolist()      # the flat index's score of the same rows


def test_the_grid_ranges_decode_every_code_exactly_and_encode_it_back():
    """The precondition of the GPU tests that compare with SQ8Index.search (another order of addition): under these (vmin, vdiff) the decode of
    code c -- three fp32 roundings -- is exactly lo + c * step, and the encode of that value is c."""
    c = np.arange(256, dtype=np.uint8)[:, None]
    for (vmin, vdiff, step), lo in zip(Y.GRID_RANGES, (-32.0, -64.0, -128.0)):
        tr = np.array([vmin, vdiff], F32)
        assert float(tr[0]) == vmin and float(tr[1]) == vdiff                    # the range itself is exact in fp32
        y = S8.decode(c, tr)
        assert np.array_equal(y[:, 0].astype(np.float64), lo + step * np.arange(256))
        assert np.array_equal(S8.encode(y, tr), c)
    tr, step = grid_trained(96, False)
    codes = np.random.default_rng(0).integers(0, 256, (50, 96)).astype(np.uint8)
    y = Y.decode(codes, tr)
    assert np.array_equal(y / step, np.round(y / step)) and np.array_equal(Y.encode(y, tr), codes)
    cent = np.random.default_rng(1).integers(-3, 4, (4, 96)).astype(F32)
    cells = np.random.default_rng(2).integers(0, 4, 50)
    x = Y.decode(codes, tr, cent, cells)                                         # grid + integer centroid: the residual is exact again
    assert np.array_equal(Y.encode(x, tr, cent, cells), codes)


def test_codes_clamp_both_ways_ignore_nan_and_a_bad_cell_is_zeros():
    tr = np.array([-1.0, 0.0, 2.0, 2.0, 0.0, 4.0], F32)                          # vmin ++ vdiff of 3 dimensions; dimension 1 has no width
    x = np.array([[-5.0, 7.0, 2.0], [9.0, -7.0, 6.5], [np.nan, np.nan, np.nan], [0.0, 0.0, 4.0], [1.0, 0.0, 6.0]], F32)
    assert Y.encode(x, tr).tolist() == [[0, 0, 0], [255, 0, 255], [0, 0, 0], [127, 0, 127], [255, 0, 255]]
    assert Y.decode(np.array([[0, 9, 255]], np.uint8), tr)[0].tolist() == [F32(-1) + F32(F32(0.5) / F32(255)) * F32(2), 0.0, F32(2) + F32(F32(255.5) / F32(255)) * F32(4)]
    cent = np.ones((2, 3), F32)
    cells = np.array([0, 1, 2, -1, 2 ** 40])
    got = Y.encode(x, tr, cent, cells)
    assert np.array_equal(got[:2], Y.encode(x[:2] - 1, tr)) and not got[2:].any()
    dec = Y.decode(got, tr, cent, cells)
    assert np.array_equal(dec[:2], (S8.decode(got[:2], tr) + 1).astype(F32)) and not dec[2:].any()
    # the range of the residuals: per dimension and over all elements, NaN ignored
    xx = np.array([[1.0, 5.0], [3.0, np.nan], [2.0, -1.0]], F32)
    c2 = np.array([[1.0, 1.0], [-1.0, -1.0]], F32)
    cl = IV.assign_cells(xx, c2)
    res = xx - c2[cl]
    assert Y.train_range(xx, c2, True, False).tolist() == [np.nanmin(res[:, 0]), np.nanmin(res[:, 1]), np.nanmax(res[:, 0]) - np.nanmin(res[:, 0]),
                                                           np.nanmax(res[:, 1]) - np.nanmin(res[:, 1])]
    assert Y.train_range(xx, c2, True, True).tolist() == [np.nanmin(res), np.nanmax(res) - np.nanmin(res)]
    assert Y.train_range(xx, c2, False, True).tolist() == [-1.0, 6.0]


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def _three_cells(d=32, qtype=0):
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((3, d)).astype(F32)
    codes = rng.integers(0, 256, (3, d)).astype(np.uint8)
    trained = rng.standard_normal(2 * d if qtype == 0 else 2).astype(F32)
    return cent, trained, [2, 0, 1], codes, np.array([0, 2, 1], np.int64)    # cell 0 holds original rows 0 and 2, cell 1 is empty, cell 2 holds row 1


@pytest.mark.parametrize("qtype", [0, 2])
def test_file_layout_field_by_field(tmp_path, qtype):
    d = 32
    cent, trained, sizes, codes, row_ids = _three_cells(d, qtype)
    nt = len(trained)
    f = str(tmp_path / "a.ivfsq8.faiss")
    index_io.write_ivf_sq8(f, cent, trained, qtype, sizes, codes, row_ids, nprobe=2, by_residual=True)
    b = open(f, "rb").read()
    assert b == Y.file_bytes(cent, trained, qtype, sizes, codes, row_ids, nprobe=2, by_residual=True)
    u = lambda fmt, off: struct.unpack_from("<" + fmt, b, off)
    assert u("4siqqqBi", 0) == (b"IwSq", d, 3, 1 << 20, 1 << 20, 1, 0)
    assert u("QQ", 37) == (3, 2)                      # nlist, nprobe
    assert u("4siqqqBi", 53) == (b"IxFI", d, 3, 1 << 20, 1 << 20, 1, 0)
    assert u("Q", 90) == (3 * d,)
    assert np.array_equal(np.frombuffer(b, "<f4", 3 * d, 98), cent.ravel())
    p = 98 + 12 * d
    assert u("BQ", p) == (0, 0)                       # direct map: NoMap, empty vector
    assert u("iifQQ", p + 9) == (qtype, 0, 0.0, d, d)  # the ScalarQuantizer: qtype, rangestat, rangestat_arg, d, code_size
    assert u("Q", p + 37) == (nt,)                    # `trained`: vmin ++ vdiff
    assert np.array_equal(np.frombuffer(b, "<f4", nt, p + 45), trained)
    p += 45 + 4 * nt
    assert u("QB", p) == (d, 1)                       # code_size, by_residual
    p += 9
    assert u("4sQQ", p) == (b"ilar", 3, d)
    assert u("4sQQQQ", p + 20) == (b"full", 3, 2, 0, 1)
    p += 56
    assert b[p:p + 2 * d] == codes[:2].tobytes() and u("qq", p + 2 * d) == (0, 2)
    p += 2 * d + 16
    assert b[p:p + d] == codes[2].tobytes() and u("q", p + d) == (1,) and len(b) == p + d + 8
    st = index_io.read_ivf_sq8(f)
    assert (st["d"], st["nlist"], st["nprobe"], st["ntotal"], st["is_trained"], st["by_residual"], st["qtype"]) == (d, 3, 2, 3, True, True, qtype)
    assert np.array_equal(st["centroids"], cent) and st["codes"].dtype == np.uint8 and np.array_equal(st["codes"], codes) and np.array_equal(st["trained"], trained)
    assert np.array_equal(st["row_ids"], row_ids) and st["list_off"].tolist() == [0, 2, 2, 3]
    assert index_io.index_record_end(f) == len(b) and index_io.peek_index_header(f) == (b"IwSq", d, 3, True, 0) and index_io.ivf_sq_qtype(f) == qtype
    with pytest.raises(ValueError, match=f"qtype {qtype}"):
        index_io.read_ivf_sq(f)                       # the fp16 reader keeps refusing the 8-bit record
    index_io.write_ivf_sq8(f, cent, trained, qtype, sizes, codes, row_ids, by_residual=False)
    assert open(f, "rb").read() == Y.file_bytes(cent, trained, qtype, sizes, codes, row_ids, by_residual=False)
    assert index_io.read_ivf_sq8(f)["by_residual"] is False


def test_both_list_size_forms_read_back_and_everything_else_is_refused_by_name(tmp_path):
    cent, trained, sizes, codes, row_ids = _three_cells()
    d = 32
    full = Y.file_bytes(cent, trained, 0, sizes, codes, row_ids, nprobe=2)
    at = full.index(b"full")
    sprs = full[:at] + b"sprs" + struct.pack("<QQQQQ", 4, 0, 2, 2, 1) + full[at + 4 + 8 + 24:]      # a hand-made sparse form of the same sizes
    f = str(tmp_path / "s.ivfsq8.faiss")
    open(f, "wb").write(sprs)
    a = index_io.read_ivf_sq8(f)
    assert index_io.index_record_end(f) == len(sprs)
    open(f, "wb").write(full)
    b = index_io.read_ivf_sq8(f)
    for key in ("centroids", "trained", "codes", "row_ids", "list_off"):
        assert np.array_equal(a[key], b[key]), key
    # the writer itself goes sparse when at most half of the cells hold rows, as faiss does (n_non0 > nlist / 2 -> 'full')
    index_io.write_ivf_sq8(f, cent, trained, 0, [0, 0, 3], codes, row_ids)
    got = open(f, "rb").read()
    assert got == Y.file_bytes(cent, trained, 0, [0, 0, 3], codes, row_ids) and b"sprs" in got and b"full" not in got
    assert index_io.read_ivf_sq8(f)["list_off"].tolist() == [0, 0, 0, 3]

    def refused(data, match):
        open(f, "wb").write(data)
        with pytest.raises(ValueError, match=match):
            index_io.read_ivf_sq8(f)
    refused(full[:at] + b"zzzz" + full[at + 4:], "zzzz")                      # another list-size form
    refused(full[:-5], "do not fill")                                         # truncated inside the last cell
    refused(full[:at + 6], "truncated")                                       # truncated inside the head
    refused(full[:60], "truncated|too short")
    refused(b"IwFl" + full[4:], "IwSq")                                       # a wrong fourcc
    p = 98 + 12 * d                                                           # the direct map
    refused(full[:p + 9] + struct.pack("<i", 4) + full[p + 13:], "qtype 4.*read_ivf_sq")     # QT_fp16: the other reader's record
    refused(full[:p + 9] + struct.pack("<i", 6) + full[p + 13:], "qtype 6")
    refused(full[:p + 9] + struct.pack("<i", 2) + full[p + 13:], "trained=64")              # QT_8bit_uniform with 2 d trained floats
    refused(full[:p + 37] + struct.pack("<Q", 2) + full[p + 45:], "trained=2")
    refused(full[:p] + struct.pack("<B", 1) + full[p + 1:], "direct map type 1")
    refused(full[:p + 1] + struct.pack("<Q", 3) + full[p + 9:], "direct map type 0 with 3 entries")
    il = full.index(b"ilar")
    refused(full[:il] + b"ilod" + full[il + 4:], "ilod")                      # other inverted lists
    refused(full[:il - 1] + struct.pack("<B", 2) + full[il:], "by_residual=2")
    refused(full[:il - 9] + struct.pack("<Q", 2 * d) + full[il - 1:], "code_size=64")
    open(f, "wb").write(full[:p + 9] + struct.pack("<i", 6) + full[p + 13:])
    assert index_io.ivf_sq_qtype(f) == 6                                      # the peek reports what the file says; the record's length is refused
    with pytest.raises(ValueError, match="qtype 6"):
        index_io.index_record_end(f)
    with pytest.raises(ValueError, match="row ids"):
        index_io.write_ivf_sq8(f, cent, trained, 0, sizes, codes[:2], row_ids)
    with pytest.raises(ValueError, match="float16"):
        index_io.write_ivf_sq8(f, cent, trained, 0, sizes, codes.astype(np.float16), row_ids)
    with pytest.raises(ValueError, match="centroids"):
        index_io.write_ivf_sq8(f, cent[:2], trained, 0, sizes, codes, row_ids)
    with pytest.raises(ValueError, match="trained floats"):
        index_io.write_ivf_sq8(f, cent, trained[:2], 0, sizes, codes, row_ids)
    with pytest.raises(ValueError, match="qtype 4"):
        index_io.write_ivf_sq8(f, cent, trained, 4, sizes, codes, row_ids)


def test_an_untrained_index_file_holds_no_centroids_and_a_record_can_follow_a_prefix(tmp_path):
    f = str(tmp_path / "u.ivfsq8.faiss")
    index_io.write_ivf_sq8(f, np.zeros((0, 32), F32), np.zeros(2, F32), 2, [0, 0], np.zeros((0, 32), np.uint8), np.zeros(0, np.int64), is_trained=False)
    st = index_io.read_ivf_sq8(f)
    assert st["is_trained"] is False and st["centroids"].shape == (0, 32) and st["ntotal"] == 0 and st["nlist"] == 2 and st["qtype"] == 2
    assert index_io.ivf_sq_qtype(f) == 2
    cent, trained, sizes, codes, row_ids = _three_cells()
    index_io.write_ivf_sq8(f, cent, trained, 0, sizes, codes, row_ids, prefix=b"0123456")
    rec = Y.file_bytes(cent, trained, 0, sizes, codes, row_ids)
    open(f, "ab").write(b"tail")
    assert open(f, "rb").read() == b"0123456" + rec + b"tail"
    assert index_io.index_record_end(f, 7) == 7 + len(rec) and index_io.peek_index_header(f, 7)[0] == b"IwSq" and index_io.ivf_sq_qtype(f, 7) == 0
    assert np.array_equal(index_io.read_ivf_sq8(f, 7, 7 + len(rec))["codes"], codes)
    with pytest.raises(ValueError):
        index_io.read_ivf_sq8(f, 7)                   # the record does not fill the rest of the file


def test_a_refine_file_takes_the_record_as_its_base_next_to_the_fp16_one(tmp_path):
    import ivfsq_yardstick as Y16
    cent, trained, sizes, codes, row_ids = _three_cells()
    f = str(tmp_path / "r.refine.faiss")
    rows = np.arange(96, dtype=F32).reshape(3, 32)
    index_io.write_refine(f, 32, 3, True, 2.5, lambda fn, prefix: index_io.write_ivf_sq8(fn, cent, trained, 0, sizes, codes, row_ids, prefix=prefix),
                          lambda fn: index_io.write_flat_ip(fn, [rows], 32, 3, append=True))
    st = index_io.read_refine(f)
    assert st["base"]["fourcc"] == b"IwSq" and st["store"]["fourcc"] == b"IxFI" and st["k_factor"] == 2.5
    assert st["base"]["end"] - st["base"]["offset"] == len(Y.file_bytes(cent, trained, 0, sizes, codes, row_ids))
    assert index_io.ivf_sq_qtype(f, st["base"]["offset"], st["base"]["end"]) == 0
    assert np.array_equal(index_io.read_ivf_sq8(f, st["base"]["offset"], st["base"]["end"])["row_ids"], row_ids)
    with pytest.raises(ValueError, match="qtype 0"):
        index_io.read_ivf_sq(f, st["base"]["offset"], st["base"]["end"])
    # the fp16 record as a base still has its own length and type
    h = codes.astype(np.float16)
    index_io.write_refine(f, 32, 3, True, 1.0, lambda fn, prefix: index_io.write_ivf_sq(fn, cent, sizes, h, row_ids, prefix=prefix),
                          lambda fn: index_io.write_flat_ip(fn, [rows], 32, 3, append=True))
    st = index_io.read_refine(f)
    assert st["base"]["end"] - st["base"]["offset"] == len(Y16.file_bytes(cent, sizes, h, row_ids))
    assert index_io.ivf_sq_qtype(f, st["base"]["offset"], st["base"]["end"]) == 4
    with pytest.raises(ValueError, match="read_ivf_sq"):
        index_io.read_ivf_sq8(f, st["base"]["offset"], st["base"]["end"])


# ---- refusals and routes -----------------------------------------------------------------------------------------------------------
def test_index_arguments_are_checked_before_the_gpu_is_needed():
    from lightretriever_amd.ivfsq8 import IVFSQ8Index, check_ivfsq8_args
    check_ivfsq8_args(2048, 1024, "QT_8bit", 32)
    check_ivfsq8_args(2048, 1024, "QT_8bit_uniform", 32)
    for kw, exc, msg in ((dict(d=64, nlist=4, qtype="QT_fp16"), NotImplementedError, "QT_fp16"), (dict(d=64, nlist=4, qtype="QT_4bit"), NotImplementedError, "QT_4bit"),
                         (dict(d=48, nlist=4), ValueError, "d=48"), (dict(d=8224, nlist=4), ValueError, "d=8224"), (dict(d=0, nlist=4), ValueError, "d=0"),
                         (dict(d=64, nlist=0), ValueError, "nlist=0"), (dict(d=64, nlist=4, nprobe=0), ValueError, "nprobe=0"),
                         (dict(d=64, nlist=4, nprobe=5), ValueError, "nprobe=5"), (dict(d=64, nlist=4096, nprobe=2049), ValueError, "nprobe=2049")):
        with pytest.raises(exc, match=msg):
            IVFSQ8Index(**kw)
    with pytest.raises(ValueError, match="IVFSQ8Index"):
        check_ivfsq8_args(64, 4, "QT_8bit", 9)
    with pytest.raises(NotImplementedError, match="range_search"):
        IVFSQ8Index.range_search(IVFSQ8Index.__new__(IVFSQ8Index), None, 0.0)


def test_searcher_arguments_and_routes():
    import lightretriever.retriever.faiss_search as shim
    import lightretriever_amd
    from lightretriever_amd import refine, torch_ops
    from lightretriever_amd.ivfsq import IVFSQIndex
    from lightretriever_amd.ivfsq8 import IVFSQ8Index
    from lightretriever_amd.retriever import FlatIPFaissSearch, HybridSearch, IVFSQ8FaissSearch, IVFSQFaissSearch, RefineFaissSearch
    assert type(HybridSearch(model=None, faiss_search_map="ivfsq8", nlist=8).dense_search) is IVFSQ8FaissSearch
    d = HybridSearch(model=None, batch_size=8, faiss_search_map="ivfsq8", nlist=8, nprobe=3, quantizer_type="QT_8bit_uniform", by_residual=False,
                     similarity_metric=0, show_progress_bar=False).dense_search
    assert (d.nlist, d.nprobe, d.quantizer_type, d.by_residual, d.similarity_metric) == (8, 3, "QT_8bit_uniform", False, 0)
    assert (d.index_ext, d.serves_rpc_shards, d.get_index_name(), d.index_cls) == ("ivfsq8", False, "ivfsq8_faiss_index", IVFSQ8Index)
    assert issubclass(IVFSQ8FaissSearch, FlatIPFaissSearch)
    d = IVFSQ8FaissSearch(model=None)
    assert (d.nlist, d.nprobe, d.quantizer_type, d.by_residual) == (1024, 32, "QT_8bit", True)
    r = RefineFaissSearch(model=None, refine_base="ivfsq8")
    assert type(r.base_search) is IVFSQ8FaissSearch
    r = HybridSearch(model=None, faiss_search_map="refine", refine_base="ivfsq8", nlist=8, by_residual=False, quantizer_type="QT_8bit_uniform", k_factor=2).dense_search
    assert type(r) is RefineFaissSearch and type(r.base_search) is IVFSQ8FaissSearch
    assert (r.base_search.nlist, r.base_search.by_residual, r.base_search.quantizer_type, r.k_factor) == (8, False, "QT_8bit_uniform", 2.0)
    assert RefineFaissSearch.BASE_SEARCHERS["ivfsq8"] is IVFSQ8FaissSearch and IVFSQ8Index in refine.BASES and IVFSQIndex in refine.BASES
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        HybridSearch(model=None, faiss_search_map="ivfsq8", nlist=8, similarity_metric=1)
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        IVFSQ8FaissSearch(model=None, similarity_metric="METRIC_L2")
    with pytest.raises(NotImplementedError, match="QT_fp16.*IVFSQFaissSearch"):
        IVFSQ8FaissSearch(model=None, quantizer_type="QT_fp16")
    with pytest.raises(NotImplementedError, match="QT_4bit"):
        HybridSearch(model=None, faiss_search_map="ivfsq8", quantizer_type="QT_4bit")
    with pytest.raises(ValueError, match="nlist=0"):
        IVFSQ8FaissSearch(model=None, nlist=0)
    with pytest.raises(ValueError, match="nprobe=0"):
        IVFSQ8FaissSearch(model=None, nprobe=0)
    # the fp16 names keep refusing the 8-bit types, and the unserved maps keep falling back to flat
    with pytest.raises(NotImplementedError, match="QT_8bit"):
        IVFSQFaissSearch(model=None, quantizer_type="QT_8bit")
    with pytest.raises(NotImplementedError, match="QT_8bit"):
        IVFSQIndex(64, 4, qtype="QT_8bit")
    assert type(HybridSearch(model=None, faiss_search_map="hnswsq", nlist=8).dense_search) is FlatIPFaissSearch
    assert type(HybridSearch(model=None, faiss_search_map="hnsw").dense_search) is FlatIPFaissSearch
    assert shim.IVFSQ8FaissSearch is IVFSQ8FaissSearch
    assert lightretriever_amd.IVFSQ8Index is IVFSQ8Index
    assert "ivf_sq8_ip_topk" in torch_ops.OPS


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported():
    l = _lib.lib()
    for name in ("lrx_ivf_sq8_ip_search", "lrx_ivf_sq8_ip_workspace_bytes", "lrx_ivf_sq8_group_rows", "lrx_ivf_sq8_encode_rows", "lrx_ivf_sq8_decode_rows"):
        assert callable(getattr(l, name)) and name in _lib.SIGNATURES
    assert l.lrx_abi_version() == 9


def _search(l, codes=FAKE, n_rows=1000, dim=64, trained=FAKE, qtype=0, nlist=16, n_queries=4, nprobe=4, ld_probe=None, by_residual=1, max_scan=500, k=10,
            ws_bytes=1 << 30, probe_scores=FAKE):
    return l.lrx_ivf_sq8_ip_search(codes, n_rows, dim, trained, qtype, FAKE, FAKE, nlist, FAKE, n_queries, FAKE, probe_scores, nprobe,
                                   nprobe if ld_probe is None else ld_probe, by_residual, max_scan, k, 0, FAKE, FAKE, None, FAKE, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [(dict(dim=48), b"dim=48"), (dict(dim=0), b"dim=0"), (dict(dim=8224), b"dim=8224"), (dict(k=0), b"k=0"), (dict(k=2049), b"k=2049"),
                                     (dict(nprobe=0), b"nprobe=0"), (dict(nprobe=17), b"nprobe=17"), (dict(nlist=4096, nprobe=2049), b"nprobe=2049"),
                                     (dict(nprobe=4, ld_probe=3), b"ld_probe=3"), (dict(nlist=0), b"nlist=0"), (dict(max_scan=-1), b"max_scan_rows=-1"),
                                     (dict(max_scan=1 << 31), b"max_scan_rows=2147483648"), (dict(n_rows=1 << 32), b"rows=4294967296"),
                                     (dict(probe_scores=None), b"by_residual=1 needs probe_scores"), (dict(codes=ctypes.c_void_p(264)), b"codes must be 16-byte aligned"),
                                     (dict(n_queries=-1), b"n_queries=-1"), (dict(qtype=4), b"qtype=4"), (dict(qtype=1), b"qtype=1"), (dict(qtype=-1), b"qtype=-1"),
                                     (dict(trained=None), b"trained"), (dict(trained=ctypes.c_void_p(260)), b"trained")])
def test_argument_errors_are_reported_without_a_gpu(kw, msg):
    l = _lib.lib()
    assert _search(l, **kw) == -1, kw                # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert b"ivf_sq8_ip_search" in l.lrx_last_error()


def test_short_workspace_is_refused_and_no_queries_launch_nothing():
    l = _lib.lib()
    assert _search(l, ws_bytes=16) == -3             # LRX_ERR_WORKSPACE
    assert b"workspace" in l.lrx_last_error() and b"ivf_sq8_ip_search" in l.lrx_last_error()
    need = l.lrx_ivf_sq8_ip_workspace_bytes(1000, 16, 64, 4, 4, 10, 500)
    assert _search(l, ws_bytes=need - 1) == -3
    assert _search(l, n_queries=0, ws_bytes=0) == 0
    assert _search(l, n_queries=0, ws_bytes=0, by_residual=0, probe_scores=None, qtype=2) == 0


def test_the_workspace_is_the_flat_entrys_and_the_group_is_64_kib_of_decoded_rows():
    l = _lib.lib()
    for args in ((1000, 16, 64, 4, 4, 10, 500), (1 << 20, 1024, 2048, 1000, 128, 100, 200000), (0, 1, 32, 1, 1, 1, 0), (5000, 64, 8192, 5000, 64, 2048, 5000)):
        assert l.lrx_ivf_sq8_ip_workspace_bytes(*args) == l.lrx_ivf_flat_ip_workspace_bytes(*args) > 0
    assert [l.lrx_ivf_sq8_group_rows(d) for d in (32, 256, 2048, 8192)] == [128, 64, 8, 2]
    assert [l.lrx_ivf_sq8_group_rows(d) for d in (288, 4096, 512, 0)] == [56, 4, 32, 0]


def test_encode_and_decode_arguments_are_checked_without_a_gpu():
    l = _lib.lib()
    enc = lambda x=FAKE, ldx=64, n=10, dim=64, cent=FAKE, cells=FAKE, nlist=4, trained=FAKE, qtype=0, codes=FAKE, row0=0: l.lrx_ivf_sq8_encode_rows(
        x, ldx, n, dim, cent, cells, nlist, trained, qtype, codes, row0, None)
    for kw, msg in ((dict(dim=48, ldx=48), b"dim=48"), (dict(n=-1), b"out of range"), (dict(row0=(1 << 32) - 5), b"out of range"), (dict(nlist=0), b"nlist=0"),
                    (dict(cells=None), b"centroids need cells"), (dict(ldx=60), b"ldx=60"), (dict(ldx=66), b"ldx=66"), (dict(x=ctypes.c_void_p(260)), b"16-byte aligned"),
                    (dict(x=None), b"null pointer"), (dict(codes=None), b"null pointer"), (dict(trained=None), b"null pointer"), (dict(qtype=4), b"qtype=4"),
                    (dict(qtype=3), b"qtype=3")):
        assert enc(**kw) == -1, kw
        assert msg in l.lrx_last_error() and b"ivf_sq8_encode_rows" in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert enc(n=0, x=None, codes=None) == 0
    dec = lambda codes=FAKE, row0=0, n=10, dim=64, trained=FAKE, qtype=0, cent=FAKE, cells=FAKE, nlist=4, out=FAKE, ldo=64: l.lrx_ivf_sq8_decode_rows(
        codes, row0, n, dim, trained, qtype, cent, cells, nlist, out, ldo, None)
    for kw, msg in ((dict(dim=48, ldo=48), b"dim=48"), (dict(n=-1), b"out of range"), (dict(row0=(1 << 32) - 5), b"out of range"), (dict(nlist=0), b"nlist=0"),
                    (dict(cells=None), b"centroids need cells"), (dict(ldo=60), b"ldo=60"), (dict(codes=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(trained=None), b"null pointer"), (dict(qtype=4), b"qtype=4"), (dict(codes=ctypes.c_void_p(258)), b"4-byte aligned")):
        assert dec(**kw) == -1, kw
        assert msg in l.lrx_last_error() and b"ivf_sq8_decode_rows" in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert dec(n=0, codes=None, out=None) == 0
