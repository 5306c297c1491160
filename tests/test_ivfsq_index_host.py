"""CPU: the inverted-file fp16 scalar-quantised index (IVFSQIndex / IVFSQFaissSearch / lrx_ivf_sq_fp16_ip_search) as far as no
GPU is needed -- the numpy yardstick against ivf_yardstick and against fp64, the 'IwSq' file layout, the argument refusals, the HybridSearch and
refine routes, the exported symbols, the argument checks of the C entry points, the workspace and the group size."""
import ctypes
import struct

import numpy as np
import pytest

from lightretriever_amd import _lib, index_io

import ivf_yardstick as IV
import ivfsq_yardstick as Y

FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work


def _fixture(n=300, d=64, nlist=5, Q=4, seed=0):
    """Integer rows, queries and centroids in [-3, 3]: codes exact in fp16, every fp64 sum exact in any order."""
    rng = np.random.default_rng(seed)
    cent = rng.integers(-3, 4, (nlist, d)).astype(np.float32)
    x = rng.integers(-3, 4, (n, d)).astype(np.float32)
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    q = rng.integers(-3, 4, (Q, d)).astype(np.float32)
    return rng, cent, x, cells, row_ids, list_off, q


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
def test_without_residuals_it_is_the_ivf_yardstick_over_the_decoded_rows():
    rng, cent, x, cells, row_ids, list_off, q = _fixture()
    codes = Y.encode(x[row_ids])
    assert codes.dtype == np.float16 and np.array_equal(Y.decode(codes), x[row_ids])
    probes = np.array([[0, 3, 3], [4, -1, 9], [2, 1, 0], [1, 1, 1]])
    got = Y.search(q, codes, list_off, row_ids, probes, None, False, 20, id_base=7)
    assert same(got, IV.search(q, Y.decode(codes), list_off, row_ids, probes, 20, id_base=7))
    rm = np.arange(len(x)) * 3 + 1
    assert same(Y.search(q, codes, list_off, row_ids, probes, None, False, 500, row_map=rm), IV.search(q, Y.decode(codes), list_off, row_ids, probes, 500, row_map=rm))
    assert same(Y.search(q, codes, list_off, None, probes, None, False, 9), IV.search(q, Y.decode(codes), list_off, None, probes, 9))
    assert (Y.search(q, codes, list_off, row_ids, probes, None, False, 8, max_scan_rows=1)[1] == -1).all()
    # d past one 2048-element block, and a d that fills no block
    for d in (2112, 32):
        rng, cent, x, cells, row_ids, list_off, q = _fixture(n=40, d=d, nlist=3, Q=2, seed=d)
        probes = np.array([[0, 1, 2], [2, 2, 0]])
        assert same(Y.search(q, Y.encode(x[row_ids]), list_off, row_ids, probes, None, False, 15), IV.search(q, x[row_ids], list_off, row_ids, probes, 15))


def test_residual_scores_are_the_fp64_product_with_centroid_plus_code_rounded_once():
    rng, cent, x, cells, row_ids, list_off, q = _fixture()
    n, nlist = len(x), len(cent)
    codes = Y.encode(x[row_ids], cent, cells[row_ids])
    assert np.array_equal(Y.decode(codes, cent, cells[row_ids]), x[row_ids])     # integers: the residual and its code are exact
    probes = IV.probe_lists(q, cent, nlist)
    base = np.stack([IV.exact_scores(q[i], cent)[probes[i]] for i in range(len(q))])
    D, I = Y.search(q, codes, list_off, row_ids, probes, base, True, n)
    assert (np.sort(I, axis=1) == np.arange(n)[None, :]).all()                   # every row once
    pos_of = np.argsort(row_ids)
    for i in range(len(q)):
        for r, s in zip(I[i], D[i]):
            full = cent[cells[r]].astype(np.float64) + codes[pos_of[r]].astype(np.float64)
            assert s == np.float32(np.dot(q[i].astype(np.float64), full)), (i, r)
    # hand-given probe scores in quarters stay exact too, and a repeat keeps the base of its first occurrence
    probes = np.array([[2, 2], [1, -1], [9, 3], [0, 4]])
    base = np.array([[1.5, 1e30], [0.25, 1e30], [1e30, -2.75], [0.0, 3.5]], np.float32)
    D, I = Y.search(q, codes, list_off, row_ids, probes, base, True, 500)
    one = Y.search(q, codes, list_off, row_ids, probes[:, :1], base[:, :1], True, 500)
    assert np.array_equal(I[0], one[1][0]) and np.array_equal(D[0], one[0][0]) and np.array_equal(I[1], one[1][1])
    assert D[0, 0] < 1e20 and I[2][I[2] >= 0].size == (cells == 3).sum()
    r = I[3, 0]
    assert D[3, 0] == np.float32((0.0 if cells[r] == 0 else 3.5) + np.dot(q[3].astype(np.float64), codes[pos_of[r]].astype(np.float64)))


def test_codes_round_to_nearest_even_saturate_and_keep_subnormals():
    x = np.array([[1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, 1e9, -1e9, -65520.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                   2.0 ** -14 - 2.0 ** -25, np.inf, -np.inf, np.nan]], np.float32)
    want = np.array([[1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, 65504.0, 65504.0, -65504.0, -65504.0, 2.0 ** -24, 0.0, 2.0 ** -23, 2.0 ** -14, 65504.0,
                      -65504.0, -65504.0]], np.float64)
    got = Y.encode(x)
    assert np.array_equal(got.astype(np.float64), want)
    cent = np.full((2, 16), 0.5, np.float32)
    assert np.array_equal(Y.encode(x[:, :3], cent[:, :3], [1]).astype(np.float32), (x[:, :3] - np.float32(0.5)).astype(np.float16).astype(np.float32))


def test_the_ordered_sum_is_exact_dots_order():
    """On data whose sums are NOT exact the order shows: the yardstick follows lane sub = (e % 128) / 4, blocks of 2048, then the xor tree."""
    rng = np.random.default_rng(5)
    d = 2112
    q = rng.standard_normal(d).astype(np.float32)
    c = rng.standard_normal((3, d)).astype(np.float16)
    p = c.astype(np.float64) * q.astype(np.float64)[None, :]
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
        assert Y.ordered_sums(q, c)[r] == lanes[0]
    assert abs(Y.ordered_sums(q, c)[0] - p[0].sum()) < 1e-10


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def _three_cells(d=32):
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((3, d)).astype(np.float32)
    codes = rng.standard_normal((3, d)).astype(np.float16)
    return cent, [2, 0, 1], codes, np.array([0, 2, 1], np.int64)          # cell 0 holds original rows 0 and 2, cell 1 is empty, cell 2 holds row 1


def test_file_layout_field_by_field(tmp_path):
    d = 32
    cent, sizes, codes, row_ids = _three_cells(d)
    f = str(tmp_path / "a.ivfsq.faiss")
    index_io.write_ivf_sq(f, cent, sizes, codes, row_ids, nprobe=2, by_residual=True)
    b = open(f, "rb").read()
    assert b == Y.file_bytes(cent, sizes, codes, row_ids, nprobe=2, by_residual=True)
    u = lambda fmt, off: struct.unpack_from("<" + fmt, b, off)
    assert u("4siqqqBi", 0) == (b"IwSq", d, 3, 1 << 20, 1 << 20, 1, 0)
    assert u("QQ", 37) == (3, 2)                      # nlist, nprobe
    assert u("4siqqqBi", 53) == (b"IxFI", d, 3, 1 << 20, 1 << 20, 1, 0)
    assert u("Q", 90) == (3 * d,)
    assert np.array_equal(np.frombuffer(b, "<f4", 3 * d, 98), cent.ravel())
    p = 98 + 12 * d
    assert u("BQ", p) == (0, 0)                       # direct map: NoMap, empty vector
    assert u("iifQQ", p + 9) == (4, 0, 0.0, d, 2 * d)  # the ScalarQuantizer: QT_fp16, rangestat, rangestat_arg, d, code_size
    assert u("Q", p + 37) == (0,)                     # its empty `trained`
    assert u("QB", p + 45) == (2 * d, 1)              # code_size, by_residual
    p += 54
    assert u("4sQQ", p) == (b"ilar", 3, 2 * d)
    assert u("4sQQQQ", p + 20) == (b"full", 3, 2, 0, 1)
    p += 56
    assert b[p:p + 4 * d] == codes[:2].tobytes() and u("qq", p + 4 * d) == (0, 2)
    p += 4 * d + 16
    assert b[p:p + 2 * d] == codes[2].tobytes() and u("q", p + 2 * d) == (1,) and len(b) == p + 2 * d + 8
    st = index_io.read_ivf_sq(f)
    assert (st["d"], st["nlist"], st["nprobe"], st["ntotal"], st["is_trained"], st["by_residual"]) == (d, 3, 2, 3, True, True)
    assert np.array_equal(st["centroids"], cent) and st["codes"].dtype == np.float16 and np.array_equal(st["codes"].view(np.int16), codes.view(np.int16))
    assert np.array_equal(st["row_ids"], row_ids) and st["list_off"].tolist() == [0, 2, 2, 3]
    assert index_io.index_record_end(f) == len(b) and index_io.peek_index_header(f) == (b"IwSq", d, 3, True, 0)
    index_io.write_ivf_sq(f, cent, sizes, codes, row_ids, by_residual=False)
    assert open(f, "rb").read() == Y.file_bytes(cent, sizes, codes, row_ids, by_residual=False)
    assert index_io.read_ivf_sq(f)["by_residual"] is False


def test_both_list_size_forms_read_back_and_everything_else_is_refused_by_name(tmp_path):
    cent, sizes, codes, row_ids = _three_cells()
    d = 32
    full = Y.file_bytes(cent, sizes, codes, row_ids, nprobe=2)
    at = full.index(b"full")
    sprs = full[:at] + b"sprs" + struct.pack("<QQQQQ", 4, 0, 2, 2, 1) + full[at + 4 + 8 + 24:]      # a hand-made sparse form of the same sizes
    f = str(tmp_path / "s.ivfsq.faiss")
    open(f, "wb").write(sprs)
    a = index_io.read_ivf_sq(f)
    assert index_io.index_record_end(f) == len(sprs)
    open(f, "wb").write(full)
    b = index_io.read_ivf_sq(f)
    for key in ("centroids", "codes", "row_ids", "list_off"):
        assert np.array_equal(a[key], b[key]), key
    # the writer itself goes sparse when at most half of the cells hold rows, as faiss does (n_non0 > nlist / 2 -> 'full')
    index_io.write_ivf_sq(f, cent, [0, 0, 3], codes, row_ids)
    got = open(f, "rb").read()
    assert got == Y.file_bytes(cent, [0, 0, 3], codes, row_ids) and b"sprs" in got and b"full" not in got
    assert index_io.read_ivf_sq(f)["list_off"].tolist() == [0, 0, 0, 3]

    def refused(data, match):
        open(f, "wb").write(data)
        with pytest.raises(ValueError, match=match):
            index_io.read_ivf_sq(f)
    refused(full[:at] + b"zzzz" + full[at + 4:], "zzzz")                      # another list-size form
    refused(full[:-5], "do not fill")                                         # truncated inside the last cell
    refused(full[:at + 6], "truncated")                                       # truncated inside the head
    refused(full[:60], "truncated|too short")
    refused(b"IwFl" + full[4:], "IwSq")                                       # a wrong fourcc
    p = 98 + 12 * d                                                           # the direct map
    refused(full[:p + 9] + struct.pack("<i", 0) + full[p + 13:], "qtype 0")   # QT_8bit
    refused(full[:p + 9] + struct.pack("<i", 6) + full[p + 13:], "qtype 6")
    refused(full[:p] + struct.pack("<B", 1) + full[p + 1:], "direct map type 1")
    refused(full[:p + 1] + struct.pack("<Q", 3) + full[p + 9:], "direct map type 0 with 3 entries")
    il = full.index(b"ilar")
    refused(full[:il] + b"ilod" + full[il + 4:], "ilod")                      # other inverted lists
    refused(full[:p + 54 - 1] + struct.pack("<B", 2) + full[p + 54:], "by_residual=2")
    with pytest.raises(ValueError, match="row ids"):
        index_io.write_ivf_sq(f, cent, sizes, codes[:2], row_ids)
    with pytest.raises(ValueError, match="float32"):
        index_io.write_ivf_sq(f, cent, sizes, codes.astype(np.float32), row_ids)
    with pytest.raises(ValueError, match="centroids"):
        index_io.write_ivf_sq(f, cent[:2], sizes, codes, row_ids)


def test_an_untrained_index_file_holds_no_centroids_and_a_record_can_follow_a_prefix(tmp_path):
    f = str(tmp_path / "u.ivfsq.faiss")
    index_io.write_ivf_sq(f, np.zeros((0, 32), np.float32), [0, 0], np.zeros((0, 32), np.float16), np.zeros(0, np.int64), is_trained=False)
    st = index_io.read_ivf_sq(f)
    assert st["is_trained"] is False and st["centroids"].shape == (0, 32) and st["ntotal"] == 0 and st["nlist"] == 2
    cent, sizes, codes, row_ids = _three_cells()
    index_io.write_ivf_sq(f, cent, sizes, codes, row_ids, prefix=b"0123456")
    rec = Y.file_bytes(cent, sizes, codes, row_ids)
    open(f, "ab").write(b"tail")
    assert open(f, "rb").read() == b"0123456" + rec + b"tail"
    assert index_io.index_record_end(f, 7) == 7 + len(rec) and index_io.peek_index_header(f, 7)[0] == b"IwSq"
    assert np.array_equal(index_io.read_ivf_sq(f, 7, 7 + len(rec))["codes"], codes)
    with pytest.raises(ValueError):
        index_io.read_ivf_sq(f, 7)                    # the record does not fill the rest of the file


def test_a_refine_file_takes_the_record_as_its_base(tmp_path):
    cent, sizes, codes, row_ids = _three_cells()
    f = str(tmp_path / "r.refine.faiss")
    rows = np.arange(96, dtype=np.float32).reshape(3, 32)
    index_io.write_refine(f, 32, 3, True, 2.5, lambda fn, prefix: index_io.write_ivf_sq(fn, cent, sizes, codes, row_ids, prefix=prefix),
                          lambda fn: index_io.write_flat_ip(fn, [rows], 32, 3, append=True))
    st = index_io.read_refine(f)
    assert st["base"]["fourcc"] == b"IwSq" and st["store"]["fourcc"] == b"IxFI" and st["k_factor"] == 2.5
    assert st["base"]["end"] - st["base"]["offset"] == len(Y.file_bytes(cent, sizes, codes, row_ids))
    assert np.array_equal(index_io.read_ivf_sq(f, st["base"]["offset"], st["base"]["end"])["row_ids"], row_ids)


# ---- refusals and routes -----------------------------------------------------------------------------------------------------------
def test_index_arguments_are_checked_before_the_gpu_is_needed():
    from lightretriever_amd.ivfsq import IVFSQIndex, check_ivfsq_args
    check_ivfsq_args(2048, 1024, "QT_fp16", 32)
    for kw, exc, msg in ((dict(d=64, nlist=4, qtype="QT_8bit"), NotImplementedError, "QT_8bit"), (dict(d=64, nlist=4, qtype="QT_bf16"), NotImplementedError, "QT_bf16"),
                         (dict(d=48, nlist=4), ValueError, "d=48"), (dict(d=8224, nlist=4), ValueError, "d=8224"), (dict(d=0, nlist=4), ValueError, "d=0"),
                         (dict(d=64, nlist=0), ValueError, "nlist=0"), (dict(d=64, nlist=4, nprobe=0), ValueError, "nprobe=0"),
                         (dict(d=64, nlist=4, nprobe=5), ValueError, "nprobe=5"), (dict(d=64, nlist=4096, nprobe=2049), ValueError, "nprobe=2049")):
        with pytest.raises(exc, match=msg):
            IVFSQIndex(**kw)
    with pytest.raises(ValueError, match="IVFSQIndex"):
        check_ivfsq_args(64, 4, "QT_fp16", 9)
    with pytest.raises(NotImplementedError, match="range_search"):
        IVFSQIndex.range_search(IVFSQIndex.__new__(IVFSQIndex), None, 0.0)


def test_searcher_arguments_and_routes():
    import lightretriever.retriever.faiss_search as shim
    import lightretriever_amd
    from lightretriever_amd import refine, torch_ops
    from lightretriever_amd.ivfsq import IVFSQIndex
    from lightretriever_amd.retriever import FlatIPFaissSearch, HybridSearch, IVFSQFaissSearch, RefineFaissSearch
    assert type(HybridSearch(model=None, faiss_search_map="ivfsq", nlist=8).dense_search) is IVFSQFaissSearch
    d = HybridSearch(model=None, batch_size=8, faiss_search_map="ivfsq", nlist=8, nprobe=3, quantizer_type="QT_fp16", by_residual=False, similarity_metric=0,
                     show_progress_bar=False).dense_search
    assert (d.nlist, d.nprobe, d.quantizer_type, d.by_residual, d.similarity_metric) == (8, 3, "QT_fp16", False, 0)
    assert (d.index_ext, d.serves_rpc_shards, d.get_index_name(), d.index_cls) == ("ivfsq", False, "ivfsq_faiss_index", IVFSQIndex)
    assert issubclass(IVFSQFaissSearch, FlatIPFaissSearch)
    d = IVFSQFaissSearch(model=None)
    assert (d.nlist, d.nprobe, d.quantizer_type, d.by_residual) == (1024, 32, "QT_fp16", True)
    r = RefineFaissSearch(model=None, refine_base="ivfsq")
    assert type(r.base_search) is IVFSQFaissSearch
    r = HybridSearch(model=None, faiss_search_map="refine", refine_base="ivfsq", nlist=8, by_residual=False, k_factor=2).dense_search
    assert type(r) is RefineFaissSearch and type(r.base_search) is IVFSQFaissSearch and (r.base_search.nlist, r.base_search.by_residual, r.k_factor) == (8, False, 2.0)
    assert RefineFaissSearch.BASE_SEARCHERS["ivfsq"] is IVFSQFaissSearch and IVFSQIndex in refine.BASES
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        HybridSearch(model=None, faiss_search_map="ivfsq", nlist=8, similarity_metric=1)
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        IVFSQFaissSearch(model=None, similarity_metric="METRIC_L2")
    with pytest.raises(NotImplementedError, match="QT_8bit"):
        IVFSQFaissSearch(model=None, quantizer_type="QT_8bit")
    with pytest.raises(NotImplementedError, match="QT_8bit_uniform"):
        HybridSearch(model=None, faiss_search_map="ivfsq", quantizer_type="QT_8bit_uniform")
    with pytest.raises(ValueError, match="nlist=0"):
        IVFSQFaissSearch(model=None, nlist=0)
    with pytest.raises(ValueError, match="nprobe=0"):
        IVFSQFaissSearch(model=None, nprobe=0)
    assert type(HybridSearch(model=None, faiss_search_map="hnswsq", nlist=8).dense_search) is FlatIPFaissSearch
    assert shim.IVFSQFaissSearch is IVFSQFaissSearch
    assert lightretriever_amd.IVFSQIndex is IVFSQIndex
    assert "ivf_sq_fp16_ip_topk" in torch_ops.OPS


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported():
    l = _lib.lib()
    for name in ("lrx_ivf_sq_fp16_ip_search", "lrx_ivf_sq_fp16_ip_workspace_bytes", "lrx_ivf_sq_fp16_group_rows", "lrx_ivf_sq_fp16_encode_rows"):
        assert callable(getattr(l, name)) and name in _lib.SIGNATURES
    assert l.lrx_abi_version() == 9


def _search(l, codes=FAKE, n_rows=1000, dim=64, nlist=16, n_queries=4, nprobe=4, ld_probe=None, by_residual=1, max_scan=500, k=10, ws_bytes=1 << 30,
            probe_scores=FAKE):
    return l.lrx_ivf_sq_fp16_ip_search(codes, n_rows, dim, FAKE, FAKE, nlist, FAKE, n_queries, FAKE, probe_scores, nprobe, nprobe if ld_probe is None else ld_probe,
                                       by_residual, max_scan, k, 0, FAKE, FAKE, None, FAKE, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [(dict(dim=48), b"dim=48"), (dict(dim=0), b"dim=0"), (dict(dim=8224), b"dim=8224"), (dict(k=0), b"k=0"), (dict(k=2049), b"k=2049"),
                                     (dict(nprobe=0), b"nprobe=0"), (dict(nprobe=17), b"nprobe=17"), (dict(nlist=4096, nprobe=2049), b"nprobe=2049"),
                                     (dict(nprobe=4, ld_probe=3), b"ld_probe=3"), (dict(nlist=0), b"nlist=0"), (dict(max_scan=-1), b"max_scan_rows=-1"),
                                     (dict(max_scan=1 << 31), b"max_scan_rows=2147483648"), (dict(n_rows=1 << 32), b"rows=4294967296"),
                                     (dict(probe_scores=None), b"by_residual=1 needs probe_scores"), (dict(codes=ctypes.c_void_p(264)), b"codes must be 16-byte aligned"),
                                     (dict(n_queries=-1), b"n_queries=-1")])
def test_argument_errors_are_reported_without_a_gpu(kw, msg):
    l = _lib.lib()
    assert _search(l, **kw) == -1, kw                # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert b"ivf_sq_fp16_ip_search" in l.lrx_last_error()


def test_short_workspace_is_refused_and_no_queries_launch_nothing():
    l = _lib.lib()
    assert _search(l, ws_bytes=16) == -3             # LRX_ERR_WORKSPACE
    assert b"workspace" in l.lrx_last_error() and b"ivf_sq_fp16_ip_search" in l.lrx_last_error()
    need = l.lrx_ivf_sq_fp16_ip_workspace_bytes(1000, 16, 64, 4, 4, 10, 500)
    assert _search(l, ws_bytes=need - 1) == -3
    assert _search(l, n_queries=0, ws_bytes=0) == 0
    assert _search(l, n_queries=0, ws_bytes=0, by_residual=0, probe_scores=None) == 0


def test_the_workspace_is_the_flat_entrys_and_the_group_is_64_kib_of_codes():
    l = _lib.lib()
    for args in ((1000, 16, 64, 4, 4, 10, 500), (1 << 20, 1024, 2048, 1000, 128, 100, 200000), (0, 1, 32, 1, 1, 1, 0), (5000, 64, 8192, 5000, 64, 2048, 5000)):
        assert l.lrx_ivf_sq_fp16_ip_workspace_bytes(*args) == l.lrx_ivf_flat_ip_workspace_bytes(*args) > 0
    assert [l.lrx_ivf_sq_fp16_group_rows(d) for d in (32, 256, 2048, 8192)] == [128, 128, 16, 4]
    assert [l.lrx_ivf_sq_fp16_group_rows(d) for d in (288, 4096, 512)] == [113, 8, 64]


def test_encode_arguments_are_checked_without_a_gpu():
    l = _lib.lib()
    enc = lambda x=FAKE, ldx=64, n=10, dim=64, cent=FAKE, cells=FAKE, nlist=4, codes=FAKE, row0=0: l.lrx_ivf_sq_fp16_encode_rows(x, ldx, n, dim, cent, cells, nlist, codes,
                                                                                                                                row0, None)
    for kw, msg in ((dict(dim=48, ldx=48), b"dim=48"), (dict(n=-1), b"out of range"), (dict(row0=(1 << 32) - 5), b"out of range"), (dict(nlist=0), b"nlist=0"),
                    (dict(cells=None), b"centroids need cells"), (dict(ldx=60), b"ldx=60"), (dict(ldx=66), b"ldx=66"), (dict(x=ctypes.c_void_p(260)), b"16-byte aligned"),
                    (dict(x=None), b"null pointer"), (dict(codes=None), b"null pointer")):
        assert enc(**kw) == -1, kw
        assert msg in l.lrx_last_error() and b"ivf_sq_fp16_encode_rows" in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert enc(n=0, x=None, codes=None) == 0
