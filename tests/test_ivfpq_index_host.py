"""CPU: the inverted-file product-quantised index (IVFPQIndex / IVFPQFaissSearch / lrx_ivf_pq_ip_search) as far as no GPU is
needed -- the numpy yardstick against pq_yardstick and against fp64, the 'IwPQ' file layout, the argument refusals, the HybridSearch and refine
routes, the exported symbols, the argument checks of the C entry point and the workspace size."""
import ctypes
import struct

import numpy as np
import pytest

from lightretriever_amd import _lib, index_io

import ivf_yardstick as IV
import ivfpq_yardstick as Y
import pq_yardstick as PQ

FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work


def _fixture(n=300, d=32, M=8, nlist=5, Q=4, seed=0):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = IV.cell_order(cells, nlist)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    return rng, cent, C, codes, cells, row_ids, list_off, q


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
def test_one_cell_without_residuals_is_the_pq_yardstick_bit_for_bit():
    rng, _, C, codes, _, _, _, q = _fixture(M=6, d=48)
    n = len(codes)
    got = Y.search(q, C, codes, [0, n], None, np.zeros((len(q), 1), np.int64), None, False, 20)
    want = PQ.search(q, C, codes, 20)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
    # more than the rows: padding
    got = Y.search(q, C, codes[:7], [0, 7], None, np.zeros((len(q), 1), np.int64), None, False, 10)
    want = PQ.search(q, C, codes[:7], 10)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.int32), want[0].view(np.int32))


def test_residual_scores_are_close_to_the_fp64_inner_product():
    """|score - <q, centroid + decoded residual>| <= (M + 2) 2^-23 (|base| + sum_m |LUT_m|): every table entry and the base carry one
    rounding of 2^-24 relative (M + 1 terms), each of the M adds one more of the partial sum, which the sum of the magnitudes bounds
    (to first order; the factor (1 + 2^-24)^M is far inside the remaining factor of 2): (2 M + 1) 2^-24 <= (M + 2) 2^-23."""
    rng, cent, C, codes, cells, row_ids, list_off, q = _fixture()
    n, M, nlist = len(codes), C.shape[0], len(cent)
    stored = codes                                                            # position p holds original row row_ids[p]
    probes = IV.probe_lists(q, cent, nlist)
    base = np.stack([IV.exact_scores(q[i], cent)[probes[i]] for i in range(len(q))])
    D, I = Y.search(q, C, stored, list_off, row_ids, probes, base, True, n)
    assert (np.sort(I, axis=1) == np.arange(n)[None, :]).all()               # every row once
    L = PQ.lut(q, C).astype(np.float64)
    pos_of = np.argsort(row_ids)
    dec = Y.decode(stored, C).astype(np.float64)
    worst = 0.0
    for i in range(len(q)):
        for r, s in zip(I[i], D[i]):
            p = pos_of[r]
            c = cells[r]
            exact = float(np.dot(q[i].astype(np.float64), cent[c].astype(np.float64) + dec[p]))
            b = float(np.float32(IV.exact_scores(q[i], cent)[c]))
            mag = abs(b) + sum(abs(L[i, m, stored[p, m]]) for m in range(M))
            bound = (M + 2) * 2.0 ** -23 * mag
            worst = max(worst, abs(float(s) - exact) / bound)
            assert abs(float(s) - exact) <= bound, (i, r, float(s), exact, bound)
    print(f"largest |score - fp64| / bound: {worst:.3f}")


def test_a_repeated_cell_keeps_the_base_of_its_first_occurrence_and_bad_entries_are_skipped():
    rng, cent, C, codes, cells, row_ids, list_off, q = _fixture()
    probes = np.array([[2, 2], [1, -1], [9, 3], [0, 4]])
    base = np.array([[1.5, 1e30], [0.25, 1e30], [1e30, -2.0], [0.0, 3.0]], np.float32)
    D, I = Y.search(q, C, codes, list_off, row_ids, probes, base, True, 500)
    one = Y.search(q, C, codes, list_off, row_ids, probes[:, :1], base[:, :1], True, 500)
    assert np.array_equal(I[0], one[1][0]) and np.array_equal(D[0], one[0][0]) and np.array_equal(I[1], one[1][1])
    assert D[0, 0] < 1e20 and (I[2][I[2] >= 0].size == (cells == 3).sum())
    assert (Y.search(q, C, codes, list_off, row_ids, probes, base, True, 8, max_scan_rows=1)[1] == -1).all()
    D7, I7 = Y.search(q, C, codes, list_off, row_ids, probes, base, True, 8, id_base=7)
    assert np.array_equal(I7[I7 >= 0], I[:, :8][I[:, :8] >= 0] + 7)


def test_yardstick_training_is_deterministic_and_uses_residuals():
    x, _ = IV.clustered_corpus(n=600, d=32, n_clusters=12)
    a = Y.train(x, 8, 4, niter=1)
    b = Y.train(x, 8, 4, niter=1)
    assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(a, b))
    assert np.array_equal(a[0].view(np.int32), IV.kmeans(x, 8, 1).view(np.int32))
    r = Y.residuals(x, a[0], IV.assign_cells(x, a[0]))
    assert np.array_equal(a[1].view(np.int32), PQ.kmeans(r, 4, 1).view(np.int32))
    plain = Y.train(x, 8, 4, by_residual=False, niter=1)
    assert np.array_equal(plain[1].view(np.int32), PQ.kmeans(x, 4, 1).view(np.int32))
    with pytest.raises(ValueError):
        Y.train(x[:255], 8, 4)


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def _three_cells(d=32, M=4):
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((3, d)).astype(np.float32)
    C = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, (3, M)).astype(np.uint8)
    return cent, C, [2, 0, 1], codes, np.array([0, 2, 1], np.int64)      # cell 0 holds original rows 0 and 2, cell 1 is empty, cell 2 holds row 1


def test_file_layout_field_by_field(tmp_path):
    d, M = 32, 4
    cent, C, sizes, codes, row_ids = _three_cells(d, M)
    f = str(tmp_path / "a.ivfpq.faiss")
    index_io.write_ivf_pq(f, cent, C, sizes, codes, row_ids, nprobe=2, by_residual=True)
    b = open(f, "rb").read()
    assert b == Y.file_bytes(cent, C, sizes, codes, row_ids, nprobe=2, by_residual=True)
    u = lambda fmt, off: struct.unpack_from("<" + fmt, b, off)
    assert u("4siqqqBi", 0) == (b"IwPQ", d, 3, 1 << 20, 1 << 20, 1, 0)
    assert u("QQ", 37) == (3, 2)                      # nlist, nprobe
    assert u("4siqqqBi", 53) == (b"IxFI", d, 3, 1 << 20, 1 << 20, 1, 0)
    assert u("Q", 90) == (3 * d,)
    p = 98 + 12 * d
    assert u("BQ", p) == (0, 0)                       # direct map: NoMap, empty vector
    assert u("BQ", p + 9) == (1, M)                   # by_residual, code_size
    assert u("QQQQ", p + 18) == (d, M, 8, 256 * d)
    assert np.array_equal(np.frombuffer(b, "<f4", 256 * d, p + 50), C.ravel())
    p += 50 + 1024 * d
    assert u("4sQQ", p) == (b"ilar", 3, M)
    assert u("4sQQQQ", p + 20) == (b"full", 3, 2, 0, 1)
    p += 56
    assert b[p:p + 2 * M] == codes[:2].tobytes() and u("qq", p + 2 * M) == (0, 2)
    p += 2 * M + 16
    assert b[p:p + M] == codes[2].tobytes() and u("q", p + M) == (1,) and len(b) == p + M + 8
    st = index_io.read_ivf_pq(f)
    assert (st["d"], st["nlist"], st["nprobe"], st["ntotal"], st["is_trained"], st["by_residual"], st["M"]) == (d, 3, 2, 3, True, True, M)
    assert np.array_equal(st["centroids"], cent) and np.array_equal(st["pq_centroids"], C) and np.array_equal(st["codes"], codes)
    assert np.array_equal(st["row_ids"], row_ids) and st["list_off"].tolist() == [0, 2, 2, 3]
    assert index_io.index_record_end(f) == len(b) and index_io.peek_index_header(f)[0] == b"IwPQ"
    index_io.write_ivf_pq(f, cent, C, sizes, codes, row_ids, by_residual=False)
    assert open(f, "rb").read() == Y.file_bytes(cent, C, sizes, codes, row_ids, by_residual=False)
    assert index_io.read_ivf_pq(f)["by_residual"] is False


def test_sparse_list_sizes_read_back_and_unknown_forms_are_refused(tmp_path):
    cent, C, sizes, codes, row_ids = _three_cells()
    full = Y.file_bytes(cent, C, sizes, codes, row_ids, nprobe=2)
    at = full.index(b"full")
    sprs = full[:at] + b"sprs" + struct.pack("<QQQQQ", 4, 0, 2, 2, 1) + full[at + 4 + 8 + 24:]      # a hand-made sparse form of the same sizes
    f = str(tmp_path / "s.ivfpq.faiss")
    open(f, "wb").write(sprs)
    a = index_io.read_ivf_pq(f)
    assert index_io.index_record_end(f) == len(sprs)
    open(f, "wb").write(full)
    b = index_io.read_ivf_pq(f)
    for key in ("centroids", "pq_centroids", "codes", "row_ids", "list_off"):
        assert np.array_equal(a[key], b[key]), key
    # the writer itself goes sparse when at most half of the cells hold rows, as faiss does (n_non0 > nlist / 2 -> 'full')
    index_io.write_ivf_pq(f, cent, C, [0, 0, 3], codes, row_ids)
    got = open(f, "rb").read()
    assert got == Y.file_bytes(cent, C, [0, 0, 3], codes, row_ids) and b"sprs" in got and b"full" not in got
    assert index_io.read_ivf_pq(f)["list_off"].tolist() == [0, 0, 0, 3]
    open(f, "wb").write(full[:at] + b"zzzz" + full[at + 4:])
    with pytest.raises(ValueError, match="zzzz"):
        index_io.read_ivf_pq(f)
    open(f, "wb").write(full[:-5])
    with pytest.raises(ValueError):
        index_io.read_ivf_pq(f)
    open(f, "wb").write(b"IwFl" + full[4:])
    with pytest.raises(ValueError, match="IwPQ"):
        index_io.read_ivf_pq(f)
    with pytest.raises(ValueError, match="codebooks"):
        index_io.write_ivf_pq(f, cent, C[:, :100], sizes, codes, row_ids)
    with pytest.raises(ValueError, match="row ids"):
        index_io.write_ivf_pq(f, cent, C, sizes, codes[:2], row_ids)


def test_an_untrained_index_file_holds_no_centroids_and_a_record_can_follow_a_prefix(tmp_path):
    f = str(tmp_path / "u.ivfpq.faiss")
    C = np.zeros((4, 256, 8), np.float32)
    index_io.write_ivf_pq(f, np.zeros((0, 32), np.float32), C, [0, 0], np.zeros((0, 4), np.uint8), np.zeros(0, np.int64), is_trained=False)
    st = index_io.read_ivf_pq(f)
    assert st["is_trained"] is False and st["centroids"].shape == (0, 32) and st["ntotal"] == 0 and st["nlist"] == 2
    cent, C, sizes, codes, row_ids = _three_cells()
    index_io.write_ivf_pq(f, cent, C, sizes, codes, row_ids, prefix=b"0123456")
    rec = Y.file_bytes(cent, C, sizes, codes, row_ids)
    open(f, "ab").write(b"tail")
    assert open(f, "rb").read() == b"0123456" + rec + b"tail"
    assert index_io.index_record_end(f, 7) == 7 + len(rec)
    assert np.array_equal(index_io.read_ivf_pq(f, 7, 7 + len(rec))["codes"], codes)
    with pytest.raises(ValueError):
        index_io.read_ivf_pq(f, 7)                    # the record does not fill the rest of the file


# ---- refusals and routes -----------------------------------------------------------------------------------------------------------
def test_index_arguments_are_checked_before_the_gpu_is_needed():
    from lightretriever_amd.ivfpq import IVFPQIndex, check_ivfpq_args
    check_ivfpq_args(2048, 1024, 128, 8, 32)
    for kw, exc, msg in ((dict(d=64, nlist=4, M=8, nbits=4), NotImplementedError, "nbits=4"), (dict(d=2048, nlist=4, M=16), NotImplementedError, "128 > 64"),
                         (dict(d=64, nlist=4, M=7), ValueError, "M=7"), (dict(d=64, nlist=4, M=0), ValueError, "M=0"),
                         (dict(d=48, nlist=4, M=4), ValueError, "d=48"), (dict(d=8224, nlist=4, M=257), ValueError, "d=8224"),
                         (dict(d=64, nlist=0, M=8), ValueError, "nlist=0"), (dict(d=64, nlist=4, M=8, nprobe=0), ValueError, "nprobe=0"),
                         (dict(d=64, nlist=4, M=8, nprobe=5), ValueError, "nprobe=5"), (dict(d=64, nlist=4096, M=8, nprobe=2049), ValueError, "nprobe=2049")):
        with pytest.raises(exc, match=msg):
            IVFPQIndex(**kw)
    with pytest.raises(ValueError, match="IVFPQIndex"):
        check_ivfpq_args(64, 4, 8, 8, 9)
    with pytest.raises(NotImplementedError, match="range_search"):
        IVFPQIndex.range_search(IVFPQIndex.__new__(IVFPQIndex), None, 0.0)


def test_searcher_arguments_and_routes():
    import lightretriever.retriever.faiss_search as shim
    import lightretriever_amd
    from lightretriever_amd import refine, torch_ops
    from lightretriever_amd.ivfpq import IVFPQIndex
    from lightretriever_amd.retriever import FlatIPFaissSearch, HybridSearch, IVFPQFaissSearch, RefineFaissSearch
    assert type(HybridSearch(model=None, faiss_search_map="ivfpq", nlist=8).dense_search) is IVFPQFaissSearch
    d = HybridSearch(model=None, batch_size=8, faiss_search_map="ivfpq", nlist=8, nprobe=3, num_of_centroids=16, code_size=8, by_residual=False,
                     similarity_metric=0, show_progress_bar=False).dense_search
    assert (d.nlist, d.nprobe, d.num_of_centroids, d.code_size, d.by_residual, d.similarity_metric) == (8, 3, 16, 8, False, 0)
    assert (d.index_ext, d.serves_rpc_shards, d.get_index_name(), d.index_cls) == ("ivfpq", False, "ivfpq_faiss_index", IVFPQIndex)
    assert issubclass(IVFPQFaissSearch, FlatIPFaissSearch)
    d = IVFPQFaissSearch(model=None)
    assert (d.nlist, d.nprobe, d.num_of_centroids, d.code_size, d.by_residual) == (1024, 32, 96, 8, True)
    r = HybridSearch(model=None, faiss_search_map="refine", refine_base="ivfpq", nlist=8, num_of_centroids=4, k_factor=2).dense_search
    assert type(r) is RefineFaissSearch and type(r.base_search) is IVFPQFaissSearch and (r.base_search.nlist, r.base_search.num_of_centroids) == (8, 4)
    assert RefineFaissSearch.BASE_SEARCHERS["ivfpq"] is IVFPQFaissSearch and IVFPQIndex in refine.BASES
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        HybridSearch(model=None, faiss_search_map="ivfpq", nlist=8, similarity_metric=1)
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        IVFPQFaissSearch(model=None, similarity_metric="METRIC_L2")
    with pytest.raises(NotImplementedError, match="code_size"):
        IVFPQFaissSearch(model=None, code_size=4)
    with pytest.raises(ValueError, match="nlist=0"):
        IVFPQFaissSearch(model=None, nlist=0)
    with pytest.raises(ValueError, match="num_of_centroids=0"):
        IVFPQFaissSearch(model=None, num_of_centroids=0)
    assert type(HybridSearch(model=None, faiss_search_map="hnsw", nlist=8).dense_search) is FlatIPFaissSearch
    assert shim.IVFPQFaissSearch is IVFPQFaissSearch
    assert lightretriever_amd.IVFPQIndex is IVFPQIndex
    assert "ivf_pq_ip_topk" in torch_ops.OPS


# ---- the C entry point ------------------------------------------------------------------------------------------------------------
def test_both_symbols_are_exported():
    l = _lib.lib()
    assert callable(l.lrx_ivf_pq_ip_search) and callable(l.lrx_ivf_pq_ip_workspace_bytes)
    assert l.lrx_abi_version() == 9


def _search(l, n_rows=1000, dim=64, M=8, nlist=16, n_queries=4, nprobe=4, ld_probe=None, by_residual=1, max_scan=500, k=10, ws_bytes=1 << 30,
            probe_scores=FAKE):
    return l.lrx_ivf_pq_ip_search(FAKE, n_rows, FAKE, dim, M, FAKE, FAKE, nlist, FAKE, n_queries, FAKE, probe_scores, nprobe,
                                  nprobe if ld_probe is None else ld_probe, by_residual, max_scan, k, 0, FAKE, FAKE, None, FAKE, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [(dict(dim=60), b"dim=60 is not a multiple of M=8"), (dict(nprobe=17), b"nprobe=17"), (dict(k=0), b"k=0"),
                                     (dict(k=2049), b"k=2049"), (dict(nprobe=4, ld_probe=3), b"ld_probe=3"), (dict(M=0), b"M=0"),
                                     (dict(nprobe=0), b"nprobe=0"), (dict(nlist=0), b"nlist=0"), (dict(max_scan=-1), b"max_scan_rows=-1"),
                                     (dict(max_scan=1 << 31), b"max_scan_rows=2147483648"), (dict(n_rows=1 << 32), b"rows=4294967296"),
                                     (dict(probe_scores=None), b"probe_scores")])
def test_argument_errors_are_reported_without_a_gpu(kw, msg):
    l = _lib.lib()
    assert _search(l, **kw) == -1, kw                # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert b"ivf_pq_ip_search" in l.lrx_last_error()


def test_short_workspace_is_refused_and_no_queries_launch_nothing():
    l = _lib.lib()
    assert _search(l, ws_bytes=16) == -3             # LRX_ERR_WORKSPACE
    assert b"workspace" in l.lrx_last_error()
    need = l.lrx_ivf_pq_ip_workspace_bytes(1000, 16, 64, 8, 4, 4, 10, 500)
    assert _search(l, ws_bytes=need - 1) == -3
    assert _search(l, n_queries=0, ws_bytes=0) == 0


def test_workspace_never_decreases_in_the_queries_or_the_scan_bound():
    l = _lib.lib()
    ws = lambda nq, scan=500, nprobe=4, M=8: l.lrx_ivf_pq_ip_workspace_bytes(100000, 64, 128, M, nq, nprobe, 10, scan)
    queries = (0, 1, 2, 7, 64, 95, 96, 97, 500, 1023, 1024, 1025, 5000, 100000)
    scans = (0, 1, 500, 2048, 98303, 98304, 98305, 1 << 20, (1 << 20) + 1, 3 << 20, 100663296, 100663297, (1 << 31) - 1)
    for scan in scans:
        sizes = [ws(nq, scan) for nq in queries]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (scan, sizes)
    for nq in queries:
        sizes = [ws(nq, scan) for scan in scans]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, sizes)
    assert ws(1) < ws(2) < ws(1024) == ws(1025) == ws(100000)         # grows up to the chunk of 1024 queries and stops there
    assert ws(8, 500) < ws(8, 600) and ws(8, 500, 64) > ws(8, 500, 4) and ws(8, 500, 4, 16) > ws(8, 500, 4, 8)
    assert ws(5000, 1 << 20, 32, 128) < (1 << 30)                     # tables of 1024 queries + 768 MiB of score words
    assert ws(1, 0) > 0
