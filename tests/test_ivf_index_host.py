"""CPU: the inverted-file flat index (IVFFlatIndex / IVFFaissSearch / lrx_ivf_flat_ip_search) as far as no GPU is needed -- the
HybridSearch route, the exported symbols, the argument checks of the C entry point, the workspace size, the 'IwFl' file layout and the numpy
yardstick's own sanity."""
import ctypes
import struct

import numpy as np
import pytest

from lightretriever_amd import _lib, index_io

import ivf_yardstick as Y

FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work


# ---- the route --------------------------------------------------------------------------------------------------------------------
def test_hybrid_search_routes_ivf_to_the_ivf_searcher():
    from lightretriever_amd.ivf import IVFFlatIndex
    from lightretriever_amd.retriever import FlatIPFaissSearch, HybridSearch, IVFFaissSearch
    assert type(HybridSearch(model=None, faiss_search_map="ivf", nlist=8).dense_search) is IVFFaissSearch
    d = HybridSearch(model=None, batch_size=8, faiss_search_map="ivf", nlist=8, nprobe=3, similarity_metric=0, show_progress_bar=False).dense_search
    assert (d.nlist, d.nprobe, d.similarity_metric) == (8, 3, 0)
    assert (d.index_ext, d.serves_rpc_shards, d.get_index_name(), d.index_cls) == ("ivf", False, "ivf_faiss_index", IVFFlatIndex)
    assert issubclass(IVFFaissSearch, FlatIPFaissSearch)
    d = IVFFaissSearch(model=None)
    assert (d.nlist, d.nprobe) == (1024, 32)


def test_a_metric_other_than_inner_product_is_refused():
    from lightretriever_amd.retriever import HybridSearch, IVFFaissSearch
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        HybridSearch(model=None, faiss_search_map="ivf", nlist=8, similarity_metric=1)
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        IVFFaissSearch(model=None, similarity_metric="METRIC_L2")


def test_hnsw_is_still_served_flat():
    from lightretriever_amd.retriever import FlatIPFaissSearch, HybridSearch
    assert type(HybridSearch(model=None, faiss_search_map="hnsw", nlist=8).dense_search) is FlatIPFaissSearch
    assert type(HybridSearch(model=None, faiss_search_map="hnswsq").dense_search) is FlatIPFaissSearch


def test_exports_and_shim():
    import lightretriever.retriever.faiss_search as shim
    import lightretriever_amd
    from lightretriever_amd import torch_ops
    from lightretriever_amd.retriever import IVFFaissSearch
    assert shim.IVFFaissSearch is IVFFaissSearch
    assert lightretriever_amd.IVFFlatIndex.__name__ == "IVFFlatIndex"
    assert "ivf_flat_ip_topk" in torch_ops.OPS


def test_index_arguments_are_checked_before_the_gpu_is_needed():
    from lightretriever_amd.ivf import IVFFlatIndex
    for kw, msg in ((dict(d=48, nlist=4), "d=48"), (dict(d=16, nlist=4), "d=16"), (dict(d=8224, nlist=4), "d=8224"), (dict(d=64, nlist=0), "nlist=0"),
                    (dict(d=64, nlist=4, nprobe=0), "nprobe=0"), (dict(d=64, nlist=4, nprobe=5), "nprobe=5"),
                    (dict(d=64, nlist=4096, nprobe=2049), "nprobe=2049")):
        with pytest.raises(ValueError, match=msg):
            IVFFlatIndex(**kw)
    with pytest.raises(NotImplementedError, match="range_search"):
        IVFFlatIndex.range_search(IVFFlatIndex.__new__(IVFFlatIndex), None, 0.0)


# ---- the C entry point ------------------------------------------------------------------------------------------------------------
def test_both_symbols_are_exported():
    l = _lib.lib()
    assert callable(l.lrx_ivf_flat_ip_search) and callable(l.lrx_ivf_flat_ip_workspace_bytes)
    assert l.lrx_abi_version() == 9


def _search(l, n_rows=1000, dim=64, nlist=16, n_queries=4, nprobe=4, ld_probe=None, max_scan=500, k=10, ws_bytes=1 << 30, ldx=None):
    return l.lrx_ivf_flat_ip_search(FAKE, n_rows, dim if ldx is None else ldx, dim, FAKE, FAKE, nlist, FAKE, n_queries, FAKE, nprobe,
                                    nprobe if ld_probe is None else ld_probe, max_scan, k, 0, FAKE, FAKE, None, FAKE, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [(dict(dim=7), b"dim=7"), (dict(k=0), b"k=0"), (dict(k=2049), b"k=2049"), (dict(nprobe=0), b"nprobe=0"),
                                     (dict(nprobe=4, ld_probe=3), b"ld_probe=3"), (dict(nlist=0), b"nlist=0"), (dict(nprobe=17), b"nprobe=17"),
                                     (dict(dim=8224), b"dim=8224"), (dict(max_scan=-1), b"max_scan_rows=-1"), (dict(n_rows=1 << 32), b"rows=4294967296"),
                                     (dict(ldx=60), b"ldx=60")])
def test_argument_errors_are_reported_without_a_gpu(kw, msg):
    l = _lib.lib()
    assert _search(l, **kw) == -1, kw                # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())


def test_short_workspace_is_refused_and_no_queries_launch_nothing():
    l = _lib.lib()
    assert _search(l, ws_bytes=16) == -3             # LRX_ERR_WORKSPACE
    assert b"workspace" in l.lrx_last_error()
    assert _search(l, n_queries=0, ws_bytes=0) == 0


def test_workspace_grows_with_the_queries_up_to_the_chunk_and_stops_there():
    l = _lib.lib()
    ws = lambda nq, scan=500, nprobe=4: l.lrx_ivf_flat_ip_workspace_bytes(100000, 64, 128, nq, nprobe, 10, scan)
    sizes = [ws(nq) for nq in (1, 2, 7, 64, 500, 1024)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert ws(1024) == ws(1025) == ws(100000)        # the chunk: 1024 queries
    # a large scan bound shrinks the chunk so that the score words stay under 768 MiB: 768 Mi / (8 * 1 Mi) = 96 queries
    big = [ws(nq, 1 << 20) for nq in (1, 95, 96, 97, 5000)]
    assert big[0] < big[1] < big[2] == big[3] == big[4] < (1 << 30)
    assert ws(1, 0) > 0 and ws(0) == ws(1)
    assert ws(8, 500, 8) > ws(8, 500, 4)


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def _three_cells(d=32):
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((3, d)).astype(np.float32)
    rows = rng.standard_normal((3, d)).astype(np.float32)
    return cent, [2, 0, 1], rows, np.array([0, 2, 1], np.int64)      # cell 0 holds original rows 0 and 2, cell 1 is empty, cell 2 holds row 1


def test_file_layout_field_by_field(tmp_path):
    d = 32
    cent, sizes, rows, row_ids = _three_cells(d)
    f = str(tmp_path / "a.ivf.faiss")
    index_io.write_ivf_flat(f, cent, sizes, rows, row_ids, nprobe=2)
    b = open(f, "rb").read()
    assert b == Y.ivf_file_bytes(cent, sizes, rows, row_ids, nprobe=2)
    u = lambda fmt, off: struct.unpack_from("<" + fmt, b, off)
    assert u("4siqqqBi", 0) == (b"IwFl", d, 3, 1 << 20, 1 << 20, 1, 0)
    assert u("QQ", 37) == (3, 2)                      # nlist, nprobe
    assert u("4siqqqBi", 53) == (b"IxFI", d, 3, 1 << 20, 1 << 20, 1, 0)
    assert u("Q", 90) == (3 * d,)
    assert np.array_equal(np.frombuffer(b, "<f4", 3 * d, 98), cent.ravel())
    p = 98 + 12 * d
    assert u("BQ", p) == (0, 0)                       # direct map: NoMap, empty vector
    assert u("4sQQ", p + 9) == (b"ilar", 3, 4 * d)
    assert u("4sQQQQ", p + 29) == (b"full", 3, 2, 0, 1)
    p += 65
    assert np.array_equal(np.frombuffer(b, "<f4", 2 * d, p), rows[:2].ravel())
    assert u("qq", p + 8 * d) == (0, 2)
    p += 8 * d + 16
    assert np.array_equal(np.frombuffer(b, "<f4", d, p), rows[2])
    assert u("q", p + 4 * d) == (1,) and len(b) == p + 4 * d + 8
    st = index_io.read_ivf_flat(f)
    assert (st["d"], st["nlist"], st["nprobe"], st["ntotal"], st["is_trained"]) == (d, 3, 2, 3, True)
    assert np.array_equal(st["centroids"], cent) and np.array_equal(st["rows"], rows) and np.array_equal(st["row_ids"], row_ids)
    assert st["list_off"].tolist() == [0, 2, 2, 3]


def test_sparse_list_sizes_read_back_and_unknown_forms_are_refused(tmp_path):
    d = 32
    cent, sizes, rows, row_ids = _three_cells(d)
    full = Y.ivf_file_bytes(cent, sizes, rows, row_ids, nprobe=2)
    at = full.index(b"full")
    sprs = full[:at] + b"sprs" + struct.pack("<QQQQQ", 4, 0, 2, 2, 1) + full[at + 4 + 8 + 24:]      # a hand-made sparse form of the same sizes
    f = str(tmp_path / "s.ivf.faiss")
    open(f, "wb").write(sprs)
    a = index_io.read_ivf_flat(f)
    open(f, "wb").write(full)
    b = index_io.read_ivf_flat(f)
    for key in ("centroids", "rows", "row_ids", "list_off"):
        assert np.array_equal(a[key], b[key]), key
    # the writer itself goes sparse when at most half of the cells hold rows, as faiss does (n_non0 > nlist / 2 -> 'full')
    index_io.write_ivf_flat(f, cent, [0, 0, 3], rows, row_ids)
    got = open(f, "rb").read()
    assert got == Y.ivf_file_bytes(cent, [0, 0, 3], rows, row_ids) and b"sprs" in got and b"full" not in got
    assert index_io.read_ivf_flat(f)["list_off"].tolist() == [0, 0, 0, 3]
    open(f, "wb").write(full[:at] + b"zzzz" + full[at + 4:])
    with pytest.raises(ValueError, match="zzzz"):
        index_io.read_ivf_flat(f)
    open(f, "wb").write(full[:-5])
    with pytest.raises(ValueError):
        index_io.read_ivf_flat(f)
    open(f, "wb").write(b"IxFI" + full[4:])
    with pytest.raises(ValueError, match="IwFl"):
        index_io.read_ivf_flat(f)


def test_an_untrained_index_file_holds_no_centroids(tmp_path):
    f = str(tmp_path / "u.ivf.faiss")
    index_io.write_ivf_flat(f, np.zeros((0, 32), np.float32), [0, 0], np.zeros((0, 32), np.float32), np.zeros(0, np.int64), is_trained=False)
    st = index_io.read_ivf_flat(f)
    assert st["is_trained"] is False and st["centroids"].shape == (0, 32) and st["ntotal"] == 0 and st["nlist"] == 2


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
def _clusters(n=2000, d=32, k=20, seed=1):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((k, d)).astype(np.float32) * 4
    return (c[rng.integers(0, k, n)] + rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def test_yardstick_kmeans_is_deterministic_and_lowers_the_objective():
    x = _clusters()
    a, b = Y.kmeans(x, 16, niter=5), Y.kmeans(x, 16, niter=5)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    c0 = Y.kmeans(x, 16, niter=0)
    _, xs, init = Y.sample_and_init(x, 16)
    assert np.array_equal(c0, init) and all(any(np.array_equal(r, row) for row in xs) for r in c0)
    assert Y.objective(x, a) < Y.objective(x, c0)
    with pytest.raises(ValueError):
        Y.kmeans(x[:10], 16)
    # more rows than 256 per centroid: the sample is 256 * nlist sorted distinct rows
    _, xs, _ = Y.sample_and_init(x, 4)
    assert xs.shape[0] == 1024


def test_yardstick_search_agrees_with_a_double_loop():
    rng = np.random.default_rng(2)
    n, d, nlist = 60, 32, 5
    X = rng.integers(-3, 4, (n, d)).astype(np.float32)
    q = rng.integers(-3, 4, (3, d)).astype(np.float32)
    cells = rng.integers(0, nlist, n)
    row_ids, list_off = Y.cell_order(cells, nlist)
    stored = X[row_ids]
    probes = np.array([[0, 3, 3], [4, -1, 9], [2, 1, 0]])
    D, I = Y.search(q, stored, list_off, row_ids, probes, 8, id_base=100)
    for i in range(3):
        want = sorted(((-float(np.dot(q[i].astype(np.float64), X[r].astype(np.float64))), r) for r in range(n)
                       if cells[r] in [c for c in probes[i] if 0 <= c < nlist]))[:8]
        assert I[i, :len(want)].tolist() == [100 + r for _, r in want] and D[i, :len(want)].tolist() == [-s for s, _ in want]
        assert (I[i, len(want):] == -1).all() and (D[i, len(want):] == -Y.FLT_MAX).all()
    assert np.array_equal(Y.assign_cells(X[:4], X[:4] * 0 + np.eye(4, d, dtype=np.float32)), np.argmax(X[:4, :4], axis=1))
    # over the scan bound: padding
    assert (Y.search(q, stored, list_off, row_ids, probes, 8, max_scan_rows=1)[1] == -1).all()
