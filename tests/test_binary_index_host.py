"""CPU: the binary flat index's host side -- the IndexBinaryFlat file layout, the searcher's argument checks, the shim exports, the C ABI's
argument errors, and the numpy yardstick (tests/binary_yardstick.py) against hand-written cases."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binary_yardstick as Y  # noqa: E402


def packed_rows(n, d, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n, d // 8), dtype=np.uint8)


def test_ibxf_header_bytes_and_round_trip(tmp_path):
    from lightretriever_amd.index_io import read_binary_flat, write_binary_flat
    d, n = 72, 5
    rows = packed_rows(n, d)
    path = str(tmp_path / "a.bin.faiss")
    write_binary_flat(path, [rows[:2], rows[2:]], d, n)
    raw = open(path, "rb").read()
    assert raw[0:4] == b"IBxF"
    assert struct.unpack_from("<i", raw, 4) == (d,)                  # bits
    assert struct.unpack_from("<i", raw, 8) == (d // 8,)             # code_size
    assert struct.unpack_from("<q", raw, 12) == (n,)                 # ntotal
    assert raw[20] == 1                                              # is_trained
    assert struct.unpack_from("<i", raw, 21) == (1,)                 # metric_type
    assert struct.unpack_from("<Q", raw, 25) == (n * d // 8,)        # size word of xb
    assert raw[33:] == rows.tobytes() and len(raw) == 33 + n * d // 8
    back = read_binary_flat(path)
    assert back.dtype == np.uint8 and back.shape == (n, d // 8) and np.array_equal(back, rows)
    write_binary_flat(path, [], 64, 0)
    assert read_binary_flat(path).shape == (0, 8)


def test_bad_binary_files_are_rejected(tmp_path):
    from lightretriever_amd.index_io import read_binary_flat, read_flat_ip, write_binary_flat, write_flat_ip
    d, n = 64, 7
    rows = packed_rows(n, d)
    path = str(tmp_path / "a.bin.faiss")
    write_binary_flat(path, [rows], d, n)
    raw = open(path, "rb").read()
    bad = str(tmp_path / "bad.faiss")

    def rejects(data):
        open(bad, "wb").write(data)
        with pytest.raises(ValueError):
            read_binary_flat(bad)
    rejects(b"IxFI" + raw[4:])                                       # wrong fourcc
    rejects(raw[:-1])                                                # truncated rows
    rejects(raw[:20])                                                # truncated header
    rejects(raw + b"\0")                                             # trailing bytes
    rejects(raw[:8] + struct.pack("<i", d // 8 + 1) + raw[12:])      # code_size != d / 8
    rejects(raw[:25] + struct.pack("<Q", n * d // 8 - 1) + raw[33:])  # size word
    with pytest.raises(ValueError):
        read_flat_ip(path)                                           # and the float reader refuses a binary file
    flat = str(tmp_path / "f.faiss")
    write_flat_ip(flat, [np.zeros((2, 8), np.float32)], 8, 2)
    with pytest.raises(ValueError):
        read_binary_flat(flat)
    with pytest.raises(ValueError):
        write_binary_flat(bad, [rows], d, n + 1)                     # fewer rows than the header says
    with pytest.raises(ValueError):
        write_binary_flat(bad, [rows], d + 8, n)                     # block width
    with pytest.raises(ValueError):
        write_binary_flat(bad, [rows], 60, n)                        # d % 8


def test_searcher_argument_checks_and_the_hybrid_route():
    from lightretriever_amd.index import BinaryFlatIndex
    from lightretriever_amd.retriever import BinaryFaissSearch, FaissBinaryIndex, FaissIndex, FlatIPFaissSearch, HybridSearch
    s = BinaryFaissSearch(None, batch_size=8, binary_k=50, threshold=0.25)
    assert isinstance(s, FlatIPFaissSearch) and s.index_cls is BinaryFlatIndex and s.index_ext == "bin" and s.serves_rpc_shards is False
    assert s.faiss_index_cls is FaissBinaryIndex and issubclass(FaissBinaryIndex, FaissIndex)
    assert s.get_index_name() == "binary_faiss_index" and s.binary_k == 50 and s.threshold == 0.25
    with pytest.raises(ValueError, match="top_k=51.*binary_k=50"):
        s.search({}, {}, top_k=51)
    with pytest.raises(NotImplementedError, match="cos_sim"):
        s.search({}, {}, top_k=10, score_function="cos_sim")
    with pytest.raises(NotImplementedError, match="cos_sim"):
        BinaryFaissSearch(None, score_function="cos_sim")
    for bad in (0, 2049):
        with pytest.raises(ValueError, match="binary_k"):
            BinaryFaissSearch(None, binary_k=bad)
    h = HybridSearch(model=None, faiss_search_map="binary")
    assert type(h.dense_search) is BinaryFaissSearch and h.dense_search.binary_k == 1000 and h.dense_search.threshold == 0
    h = HybridSearch(model=None, batch_size=4, faiss_search_map="binary", binary_k=200, threshold=0.5)
    assert h.dense_search.binary_k == 200 and h.dense_search.threshold == 0.5 and h.dense_search.batch_size == 4
    assert type(HybridSearch(model=None, faiss_search_map="hnsw").dense_search) is FlatIPFaissSearch        # other unknown maps: still flat


def test_shim_exports():
    from lightretriever.retriever.faiss_index import FaissBinaryIndex, FaissIndex
    from lightretriever.retriever.faiss_search import BinaryFaissSearch
    import lightretriever_amd
    from lightretriever_amd import retriever
    assert BinaryFaissSearch is retriever.BinaryFaissSearch and FaissBinaryIndex is retriever.FaissBinaryIndex and FaissIndex is retriever.FaissIndex
    assert lightretriever_amd.BinaryFlatIndex is retriever.BinaryFlatIndex


def test_c_abi_argument_errors_without_a_gpu():
    from lightretriever_amd import _lib
    l = _lib.lib()
    for s in ("lrx_binary_pack_rows", "lrx_binary_store_rows", "lrx_binary_decode_rows", "lrx_binary_workspace_bytes", "lrx_binary_hamming_search",
              "lrx_binary_ip_search"):
        assert s in _lib.SIGNATURES, s
    assert l.lrx_abi_version() == 9
    assert l.lrx_binary_workspace_bytes(1000, 2048, 10, 1000) > 0 and l.lrx_binary_workspace_bytes(1000, 100, 10, 1000) == 0
    assert l.lrx_binary_ip_search(None, 10, 64, None, 1, 0.0, None, 5, 4, 0, None, None, None, None, 0, 0, None) == -1   # k > binary_k
    assert b"binary_k" in l.lrx_last_error()
    assert l.lrx_binary_ip_search(None, 10, 64, None, 1, 0.0, None, 1, 2049, 0, None, None, None, None, 0, 0, None) == -1
    assert l.lrx_binary_ip_search(None, 10, 60, None, 1, 0.0, None, 1, 10, 0, None, None, None, None, 0, 0, None) == -1 and b"dim=60" in l.lrx_last_error()
    assert l.lrx_binary_hamming_search(None, 10, 64, None, 1, 0.0, None, 0, 0, None, None, None, None, 0, 0, None) == -1
    assert l.lrx_binary_hamming_search(None, 10, 64, None, 1, 0.0, None, 5, 0, None, None, None, None, 0, 0, None) == -1 and b"null" in l.lrx_last_error()
    assert l.lrx_binary_hamming_search(None, 10, 64, None, 0, 0.0, None, 5, 0, None, None, None, None, 0, 0, None) == 0  # no queries: nothing to do
    assert l.lrx_binary_pack_rows(None, 4, 8, 64, 0.0, None, None, 0, None) == -1                                         # ldx < dim
    assert l.lrx_binary_store_rows(None, 4, 7, 64, None, 0, None) == -1
    assert l.lrx_binary_decode_rows(None, 0, 4, 64, None, 7, None) == -1
    assert l.lrx_binary_pack_rows(None, 0, 64, 64, 0.0, None, None, 0, None) == 0


def test_yardstick_hand_written_cases():
    x = np.array([[1, -1, 0.5, 0, -0.0, 2, -3, 4, 0, 0, 0, 0, 0, 0, 0, 1e-30]], np.float32)
    assert Y.pack(x).tolist() == [[0b10100101, 0b00000001]]                       # dimension 0 is the most significant bit of byte 0
    assert Y.pack(np.full((1, 8), 0.25, np.float32), threshold=0.25).tolist() == [[0]]            # equal to the threshold: strict > gives 0
    assert Y.pack(np.array([[np.nan, 1, np.nan, -1, np.inf, -np.inf, 0.0, -0.0]], np.float32)).tolist() == [[0b01001000]]
    t = np.array([0, 1, 2, 3, -1, -2, -3, 0.5], np.float32)
    assert Y.pack(np.array([[0.5, 0.5, 2.5, 2.5, -0.5, -2.5, -2.5, 0.5]], np.float32), threshold=t).tolist() == [[0b10101010]]
    a, b = np.array([[0b11110000, 0b00000001]], np.uint8), np.array([[0b11110000, 0b00000001], [0b00001111, 0b00000000], [0b11110001, 0b00000001]], np.uint8)
    assert Y.hamming(a, b).tolist() == [[0, 9, 1]]
    # rerank score: +q where the bit is set, -q where it is not
    q = np.array([[1, 2, 3, 4, 5, 6, 7, 8]], np.float32)
    rows = np.array([[0b11111111], [0b00000000], [0b10000001]], np.uint8)
    assert Y.rerank_scores(q[0], rows).tolist() == [36.0, -36.0, 1 + 8 - 27]
    D, I = Y.search(q, rows, 2, binary_k=3)
    assert I.tolist() == [[0, 2]] and D.tolist() == [[36.0, -18.0]]
    D, I = Y.search(q, rows, 2, binary_k=2)                                        # candidates: rows 0 (h = 0) and 2 (h = 6); row 1 (h = 8) is out
    assert I.tolist() == [[0, 2]]
    D, I = Y.search(q, rows[:1], 3, binary_k=3)
    assert I.tolist() == [[0, -1, -1]] and D[0, 1] == np.float32(-Y.FLT_MAX)
    g = Y.grid_queries(np.random.default_rng(0), 4, 4096)
    assert np.abs(g).max() <= 4 and np.array_equal(g * 1024, np.round(g * 1024))
    # ... on which an fp64 sum is exact in any order
    s = (g.astype(np.float64)[0])
    assert s.sum() == s[::-1].sum() == float(np.sum((s * 1024).astype(np.int64))) / 1024


def test_yardstick_tie_rule_on_duplicated_rows():
    rng = np.random.default_rng(3)
    base = packed_rows(4, 64, seed=5)
    xb = np.repeat(base, 6, axis=0)[rng.permutation(24)]                           # 4 distinct rows, 6 copies each, shuffled
    q = np.unpackbits(base[:1], axis=1).astype(np.float32) * 2 - 1                 # the query's bits are row class 0's
    H = Y.hamming(Y.pack(q), xb)
    D, I = Y.hamming_topk(H, 9)
    same = np.flatnonzero((xb == base[0]).all(axis=1))
    assert I[0, :6].tolist() == sorted(same.tolist()) and D[0, :6].tolist() == [0] * 6          # six ties at h = 0: ascending rows
    assert all(D[0, i] < D[0, i + 1] or (D[0, i] == D[0, i + 1] and I[0, i] < I[0, i + 1]) for i in range(8))
    D, I = Y.hamming_topk(H, 30)
    assert I[0, 24:].tolist() == [-1] * 6 and D[0, 24:].tolist() == [Y.INT_MAX] * 6
    # the candidate cut falls inside a tie class: the lowest rows of the class are the candidates, and equal scores keep the lower row first
    Dr, Ir = Y.search(q, xb, 4, binary_k=4)
    assert Ir[0].tolist() == sorted(same.tolist())[:4] and len(set(Dr[0].tolist())) == 1
