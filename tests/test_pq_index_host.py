"""CPU side of the product-quantised index: the IxPq file layout (index_io), PQFaissSearch's argument checks and HybridSearch routing, the
shim export, and the determinism of the yardstick's k-means (tests/pq_yardstick.py)."""
import struct

import numpy as np
import pytest

from lightretriever_amd import index_io

import pq_yardstick as Y


def write(path, cent, codes, d, M):
    index_io.write_pq(str(path), cent, [codes], d, M, codes.shape[0])
    return path.read_bytes()


def sample(d=32, M=4, n=5, seed=0):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, size=(n, M)).astype(np.uint8)
    return cent, codes


def test_ixpq_header_bytes_and_field_order(tmp_path):
    d, M, n = 32, 4, 5
    cent, codes = sample(d, M, n)
    b = write(tmp_path / "a.pq.faiss", cent, codes, d, M)
    assert b[:4] == b"IxPq"
    assert struct.unpack_from("<iqqqBi", b, 4) == (d, n, 1 << 20, 1 << 20, 1, 0)       # the IxFI index header
    assert struct.unpack_from("<QQQQ", b, 37) == (d, M, 8, d * 256)                    # d, M, nbits, centroid count
    off = 37 + 32
    assert np.array_equal(np.frombuffer(b[off:off + 4 * d * 256], dtype="<f4").reshape(M, 256, d // M), cent)
    off += 4 * d * 256
    assert struct.unpack_from("<Q", b, off) == (n * M,)
    off += 8
    assert np.array_equal(np.frombuffer(b[off:off + n * M], dtype=np.uint8).reshape(n, M), codes)
    off += n * M
    assert struct.unpack_from("<iBi", b, off) == (0, 0, M * 8 + 1)                     # search_type, encode_signs, polysemous_ht
    assert len(b) == off + 9
    c2, k2, trained = index_io.read_pq(str(tmp_path / "a.pq.faiss"))
    assert trained and np.array_equal(c2, cent) and np.array_equal(np.asarray(k2), codes)


def test_ixpq_round_trip_of_an_empty_index(tmp_path):
    cent, _ = sample()
    index_io.write_pq(str(tmp_path / "e"), cent, [], 32, 4, 0)
    c2, k2, _ = index_io.read_pq(str(tmp_path / "e"))
    assert np.array_equal(c2, cent) and k2.shape == (0, 4)


def test_ixpq_rejects_wrong_fourcc_nbits_and_truncated_files(tmp_path):
    d, M = 32, 4
    cent, codes = sample(d, M, 3)
    b = write(tmp_path / "a", cent, codes, d, M)
    bad = tmp_path / "b"
    b2 = bytearray(b)
    struct.pack_into("<Q", b2, 37 + 16, 4)                                              # nbits = 4
    bad.write_bytes(bytes(b2))
    with pytest.raises(ValueError, match="nbits"):
        index_io.read_pq(str(bad))
    bad.write_bytes(b"IxFI" + b[4:])
    with pytest.raises(ValueError, match="IxPq"):
        index_io.read_pq(str(bad))
    for cut in (len(b) - 1, len(b) - 9 - 2, 60, 37 + 32 + 100):
        bad.write_bytes(b[:cut])
        with pytest.raises(ValueError):
            index_io.read_pq(str(bad))
    b3 = bytearray(b)
    struct.pack_into("<iBi", b3, len(b) - 9, 1, 0, M * 8 + 1)                            # polysemous search type
    bad.write_bytes(bytes(b3))
    with pytest.raises(ValueError, match="search_type"):
        index_io.read_pq(str(bad))


def test_pq_faiss_search_arguments():
    from lightretriever_amd.retriever import PQFaissSearch
    s = PQFaissSearch(model=None, batch_size=8)
    assert s.get_index_name() == "pq_faiss_index" and s.num_of_centroids == 96 and s.code_size == 8 and not s.serves_rpc_shards
    with pytest.raises(NotImplementedError, match="use_rotation"):
        PQFaissSearch(model=None, use_rotation=True)
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        PQFaissSearch(model=None, similarity_metric=1)                                  # faiss.METRIC_L2
    with pytest.raises(NotImplementedError, match="code_size"):
        PQFaissSearch(model=None, code_size=4)
    with pytest.raises(ValueError, match="multiple"):
        PQFaissSearch(model=None, num_of_centroids=96)._new_index(2048, 0)              # the reference's default M at d = 2048


def test_shim_exports_pq_faiss_search():
    from lightretriever.retriever.faiss_search import PQFaissSearch
    from lightretriever_amd.retriever import PQFaissSearch as P
    assert PQFaissSearch is P


def test_hybrid_search_pq_map_builds_the_pq_searcher():
    from lightretriever_amd.retriever import HybridSearch, PQFaissSearch
    h = HybridSearch(model=None, batch_size=8, faiss_search_map="pq", num_of_centroids=64)
    assert type(h.dense_search) is PQFaissSearch and h.dense_search.num_of_centroids == 64
    with pytest.raises(NotImplementedError):
        HybridSearch(model=None, batch_size=8, faiss_search_map="pq", use_rotation=True)


def test_yardstick_kmeans_is_deterministic_and_lowers_the_objective():
    x = Y.prototype_corpus(1000, 32, 4, n_proto=16, seed=3)
    a, b = Y.kmeans(x, 4, niter=5, seed=7), Y.kmeans(x, 4, niter=5, seed=7)
    assert np.array_equal(a, b)
    c0 = Y.kmeans(x, 4, niter=0, seed=7)
    assert Y.objective(x, a, Y.encode(x, a)) < 0.8 * Y.objective(x, c0, Y.encode(x, c0))   # (0.64 of it on this run)


def test_yardstick_contract_on_a_hand_example():
    # two sub-spaces of one dimension; duplicate centroids go to the lower j; ties between rows go to the lower row
    C = np.zeros((2, 256, 1), np.float32)
    C[0, :, 0] = np.arange(256, dtype=np.float32)
    C[1, :, 0] = -np.arange(256, dtype=np.float32)
    C[0, 7, 0] = C[0, 3, 0]
    x = np.array([[3.0, -2.0], [3.4, -2.0], [6.6, -250.0]], np.float32)
    codes = Y.encode(x, C)
    assert codes.tolist() == [[3, 2], [3, 2], [6, 250]]
    D, I = Y.search(np.array([[1.0, 1.0]], np.float32), C, codes, 5)
    assert I.tolist() == [[0, 1, 2, -1, -1]] and D[0, 0] == 1.0 and D[0, 3] == -Y.FLT_MAX
