"""CPU side of the fp16 scalar-quantised index: the IxSQ file layout (index_io), SQFaissSearch's argument checks, the shim export."""
import struct

import numpy as np
import pytest

from lightretriever_amd import index_io


def write(path, codes, d):
    index_io.write_sq_fp16(str(path), [codes], d, codes.shape[0])
    return path.read_bytes()


def test_ixsq_header_bytes_and_field_order(tmp_path):
    d, n = 128, 3
    codes = (np.arange(n * d, dtype=np.float32).reshape(n, d) / 7).astype(np.float16)
    b = write(tmp_path / "a.sq.faiss", codes, d)
    assert b[:4] == b"IxSQ"
    assert struct.unpack_from("<iqqqBi", b, 4) == (d, n, 1 << 20, 1 << 20, 1, 0)     # the IxFI index header
    assert struct.unpack_from("<iifQQ", b, 37) == (4, 0, 0.0, d, 2 * d)              # qtype QT_fp16, rangestat, arg, d, code_size
    assert struct.unpack_from("<QQ", b, 65) == (0, n * 2 * d)                         # empty `trained`, code bytes
    assert len(b) == 81 + n * 2 * d
    assert np.array_equal(np.frombuffer(b[81:], dtype="<f2").reshape(n, d), codes)
    assert np.array_equal(index_io.read_sq_fp16(str(tmp_path / "a.sq.faiss")), codes)


def test_ixsq_rejects_other_qtypes_and_truncated_files(tmp_path):
    d = 64
    b = bytearray(write(tmp_path / "a", np.ones((2, d), np.float16), d))
    bad = tmp_path / "b"
    b2 = bytearray(b)
    struct.pack_into("<i", b2, 37, 0)                                                 # QT_8bit
    bad.write_bytes(bytes(b2))
    with pytest.raises(ValueError, match="qtype"):
        index_io.read_sq_fp16(str(bad))
    bad.write_bytes(bytes(b[:-2]))
    with pytest.raises(ValueError):
        index_io.read_sq_fp16(str(bad))
    bad.write_bytes(bytes(b[:50]))
    with pytest.raises(ValueError):
        index_io.read_sq_fp16(str(bad))
    bad.write_bytes(b"IxFI" + bytes(b[4:]))
    with pytest.raises(ValueError, match="IxSQ"):
        index_io.read_sq_fp16(str(bad))


def test_sq_faiss_search_arguments():
    from lightretriever_amd.retriever import SQFaissSearch
    s = SQFaissSearch(model=None, batch_size=8)
    assert s.get_index_name() == "sq_faiss_index" and s.qname == "QT_fp16" and s.corpus_chunk_size == 8 * 800
    with pytest.raises(NotImplementedError, match="QT_8bit"):
        SQFaissSearch(model=None, quantizer_type="QT_8bit")
    with pytest.raises(NotImplementedError, match="similarity_metric"):
        SQFaissSearch(model=None, similarity_metric=1)                                # faiss.METRIC_L2


def test_shim_exports_sq_faiss_search():
    from lightretriever.retriever.faiss_search import SQFaissSearch
    from lightretriever_amd.retriever import SQFaissSearch as S
    assert SQFaissSearch is S
