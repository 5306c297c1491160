"""On-disk format of a flat inner-product index shard.

The reference persists `faiss.write_index(IndexFlatIP)` as `{prefix}.{ext}.faiss` next to a `{prefix}.{ext}.tsv` id map
(retriever/faiss_search.py:99-123, :478-488, :506-507; retriever/faiss_index.py:42-43).  The byte layout written here is Faiss's
own serialisation of IndexFlat as published in faiss/impl/index_write.cpp (v1.7.x - 1.8):

    u32   fourcc 'IxFI'                       (IndexFlatIP)
    i32   d
    i64   ntotal
    i64   dummy = 1 << 20,  i64 dummy = 1 << 20
    u8    is_trained = 1
    i32   metric_type = 0                     (METRIC_INNER_PRODUCT)
    u64   n_floats = ntotal * d               (WRITEXBVECTOR of the codes: size in 4-byte units)
    f32   x[ntotal * d]                       row-major

so a shard written here is a regular Faiss flat index file and a `{prefix}.flat.faiss` written by the reference loads here.
Faiss itself is not installed in this image: the layout is **unverified against a Faiss build** (round trip and header bytes
are tested).  Multi-rank: every rank writes `{prefix}.rank{r}-of-{R}.{ext}.faiss/.tsv` holding its own rows, so a 10 M-document
index reloads per rank without re-encoding and without one rank ever holding the whole matrix.

An fp16 scalar-quantised shard (SQFp16Index) is written as Faiss's serialisation of IndexScalarQuantizer, same source:

    u32   fourcc 'IxSQ'
          the index header of 'IxFI' above (d, ntotal, two dummies, is_trained, metric_type = 0)
    i32   qtype = 4                           (ScalarQuantizer::QT_fp16)
    i32   rangestat = 0,  f32 rangestat_arg = 0
    u64   d,  u64 code_size = 2 d
    u64   0                                   (`trained`: an empty float vector -- QT_fp16 trains nothing)
    u64   n_bytes = ntotal * 2 d              (WRITEVECTOR of the codes)
    f16   codes[ntotal * d]                   row-major, little-endian

Like the flat layout it is **unverified against a Faiss build**.  read_sq_fp16 rejects files with any other qtype.

An 8-bit scalar-quantised shard (SQ8Index) is the same 'IxSQ' record with qtype = 0 (QT_8bit: code_size = d, `trained` = vmin[d] ++ vdiff[d],
2 d floats) or qtype = 2 (QT_8bit_uniform: `trained` = vmin, vdiff, 2 floats) and one byte per element:

    u64   len(trained),  f32 trained[len(trained)]
    u64   n_bytes = ntotal * d,  u8 codes[ntotal][d]      row-major

(file size 37 + 28 + 8 + 4 len(trained) + 8 + ntotal * d).  sq_qtype(fname) tells a caller which of the two readers a file needs.

A product-quantised shard (PQIndex, faiss IndexPQ(d, M, 8, METRIC_INNER_PRODUCT)) is written as Faiss's serialisation of IndexPQ, same
source:

    u32   fourcc 'IxPq'
          the index header of 'IxFI' above (d, ntotal, two dummies, is_trained, metric_type = 0)
    u64   d,  u64 M,  u64 nbits = 8           (write_ProductQuantizer)
    u64   d * 256,  f32 centroids[M][256][d / M]
    u64   ntotal * M,  u8 codes[ntotal][M]    row-major
    i32   search_type = 0 (ST_PQ),  u8 encode_signs = 0,  i32 polysemous_ht = M * nbits + 1

It too is **unverified against a Faiss build**.  Files with nbits != 8 or any other inconsistency are rejected.

A binary flat shard (BinaryFlatIndex, faiss IndexBinaryFlat(d)) is written as Faiss's `write_index_binary` of an IndexBinaryFlat, same source
(write_index_binary_header: no dummies, and the code size in the header):

    u32   fourcc 'IBxF'
    i32   d                                   (bits)
    i32   code_size = d / 8
    i64   ntotal
    u8    is_trained = 1
    i32   metric_type = 1                     (METRIC_L2: what IndexBinary's constructor sets; the search is by Hamming distance)
    u64   n_bytes = ntotal * code_size        (WRITEVECTOR of xb)
    u8    xb[ntotal][code_size]               row-major, np.packbits bit order

Like the others it is **unverified against a Faiss build**.  Files with code_size != d / 8, a size word or a length that does not match are
rejected.

A PCA pre-transform index (PreTransformIndex over a PCAMatrix, faiss IndexPreTransform(PCAMatrix, base)) is written as Faiss's serialisation of
IndexPreTransform with a chain of one PCAMatrix (write_VectorTransform), same source:

    u32   fourcc 'IxPT'
          the index header of 'IxFI' above (d = d_in, ntotal, two dummies, is_trained, metric_type = 0)
    i32   nchain = 1
    u32   fourcc 'PcAm'                       (PCAMatrix with epsilon; the legacy 'PCAm' record has none and is rejected)
    f32   eigen_power,  f32 epsilon = 0,  u8 random_rotation,  i32 balanced_bins = 0
    u64 n, f32 mean[n]    u64 n, f32 eigenvalues[n]    u64 n, f32 PCAMat[n]        (n = d_in, d_in, d_in * d_in; all 0 when untrained)
    u8    have_bias = 1                       (the LinearTransform part)
    u64 n, f32 A[n]       u64 n, f32 b[n]                                          (n = d_out * d_in, d_out; 0 when untrained)
    i32   d_in,  i32 d_out,  u8 is_trained    (the VectorTransform part)
          the base index: a complete 'IxFI', 'IxSQ' or 'IxPq' record as above, to the end of the file

It too is **unverified against a Faiss build**.  Truncated files, other chain lengths, other transforms and inconsistent sizes are rejected.

A refine index (RefineFlatIndex, faiss IndexRefineFlat(base) / IndexRefine(base, refine_index)) is written as Faiss's serialisation of
IndexRefine, same source:

    u32   fourcc 'IxRF'
          the index header of 'IxFI' above (d, ntotal, two dummies, is_trained, metric_type = 0)
          the base index: a complete 'IxPq', 'IxSQ' or 'IxPT' record as above
          the refine index: a complete 'IxFI' record, or an 'IxSQ' record with qtype = 4 (QT_fp16)
    f32   k_factor

It too is **unverified against a Faiss build**.  Here a record is followed by more: every reader takes, next to `offset`, an optional `end`
(default: the end of the file) that its record must fill exactly, index_record_end finds where a record stops, and every writer can continue
a file (`append=True`).  Truncated files, a base or refine index whose d / ntotal disagree with the header and other record types are
rejected.

An inverted-file flat index (IVFFlatIndex, faiss IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT)) is written as Faiss's
serialisation of IndexIVFFlat (write_ivf_header, write_direct_map, write_InvertedLists of an ArrayInvertedLists), same source:

    u32   fourcc 'IwFl'
          the index header of 'IxFI' above (d, ntotal, two dummies, is_trained, metric_type = 0)
    u64   nlist,  u64 nprobe
          the quantiser: a complete 'IxFI' record over the nlist centroids (0 rows when untrained)
    u8    direct-map type = 0 (NoMap),  u64 0                  (an empty i64 vector)
    u32   fourcc 'ilar',  u64 nlist,  u64 code_size = 4 d
    u32   'full', u64 nlist, u64 sizes[nlist]       when more than nlist / 2 cells are non-empty (faiss: n_non0 > nlist / 2, integer division)
    u32   'sprs', u64 2 m, u64 (cell, size)[m]      otherwise: the m non-empty cells in ascending order
          then for every non-empty cell, in ascending order: f32 rows[size][d], i64 ids[size]

Real faiss bytes cannot be produced here (faiss is not installed): like the others the layout is **unverified against a Faiss build**.  The
reader accepts both list-size forms and refuses any other by name.

An inverted-file product-quantised index (IVFPQIndex, faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8, METRIC_INNER_PRODUCT)) is written as
Faiss's serialisation of IndexIVFPQ (write_ivf_header, then by_residual, code_size, write_ProductQuantizer, write_InvertedLists), same source:

    u32   fourcc 'IwPQ'
          the IVF header exactly as in 'IwFl' above: index header, u64 nlist, u64 nprobe, the 'IxFI' quantiser, the empty direct map
    u8    by_residual
    u64   code_size = M
    u64   d,  u64 M,  u64 nbits = 8,  u64 n = 256 d,  f32 centroids[M][256][d / M]     (the ProductQuantizer of 'IxPq' above)
    u32   fourcc 'ilar',  u64 nlist,  u64 code_size = M
          the list sizes, 'full' or 'sprs', as in 'IwFl'
          then for every non-empty cell, in ascending order: u8 codes[size][M] (row-major), i64 ids[size]

Like 'IwFl' it is **unverified against a Faiss build** (faiss is not installed here).  The reader accepts both list-size forms and refuses any
other by name; index_record_end knows the record, so a refine index can hold it as its base.

An inverted-file fp16 scalar-quantised index (IVFSQIndex, faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_fp16,
METRIC_INNER_PRODUCT)) is written as Faiss's serialisation of IndexIVFScalarQuantizer (write_ivf_header, write_ScalarQuantizer, then code_size,
by_residual, write_InvertedLists), same source:

    u32   fourcc 'IwSq'
          the IVF header exactly as in 'IwFl' above: index header, u64 nlist, u64 nprobe, the 'IxFI' quantiser, the empty direct map
    i32   qtype = 4 (QT_fp16),  i32 rangestat = 0,  f32 rangestat_arg = 0,  u64 d,  u64 code_size = 2 d     (the ScalarQuantizer of 'IxSQ' above)
    u64   0                                   (`trained`: an empty float vector)
    u64   code_size = 2 d
    u8    by_residual
    u32   fourcc 'ilar',  u64 nlist,  u64 code_size = 2 d
          the list sizes, 'full' or 'sprs', as in 'IwFl'
          then for every non-empty cell, in ascending order: f16 codes[size][d] (row-major, little-endian), i64 ids[size]

Like 'IwFl' and 'IwPQ' it is **unverified against a Faiss build** (faiss is not installed here).  The reader accepts both list-size forms and
refuses any other qtype, a non-empty direct map and other inverted lists by name; index_record_end knows the record, so a refine index can hold
it as its base.

An inverted-file 8-bit scalar-quantised index (IVFSQ8Index, faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit | QT_8bit_uniform,
METRIC_INNER_PRODUCT)) is the same 'IwSq' record with the 8-bit ScalarQuantizer of 'IxSQ' above:

    i32   qtype = 0 (QT_8bit) or 2 (QT_8bit_uniform),  i32 rangestat = 0,  f32 rangestat_arg = 0,  u64 d,  u64 code_size = d
    u64   len(trained),  f32 trained[len(trained)]        (vmin ++ vdiff: 2 d floats for QT_8bit, 2 for QT_8bit_uniform)
    u64   code_size = d
    u8    by_residual
    u32   fourcc 'ilar',  u64 nlist,  u64 code_size = d
          the list sizes, 'full' or 'sprs', then for every non-empty cell: u8 codes[size][d] (row-major), i64 ids[size]

It too is **unverified against a Faiss build**.  write_ivf_sq8 / read_ivf_sq8 serve it; read_ivf_sq keeps refusing qtype 0 / 2 and
read_ivf_sq8 refuses qtype 4 pointing to read_ivf_sq; ivf_sq_qtype(fname) tells a caller which reader a record needs (as sq_qtype does for
'IxSQ'), and index_record_end knows both lengths, so a refine index can hold either as its base."""
from __future__ import annotations

import csv
import os
import struct
from typing import Callable, Iterable, NamedTuple, Optional

import numpy as np

FOURCC_FLAT_IP = b"IxFI"
_HEADER = struct.Struct("<4siqqqBi")     # fourcc, d, ntotal, dummy, dummy, is_trained, metric_type  (37 bytes, packed)
HEADER_BYTES = _HEADER.size + 8          # + u64 vector size
MAPPING_TSV_KEYS = ["beir-docid", "faiss-docid"]


def shard_prefix(prefix: str, rank: int = 0, world: int = 1) -> str:
    return prefix if world == 1 else f"{prefix}.rank{rank}-of-{world}"


def _index_header(fourcc: bytes, d: int, ntotal: int, is_trained: bool = True) -> bytes:
    return _HEADER.pack(fourcc, d, ntotal, 1 << 20, 1 << 20, int(bool(is_trained)), 0)


def _write_index(fname: str, who: str, ntotal: int, head: bytes, blocks: Iterable[np.ndarray], dtype: str, width: int, width_name: str = "d",
                 tail: bytes = b"", prefix: bytes = b"", append: bool = False) -> None:
    """`head` (the packed index header and the format's fields up to and including the size word of the rows), the rows streamed from
    `blocks` (arrays [n_i, width] in row order, sum n_i == ntotal, written as `dtype`), then `tail` -- to a .tmp file renamed over fname.
    `prefix`: bytes that precede the record (the enclosing record of write_pre_transform); every reader takes the matching `offset`.
    append: continue the existing file fname instead (the second record of write_refine, which does the renaming itself)."""
    tmp = fname if append else fname + ".tmp"
    with open(tmp, "ab" if append else "wb") as f:
        f.write(prefix)
        f.write(head)
        rows = 0
        for b in blocks:
            b = np.ascontiguousarray(b, dtype=dtype)
            if b.ndim != 2 or b.shape[1] != width:
                raise ValueError(f"{who}: block {b.shape} does not match {width_name}={width}")
            f.write(b.tobytes())
            rows += b.shape[0]
        if rows != ntotal:
            raise ValueError(f"{who}: wrote {rows} rows, header says {ntotal}")
        f.write(tail)
    if not append:
        os.replace(tmp, fname)


def _end(fname: str, end: Optional[int]) -> int:
    """Where a record that starts somewhere in fname must stop: `end`, or the end of the file."""
    size = os.path.getsize(fname)
    if end is not None and not 0 <= end <= size:
        raise ValueError(f"{fname}: a record is said to end at byte {end} of {size}")
    return size if end is None else end


def _read_header(f, fname: str, fourcc: bytes, what: str):
    """-> (d, ntotal, is_trained, metric_type) of the common index header at f's position; ValueError unless its fourcc is `fourcc`."""
    got, d, ntotal, _, _, trained, metric = _HEADER.unpack(f.read(_HEADER.size))
    if got != fourcc:
        raise ValueError(f"{fname}: fourcc {got!r} is not {what} ({fourcc.decode()!r})")
    return d, ntotal, trained, metric


def write_flat_ip(fname: str, blocks: Iterable[np.ndarray], d: int, ntotal: int, prefix: bytes = b"", append: bool = False) -> None:
    """blocks: fp32 [n_i, d] arrays in row order (streamed: the shard comes off the GPU in chunks), sum n_i == ntotal."""
    _write_index(fname, "write_flat_ip", ntotal, _index_header(FOURCC_FLAT_IP, d, ntotal) + struct.pack("<Q", ntotal * d), blocks, "<f4", d,
                 prefix=prefix, append=append)


def read_flat_ip(fname: str, offset: int = 0, end: Optional[int] = None) -> np.memmap:
    """-> read-only memmap fp32 [ntotal, d] over the file (no copy; the caller streams it to the GPU).  offset: where the record starts; it
    runs to `end` (default: the end of the file)."""
    size = _end(fname, end) - offset
    if size < HEADER_BYTES:
        raise ValueError(f"{fname}: too short for a flat index header")
    with open(fname, "rb") as f:
        f.seek(offset)
        d, ntotal, _, metric = _read_header(f, fname, FOURCC_FLAT_IP, "an inner-product flat index")
        (n_floats,) = struct.unpack("<Q", f.read(8))
    if metric != 0 or d <= 0 or ntotal < 0 or n_floats != ntotal * d or size != HEADER_BYTES + 4 * n_floats:
        raise ValueError(f"{fname}: inconsistent flat index header (d={d}, ntotal={ntotal}, floats={n_floats}, metric={metric}, bytes={size})")
    return np.memmap(fname, dtype="<f4", mode="r", offset=offset + HEADER_BYTES, shape=(ntotal, d))


FOURCC_SQ = b"IxSQ"
QT_FP16 = 4
_SQ = struct.Struct("<iifQQ")            # qtype, rangestat, rangestat_arg, d, code_size  (28 bytes, packed)
SQ_HEADER_BYTES = _HEADER.size + _SQ.size + 8 + 8   # + empty `trained` vector + u64 code bytes


def write_sq_fp16(fname: str, blocks: Iterable[np.ndarray], d: int, ntotal: int, prefix: bytes = b"", append: bool = False) -> None:
    """blocks: fp16 [n_i, d] arrays (the codes) in row order, sum n_i == ntotal."""
    head = _index_header(FOURCC_SQ, d, ntotal) + _SQ.pack(QT_FP16, 0, 0.0, d, 2 * d) + struct.pack("<QQ", 0, ntotal * 2 * d)   # (empty `trained`, code bytes)
    _write_index(fname, "write_sq_fp16", ntotal, head, blocks, "<f2", d, prefix=prefix, append=append)


def _read_sq_prefix(f, fname: str, more: int = 8, offset: int = 0, end: Optional[int] = None):
    """The 'IxSQ' prefix (index header + _SQ) at `offset` of the open file f -> (record size, d, ntotal, is_trained, metric_type, qtype,
    sq.d, code_size); ValueError when the record is shorter than the prefix and `more` bytes, or is no 'IxSQ' record."""
    size = _end(fname, end) - offset
    if size < _HEADER.size + _SQ.size + more:
        raise ValueError(f"{fname}: too short for a scalar-quantiser index header")
    f.seek(offset)
    d, ntotal, is_trained, metric = _read_header(f, fname, FOURCC_SQ, "a scalar-quantiser index")
    qtype, _, _, sq_d, code_size = _SQ.unpack(f.read(_SQ.size))
    return size, d, ntotal, is_trained, metric, qtype, sq_d, code_size


def read_sq_fp16(fname: str, offset: int = 0, end: Optional[int] = None) -> np.memmap:
    """-> read-only memmap fp16 [ntotal, d] of the codes (no copy).  offset: where the record starts; it runs to `end` (default: the end of
    the file)."""
    with open(fname, "rb") as f:
        size, d, ntotal, _, metric, qtype, sq_d, code_size = _read_sq_prefix(f, fname, offset=offset, end=end)
        if qtype != QT_FP16:
            raise ValueError(f"{fname}: ScalarQuantizer qtype {qtype} is not served (only QT_fp16 = {QT_FP16})")
        (n_trained,) = struct.unpack("<Q", f.read(8))
        off = _HEADER.size + _SQ.size + 8 + 4 * n_trained
        f.seek(offset + off)
        tail = f.read(8) if off + 8 <= size else b""
    if len(tail) < 8:
        raise ValueError(f"{fname}: truncated scalar-quantiser index header")
    (n_bytes,) = struct.unpack("<Q", tail)
    off += 8
    if metric != 0 or d <= 0 or ntotal < 0 or sq_d != d or code_size != 2 * d or n_bytes != ntotal * 2 * d or size != off + n_bytes:
        raise ValueError(f"{fname}: inconsistent QT_fp16 index (d={d}, ntotal={ntotal}, sq.d={sq_d}, code_size={code_size}, "
                         f"code bytes={n_bytes}, metric={metric}, file bytes={size})")
    return np.memmap(fname, dtype="<f2", mode="r", offset=offset + off, shape=(ntotal, d))


QT_8BIT, QT_8BIT_UNIFORM = 0, 2
SQ8_QTYPES = {"QT_8bit": QT_8BIT, "QT_8bit_uniform": QT_8BIT_UNIFORM}


def _sq8_trained_len(qtype: int, d: int) -> int:
    if qtype not in (QT_8BIT, QT_8BIT_UNIFORM):
        raise ValueError(f"ScalarQuantizer qtype {qtype} is not an 8-bit quantiser (QT_8bit = {QT_8BIT}, QT_8bit_uniform = {QT_8BIT_UNIFORM})")
    return 2 * d if qtype == QT_8BIT else 2


def sq_qtype(fname: str, offset: int = 0, end: Optional[int] = None) -> int:
    """The ScalarQuantizer qtype of an 'IxSQ' file (faiss's enum: 0 8bit, 1 4bit, 2 8bit_uniform, 3 4bit_uniform, 4 fp16, ...)."""
    with open(fname, "rb") as f:
        return _read_sq_prefix(f, fname, more=0, offset=offset, end=end)[5]


def write_sq8(fname: str, trained: np.ndarray, blocks: Iterable[np.ndarray], d: int, ntotal: int, qtype: int = QT_8BIT, is_trained: bool = True,
              prefix: bytes = b"", append: bool = False) -> None:
    """trained: fp32 vmin ++ vdiff (2 d floats for QT_8bit, 2 for QT_8bit_uniform); blocks: uint8 [n_i, d] code arrays in row order."""
    t = np.ascontiguousarray(trained, dtype="<f4").reshape(-1)
    if t.size != _sq8_trained_len(qtype, d):
        raise ValueError(f"write_sq8: {t.size} trained floats, expected {_sq8_trained_len(qtype, d)}")
    head = _index_header(FOURCC_SQ, d, ntotal, is_trained) + _SQ.pack(qtype, 0, 0.0, d, d) + struct.pack("<Q", t.size) + t.tobytes() + struct.pack("<Q", ntotal * d)
    _write_index(fname, "write_sq8", ntotal, head, blocks, np.uint8, d, prefix=prefix, append=append)


def read_sq8(fname: str, offset: int = 0, end: Optional[int] = None):
    """-> (qtype, trained fp32 [2 d] or [2], codes: read-only memmap uint8 [ntotal, d], is_trained).  offset: where the record starts; it runs
    to `end` (default: the end of the file)."""
    fixed = _HEADER.size + _SQ.size + 8
    with open(fname, "rb") as f:
        size, d, ntotal, is_trained, metric, qtype, sq_d, code_size = _read_sq_prefix(f, fname, offset=offset, end=end)
        if qtype not in (QT_8BIT, QT_8BIT_UNIFORM):
            raise ValueError(f"{fname}: ScalarQuantizer qtype {qtype} is not served here (QT_8bit = {QT_8BIT}, QT_8bit_uniform = {QT_8BIT_UNIFORM})")
        (n_t,) = struct.unpack("<Q", f.read(8))
        if metric != 0 or d <= 0 or ntotal < 0 or sq_d != d or code_size != d or n_t != _sq8_trained_len(qtype, d) or size < fixed + 4 * n_t + 8:
            raise ValueError(f"{fname}: inconsistent 8-bit scalar-quantiser index (d={d}, ntotal={ntotal}, sq.d={sq_d}, code_size={code_size}, "
                             f"trained floats={n_t}, metric={metric}, file bytes={size})")
        trained = np.frombuffer(f.read(4 * n_t), dtype="<f4").copy()
        (n_b,) = struct.unpack("<Q", f.read(8))
    off = fixed + 4 * n_t + 8
    if n_b != ntotal * d or size != off + n_b:
        raise ValueError(f"{fname}: inconsistent 8-bit codes (code bytes={n_b}, ntotal * d={ntotal * d}, file bytes={size})")
    codes = np.memmap(fname, dtype=np.uint8, mode="r", offset=offset + off, shape=(ntotal, d)) if ntotal else np.zeros((0, d), np.uint8)
    return qtype, trained, codes, bool(is_trained)


FOURCC_PQ = b"IxPq"
_PQ = struct.Struct("<QQQ")              # d, M, nbits (write_ProductQuantizer)
_PQ_TAIL = struct.Struct("<iBi")         # search_type, encode_signs, polysemous_ht (9 bytes, packed)


def write_pq(fname: str, centroids: np.ndarray, blocks: Iterable[np.ndarray], d: int, M: int, ntotal: int, is_trained: bool = True,
             prefix: bytes = b"", append: bool = False) -> None:
    """centroids: fp32 [M, 256, d / M]; blocks: uint8 [n_i, M] code arrays in row order, sum n_i == ntotal."""
    c = np.ascontiguousarray(centroids, dtype="<f4")
    if c.size != d * 256:
        raise ValueError(f"write_pq: {c.size} centroid floats, expected d * 256 = {d * 256}")
    head = _index_header(FOURCC_PQ, d, ntotal, is_trained) + _PQ.pack(d, M, 8) + struct.pack("<Q", d * 256) + c.tobytes() + struct.pack("<Q", ntotal * M)
    _write_index(fname, "write_pq", ntotal, head, blocks, np.uint8, M, "M", _PQ_TAIL.pack(0, 0, M * 8 + 1), prefix=prefix, append=append)


def read_pq(fname: str, offset: int = 0, end: Optional[int] = None):
    """-> (centroids fp32 [M, 256, d / M], codes: read-only memmap uint8 [ntotal, M], is_trained).  offset: where the record starts; it runs to
    `end` (default: the end of the file)."""
    size = _end(fname, end) - offset
    fixed = _HEADER.size + _PQ.size + 8
    if size < fixed:
        raise ValueError(f"{fname}: too short for a product-quantiser index header")
    with open(fname, "rb") as f:
        f.seek(offset)
        d, ntotal, trained, metric = _read_header(f, fname, FOURCC_PQ, "a product-quantiser index")
        pq_d, M, nbits = _PQ.unpack(f.read(_PQ.size))
        if nbits != 8:
            raise ValueError(f"{fname}: ProductQuantizer nbits={nbits} is not served (only 8)")
        if metric != 0 or d <= 0 or ntotal < 0 or pq_d != d or M <= 0 or d % M:
            raise ValueError(f"{fname}: inconsistent IndexPQ header (d={d}, ntotal={ntotal}, pq.d={pq_d}, M={M}, metric={metric})")
        (n_c,) = struct.unpack("<Q", f.read(8))
        if n_c != d * 256 or size < fixed + 4 * n_c + 8:
            raise ValueError(f"{fname}: truncated or inconsistent centroids ({n_c} floats, expected {d * 256})")
        cent = np.frombuffer(f.read(4 * n_c), dtype="<f4").reshape(M, 256, d // M).copy()
        (n_b,) = struct.unpack("<Q", f.read(8))
        off = fixed + 4 * n_c + 8
        if n_b != ntotal * M or size != off + n_b + _PQ_TAIL.size:
            raise ValueError(f"{fname}: inconsistent IndexPQ codes (code bytes={n_b}, ntotal * M={ntotal * M}, file bytes={size})")
        f.seek(offset + off + n_b)
        search_type, _, _ = _PQ_TAIL.unpack(f.read(_PQ_TAIL.size))
    if search_type != 0:
        raise ValueError(f"{fname}: IndexPQ search_type {search_type} is not served (only ST_PQ = 0)")
    codes = np.memmap(fname, dtype=np.uint8, mode="r", offset=offset + off, shape=(ntotal, M)) if ntotal else np.zeros((0, M), np.uint8)
    return cent, codes, bool(trained)


FOURCC_BINARY_FLAT = b"IBxF"
_BIN_HEADER = struct.Struct("<4siiqBi")  # fourcc, d (bits), code_size, ntotal, is_trained, metric_type  (25 bytes, packed)
BIN_HEADER_BYTES = _BIN_HEADER.size + 8  # + u64 vector size


def write_binary_flat(fname: str, blocks: Iterable[np.ndarray], d: int, ntotal: int) -> None:
    """blocks: uint8 [n_i, d / 8] arrays of packed rows in row order, sum n_i == ntotal.  (The binary header has no dummies and carries
    code_size.)"""
    if d <= 0 or d % 8:
        raise ValueError(f"write_binary_flat: d={d} (bits) must be a positive multiple of 8")
    head = _BIN_HEADER.pack(FOURCC_BINARY_FLAT, d, d // 8, ntotal, 1, 1) + struct.pack("<Q", ntotal * (d // 8))
    _write_index(fname, "write_binary_flat", ntotal, head, blocks, np.uint8, d // 8, "code_size")


def read_binary_flat(fname: str) -> np.ndarray:
    """-> read-only memmap uint8 [ntotal, d / 8] of the packed rows (no copy)."""
    size = os.path.getsize(fname)
    if size < BIN_HEADER_BYTES:
        raise ValueError(f"{fname}: too short for a binary flat index header")
    with open(fname, "rb") as f:
        got, d, cs, ntotal, _, _ = _BIN_HEADER.unpack(f.read(_BIN_HEADER.size))
        (n_bytes,) = struct.unpack("<Q", f.read(8))
    if got != FOURCC_BINARY_FLAT:
        raise ValueError(f"{fname}: fourcc {got!r} is not a binary flat index ({FOURCC_BINARY_FLAT.decode()!r})")
    if d <= 0 or d % 8 or cs * 8 != d or ntotal < 0 or n_bytes != ntotal * cs or size != BIN_HEADER_BYTES + n_bytes:
        raise ValueError(f"{fname}: inconsistent binary flat index (d={d}, code_size={cs}, ntotal={ntotal}, code bytes={n_bytes}, file bytes={size})")
    if ntotal == 0:
        return np.zeros((0, cs), np.uint8)
    return np.memmap(fname, dtype=np.uint8, mode="r", offset=BIN_HEADER_BYTES, shape=(ntotal, cs))


FOURCC_PRE_TRANSFORM = b"IxPT"
FOURCC_PCA = b"PcAm"
_PCA = struct.Struct("<4sffBi")          # fourcc, eigen_power, epsilon, random_rotation, balanced_bins  (17 bytes, packed)
_VT_TAIL = struct.Struct("<iiB")         # d_in, d_out, is_trained (9 bytes, packed)
_PCA_VECTORS = ("mean", "eigenvalues", "PCAMat", "A", "b")


def pre_transform_prefix(pca: dict, ntotal: int, is_trained: bool = True) -> bytes:
    """The bytes of an 'IxPT' record up to its base index.  pca: d_in, d_out, eigen_power, random_rotation, is_trained and the fp32 arrays
    mean [d_in], eigenvalues [d_in], PCAMat [d_in, d_in], A [d_out, d_in], b [d_out] (all empty for an untrained transform)."""
    d_in, d_out = int(pca["d_in"]), int(pca["d_out"])
    want = dict(mean=d_in, eigenvalues=d_in, PCAMat=d_in * d_in, A=d_out * d_in, b=d_out)
    vec = {}
    for name in _PCA_VECTORS:
        v = np.ascontiguousarray(pca[name], dtype="<f4").reshape(-1)
        if v.size != (want[name] if pca["is_trained"] else 0):
            raise ValueError(f"write_pre_transform: {name} holds {v.size} floats, expected {want[name] if pca['is_trained'] else 0}")
        vec[name] = struct.pack("<Q", v.size) + v.tobytes()
    return (_index_header(FOURCC_PRE_TRANSFORM, d_in, ntotal, is_trained) + struct.pack("<i", 1)
            + _PCA.pack(FOURCC_PCA, float(pca["eigen_power"]), 0.0, int(bool(pca["random_rotation"])), 0)
            + vec["mean"] + vec["eigenvalues"] + vec["PCAMat"] + struct.pack("<B", 1) + vec["A"] + vec["b"]
            + _VT_TAIL.pack(d_in, d_out, int(bool(pca["is_trained"]))))


def write_pre_transform(fname: str, pca: dict, ntotal: int, is_trained: bool, write_base, prefix: bytes = b"") -> None:
    """An 'IxPT' file: the transform (see pre_transform_prefix), then the base index, written by `write_base(fname, prefix)` -- the writer of
    the base's class (write_flat_ip, write_sq_fp16, write_sq8, write_pq) with the bytes that precede its record.  prefix: bytes that precede
    the 'IxPT' record itself."""
    write_base(fname, prefix + pre_transform_prefix(pca, ntotal, is_trained))


def read_pre_transform(fname: str, offset: int = 0, end: Optional[int] = None):
    """-> (pca, base): pca as pre_transform_prefix takes it; base = dict(offset, fourcc, qtype, d, ntotal, is_trained): where the base index
    record starts, its fourcc ('IxFI', 'IxSQ' or 'IxPq'; qtype: the ScalarQuantizer type of an 'IxSQ' record, else None) and the header of the
    'IxPT' record.  The caller reads the base with the reader of its class at `offset` (and the same `end`).  offset / end: where the 'IxPT'
    record starts and stops (default: the whole file)."""
    size = _end(fname, end)
    with open(fname, "rb") as f:
        f.seek(offset)

        def take(n: int, what: str) -> bytes:
            b = f.read(n) if f.tell() + n <= size else b""
            if len(b) != n:
                raise ValueError(f"{fname}: truncated pre-transform index ({what})")
            return b

        fourcc, d, ntotal, _, _, is_trained, metric = _HEADER.unpack(take(_HEADER.size, "index header"))
        if fourcc != FOURCC_PRE_TRANSFORM:
            raise ValueError(f"{fname}: fourcc {fourcc!r} is not a pre-transform index ({FOURCC_PRE_TRANSFORM.decode()!r})")
        (nchain,) = struct.unpack("<i", take(4, "chain length"))
        if nchain != 1:
            raise ValueError(f"{fname}: a chain of {nchain} transforms is not served (only one PCAMatrix)")
        tcc, eigen_power, epsilon, rr, bins = _PCA.unpack(take(_PCA.size, "transform header"))
        if tcc != FOURCC_PCA:
            raise ValueError(f"{fname}: transform {tcc!r} is not served (only PCAMatrix {FOURCC_PCA.decode()!r}; the legacy 'PCAm' record has no epsilon)")
        if epsilon != 0 or bins != 0:
            raise ValueError(f"{fname}: PCAMatrix epsilon={epsilon} / balanced_bins={bins} are not served (only 0)")
        pca = dict(eigen_power=eigen_power, random_rotation=bool(rr))
        for name in _PCA_VECTORS:
            if name == "A" and take(1, "have_bias") != b"\x01":
                raise ValueError(f"{fname}: a PCAMatrix without bias is not served")
            (n,) = struct.unpack("<Q", take(8, name))
            if f.tell() + 4 * n > size:
                raise ValueError(f"{fname}: truncated pre-transform index ({name}: {n} floats)")
            pca[name] = np.frombuffer(take(4 * n, name), dtype="<f4").copy()
        d_in, d_out, t_trained = _VT_TAIL.unpack(take(_VT_TAIL.size, "transform dimensions"))
        offset = f.tell()
        sub = take(4, "base index")
    want = dict(mean=d_in, eigenvalues=d_in, PCAMat=d_in * d_in, A=d_out * d_in, b=d_out)
    sizes = {name: pca[name].size for name in _PCA_VECTORS}
    if metric != 0 or d != d_in or not 0 < d_out <= d_in or ntotal < 0 or sizes != (want if t_trained else dict.fromkeys(want, 0)):
        raise ValueError(f"{fname}: inconsistent pre-transform index (d={d}, d_in={d_in}, d_out={d_out}, ntotal={ntotal}, metric={metric}, "
                         f"trained={t_trained}, floats={sizes})")
    if t_trained:
        pca["PCAMat"], pca["A"] = pca["PCAMat"].reshape(d_in, d_in), pca["A"].reshape(d_out, d_in)
    pca.update(d_in=d_in, d_out=d_out, is_trained=bool(t_trained))
    if sub not in (FOURCC_FLAT_IP, FOURCC_SQ, FOURCC_PQ):
        raise ValueError(f"{fname}: base index {sub!r} is not served ('IxFI', 'IxSQ', 'IxPq')")
    qtype = sq_qtype(fname, offset, end) if sub == FOURCC_SQ else None
    return pca, dict(offset=offset, fourcc=sub, qtype=qtype, d=d, ntotal=ntotal, is_trained=bool(is_trained))


FOURCC_REFINE = b"IxRF"
FOURCC_IVF_PQ = b"IwPQ"
FOURCC_IVF_SQ = b"IwSq"
_REFINE_BASES = (FOURCC_PQ, FOURCC_SQ, FOURCC_PRE_TRANSFORM, FOURCC_IVF_PQ, FOURCC_IVF_SQ)


def refine_prefix(d: int, ntotal: int, is_trained: bool = True) -> bytes:
    """The bytes of an 'IxRF' record up to its base index."""
    return _index_header(FOURCC_REFINE, d, ntotal, is_trained)


def peek_index_header(fname: str, offset: int = 0, end: Optional[int] = None):
    """-> (fourcc, d, ntotal, is_trained, metric_type) of the index record that starts at `offset`; ValueError when fewer bytes are left."""
    if _end(fname, end) - offset < _HEADER.size:
        raise ValueError(f"{fname}: truncated index record at byte {offset}")
    with open(fname, "rb") as f:
        f.seek(offset)
        fourcc, d, ntotal, _, _, trained, metric = _HEADER.unpack(f.read(_HEADER.size))
    return fourcc, d, ntotal, bool(trained), metric


def index_record_end(fname: str, offset: int = 0, end: Optional[int] = None) -> int:
    """Where the 'IxFI', 'IxSQ', 'IxPq', 'IxPT', 'IwPQ' or 'IwSq' record that starts at `offset` stops, from its own size words; ValueError when that is past
    `end` (default: the end of the file) or the record is of another type.  The reader of the record's class then validates it against
    [offset, the returned end)."""
    size = _end(fname, end)
    fourcc = peek_index_header(fname, offset, end)[0]
    if fourcc == FOURCC_PRE_TRANSFORM:
        return index_record_end(fname, read_pre_transform(fname, offset, end)[1]["offset"], end)
    if fourcc in _IVF_BASES:
        with open(fname, "rb") as f:
            f.seek(offset)
            st, _, code_size, data = _read_ivf_head(f, fname, size - offset, _IVF_BASES[fourcc], served="any")
        return offset + data + st["ntotal"] * (code_size + 8)
    if fourcc not in (FOURCC_FLAT_IP, FOURCC_SQ, FOURCC_PQ):
        raise ValueError(f"{fname}: index record {fourcc!r} at byte {offset} is not served ('IxFI', 'IxSQ', 'IxPq', 'IxPT', 'IwPQ', 'IwSq')")
    with open(fname, "rb") as f:
        pos = offset + _HEADER.size + {FOURCC_FLAT_IP: 0, FOURCC_SQ: _SQ.size, FOURCC_PQ: _PQ.size}[fourcc]
        # the vectors that follow: (bytes per element, ...) -- each a u64 count and its elements
        for width in {FOURCC_FLAT_IP: (4,), FOURCC_SQ: (4, 1), FOURCC_PQ: (4, 1)}[fourcc]:
            f.seek(pos)
            word = f.read(8) if pos + 8 <= size else b""
            if len(word) != 8:
                raise ValueError(f"{fname}: truncated index record {fourcc!r} at byte {offset}")
            pos += 8 + width * struct.unpack("<Q", word)[0]
    pos += _PQ_TAIL.size if fourcc == FOURCC_PQ else 0
    if pos > size:
        raise ValueError(f"{fname}: truncated index record {fourcc!r} at byte {offset} (it needs {pos - offset} bytes, {size - offset} are left)")
    return pos


def write_refine(fname: str, d: int, ntotal: int, is_trained: bool, k_factor: float, write_base, write_store) -> None:
    """An 'IxRF' file: the header, the base index written by `write_base(fname, prefix)`, the refine index appended by `write_store(fname)` --
    the savers of the two indexes, the second one continuing the file -- and k_factor; built as fname.tmp and renamed over fname."""
    tmp = fname + ".tmp"
    write_base(tmp, refine_prefix(d, ntotal, is_trained))
    write_store(tmp)
    with open(tmp, "ab") as f:
        f.write(struct.pack("<f", float(k_factor)))
    os.replace(tmp, fname)


def read_refine(fname: str):
    """-> dict(d, ntotal, is_trained, k_factor, base, store); base / store = dict(offset, end, fourcc, qtype): where each record lies, its
    fourcc (base: 'IxPq', 'IxSQ', 'IxPT', 'IwPQ' or 'IwSq'; store: 'IxFI', or 'IxSQ' with qtype QT_fp16) and the ScalarQuantizer type of an 'IxSQ' record
    (else None).  The caller reads each with the reader of its class at (offset, end)."""
    size = os.path.getsize(fname)
    if size < _HEADER.size + 4:
        raise ValueError(f"{fname}: too short for a refine index")
    fourcc, d, ntotal, is_trained, metric = peek_index_header(fname)
    if fourcc != FOURCC_REFINE:
        raise ValueError(f"{fname}: fourcc {fourcc!r} is not a refine index ({FOURCC_REFINE.decode()!r})")
    if metric != 0 or d <= 0 or ntotal < 0:
        raise ValueError(f"{fname}: inconsistent refine index header (d={d}, ntotal={ntotal}, metric={metric})")
    body_end = size - 4
    parts, pos = [], _HEADER.size
    for what, served in (("base", _REFINE_BASES), ("refine", (FOURCC_FLAT_IP, FOURCC_SQ))):
        cc, sub_d, sub_n, _, _ = peek_index_header(fname, pos, body_end)
        if cc not in served:
            raise ValueError(f"{fname}: {what} index {cc!r} is not served ({', '.join(repr(c.decode()) for c in served)})")
        if sub_d != d or sub_n != ntotal:
            raise ValueError(f"{fname}: the refine header says d={d}, ntotal={ntotal}; its {what} index d={sub_d}, ntotal={sub_n}")
        stop = index_record_end(fname, pos, body_end)
        qtype = sq_qtype(fname, pos, stop) if cc == FOURCC_SQ else None
        parts.append(dict(offset=pos, end=stop, fourcc=cc, qtype=qtype))
        pos = stop
    if parts[1]["fourcc"] == FOURCC_SQ and parts[1]["qtype"] != QT_FP16:
        raise ValueError(f"{fname}: refine index with ScalarQuantizer qtype {parts[1]['qtype']} is not served (only QT_fp16 = {QT_FP16})")
    if pos != body_end:
        raise ValueError(f"{fname}: {body_end - pos} bytes between the refine index and k_factor")
    with open(fname, "rb") as f:
        f.seek(body_end)
        (k_factor,) = struct.unpack("<f", f.read(4))
    return dict(d=d, ntotal=ntotal, is_trained=is_trained, k_factor=k_factor, base=parts[0], store=parts[1])


FOURCC_IVF_FLAT = b"IwFl"
_ILAR, _FULL, _SPRS = b"ilar", b"full", b"sprs"

# ---- the inverted-file records: one preamble, one family-specific middle, one 'ilar' record and the cells, written and read once ----------


class _IVFFamily(NamedTuple):
    """What one inverted-file record has of its own: its fourcc, the words its messages differ in, and the reader of its middle."""
    fourcc: bytes
    noun: str          # "truncated <noun> (...)", "too short for an <noun> header", "the flat quantiser of an <noun>"
    what: str          # _read_header's name for the record
    middle: Callable   # (take, fname, d, served) -> (the family's fields, code_size, what code_size follows from)
    sum_tail: str      # closes "the list sizes sum to ..."
    unfilled: str      # the record's length is not that of its cells


def _ivf_write_args(who: str, centroids, list_sizes, row_ids):
    """The arguments every inverted-file writer takes -> (sizes int64 [nlist], ids <i8 [n], centroids <f4 [nlist or 0, d], d, ntotal)."""
    sizes = np.asarray(list_sizes, dtype=np.int64).reshape(-1)
    nlist, ntotal = sizes.shape[0], int(sizes.sum())
    ids = np.ascontiguousarray(row_ids, dtype="<i8").reshape(-1)
    cent = np.ascontiguousarray(centroids, dtype="<f4")
    if cent.ndim != 2 or cent.shape[0] not in (0, nlist) or nlist < 1:
        raise ValueError(f"{who}: centroids {cent.shape} do not match nlist={nlist}")
    return sizes, ids, cent, cent.shape[1], ntotal


def _ivf_preamble_bytes(fourcc: bytes, cent: np.ndarray, sizes: np.ndarray, nprobe: int, is_trained: bool) -> bytes:
    """An inverted-file record up to its family's own fields: index header, nlist, nprobe, the 'IxFI' quantiser, the empty direct map."""
    d = cent.shape[1]
    return (_index_header(fourcc, d, int(sizes.sum()), is_trained) + struct.pack("<QQ", sizes.shape[0], int(nprobe))
            + _index_header(FOURCC_FLAT_IP, d, cent.shape[0]) + struct.pack("<Q", cent.size) + cent.tobytes()
            + struct.pack("<BQ", 0, 0))                                # direct map: NoMap, empty array


def _list_sizes_bytes(sizes: np.ndarray) -> bytes:
    """The list sizes of an 'ilar' record: 'full' when more than nlist / 2 cells are non-empty (faiss's rule), 'sprs' otherwise."""
    nlist = sizes.shape[0]
    non0 = np.flatnonzero(sizes)
    if len(non0) > nlist // 2:
        return _FULL + struct.pack("<Q", nlist) + sizes.astype("<u8").tobytes()
    return _SPRS + struct.pack("<Q", 2 * len(non0)) + np.stack([non0, sizes[non0]], axis=1).astype("<u8").tobytes()


def _ilar_bytes(sizes: np.ndarray, code_size: int) -> bytes:
    return _ILAR + struct.pack("<QQ", sizes.shape[0], code_size) + _list_sizes_bytes(sizes)


def _write_ivf_cells(fname: str, head: bytes, sizes: np.ndarray, cell_bytes, ids: np.ndarray, prefix: bytes = b"", append: bool = False) -> None:
    """`prefix`, `head` (the record up to and including its list sizes), then for every non-empty cell the bytes of its rows --
    cell_bytes(a, b) for the stored positions [a, b), called one cell at a time -- and its ids; to a .tmp file renamed over fname, or
    (`append`) continuing the existing file fname, as in _write_index."""
    tmp = fname if append else fname + ".tmp"
    off = np.concatenate([[0], np.cumsum(sizes)])
    with open(tmp, "ab" if append else "wb") as f:
        f.write(prefix)
        f.write(head)
        for c in np.flatnonzero(sizes):
            a, b = int(off[c]), int(off[c + 1])
            f.write(cell_bytes(a, b))
            f.write(ids[a:b].tobytes())
    if not append:
        os.replace(tmp, fname)


def _read_ivf_preamble(f, take, fname: str, size: int, fam: _IVFFamily):
    """An inverted-file record from its index header through its direct map -> (d, ntotal, is_trained, nlist, nprobe, centroids)."""
    if size < 2 * _HEADER.size + 16:
        raise ValueError(f"{fname}: too short for an {fam.noun} header")
    d, ntotal, is_trained, metric = _read_header(f, fname, fam.fourcc, fam.what)
    nlist, nprobe = struct.unpack("<QQ", take(16, "nlist, nprobe"))
    if metric != 0 or d <= 0 or ntotal < 0 or nlist < 1:
        raise ValueError(f"{fname}: inconsistent {fam.noun} header (d={d}, ntotal={ntotal}, nlist={nlist}, metric={metric})")
    qd, qn, _, qmetric = _read_header(f, fname, FOURCC_FLAT_IP, f"the flat quantiser of an {fam.noun}")
    (n_floats,) = struct.unpack("<Q", take(8, "quantiser size"))
    if qd != d or qn not in (0, nlist) or n_floats != qn * d or qmetric != 0:
        raise ValueError(f"{fname}: the quantiser (d={qd}, ntotal={qn}, floats={n_floats}) does not match d={d}, nlist={nlist}")
    centroids = np.frombuffer(take(4 * n_floats, "centroids"), dtype="<f4").reshape(qn, d)
    dm_type, dm_n = struct.unpack("<BQ", take(9, "direct map"))
    if dm_type != 0 or dm_n != 0:
        raise ValueError(f"{fname}: direct map type {dm_type} with {dm_n} entries is not served (only NoMap)")
    return d, ntotal, is_trained, nlist, nprobe, centroids


def _read_ilar(take, fname: str, nlist: int, ntotal: int, code_size: int, versus: str, sum_tail: str = "") -> np.ndarray:
    """The 'ilar' record up to its list sizes, 'full' or 'sprs' -> sizes int64 [nlist], which sum to ntotal.  versus: what code_size follows
    from, for the message ("d=32", "M=8")."""
    il = take(4, "inverted lists")
    if il != _ILAR:
        raise ValueError(f"{fname}: inverted lists {il!r} are not served (only {_ILAR.decode()!r})")
    il_nlist, il_code = struct.unpack("<QQ", take(16, "inverted lists header"))
    if il_nlist != nlist or il_code != code_size:
        raise ValueError(f"{fname}: inverted lists of nlist={il_nlist}, code_size={il_code} do not match nlist={nlist}, {versus}")
    form = take(4, "list sizes")
    (n_words,) = struct.unpack("<Q", take(8, "list sizes"))
    sizes = np.zeros(nlist, dtype=np.int64)
    if form == _FULL:
        if n_words != nlist:
            raise ValueError(f"{fname}: {n_words} list sizes for nlist={nlist}")
        sizes[:] = np.frombuffer(take(8 * nlist, "list sizes"), dtype="<u8")
    elif form == _SPRS:
        pairs = np.frombuffer(take(8 * n_words, "list sizes"), dtype="<u8").reshape(-1, 2).astype(np.int64) if n_words % 2 == 0 else None
        if pairs is None or (pairs[:, 0] >= nlist).any() or len(np.unique(pairs[:, 0])) != len(pairs):
            raise ValueError(f"{fname}: inconsistent sparse list sizes")
        sizes[pairs[:, 0]] = pairs[:, 1]
    else:
        raise ValueError(f"{fname}: list-size form {form!r} is not served (only {_FULL.decode()!r} and {_SPRS.decode()!r})")
    if int(sizes.sum()) != ntotal:
        raise ValueError(f"{fname}: the list sizes sum to {int(sizes.sum())}, the header says ntotal={ntotal}{sum_tail}")
    return sizes


def _read_ivf_cells(f, sizes: np.ndarray, dtype, width: int):
    """The cells from the file position, one read per cell -> (list_off int64 [nlist + 1], rows `dtype` [ntotal, width] in cell order,
    row_ids int64 [ntotal])."""
    dtype = np.dtype(dtype)
    list_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.empty((int(list_off[-1]), width), dtype=dtype.newbyteorder("="))
    row_ids = np.empty(int(list_off[-1]), dtype=np.int64)
    for c in np.flatnonzero(sizes):
        a, b = int(list_off[c]), int(list_off[c + 1])
        rows[a:b] = np.frombuffer(f.read((b - a) * width * dtype.itemsize), dtype=dtype).reshape(b - a, width)
        row_ids[a:b] = np.frombuffer(f.read((b - a) * 8), dtype="<i8")
    return list_off, rows, row_ids


def _read_ivf_pq_middle(take, fname: str, d: int, served):
    """'IwPQ' between the direct map and 'ilar': by_residual, code_size, the ProductQuantizer."""
    by_residual, code_size = struct.unpack("<BQ", take(9, "by_residual, code_size"))
    pq_d, M, nbits = _PQ.unpack(take(_PQ.size, "product quantiser"))
    if nbits != 8:
        raise ValueError(f"{fname}: ProductQuantizer nbits={nbits} is not served (only 8)")
    (n_c,) = struct.unpack("<Q", take(8, "codebook size"))
    if pq_d != d or M <= 0 or d % M or code_size != M or n_c != d * 256 or by_residual not in (0, 1):
        raise ValueError(f"{fname}: inconsistent IndexIVFPQ quantiser (pq.d={pq_d}, M={M}, code_size={code_size}, floats={n_c}, by_residual={by_residual}; d={d})")
    pq_centroids = np.frombuffer(take(4 * n_c, "codebooks"), dtype="<f4").reshape(M, 256, d // M)
    return dict(by_residual=bool(by_residual), M=int(M), pq_centroids=pq_centroids), int(M), f"M={M}"


def _read_ivf_sq_middle(take, fname: str, d: int, served: str):
    """'IwSq' between the direct map and 'ilar': the ScalarQuantizer, `trained`, code_size, by_residual.  served: "fp16" (read_ivf_sq: QT_fp16
    alone), "8bit" (read_ivf_sq8: QT_8bit / QT_8bit_uniform) or "any" (index_record_end: the three of them)."""
    qtype, _, _, sq_d, sq_code = _SQ.unpack(take(_SQ.size, "scalar quantiser"))
    if served == "8bit" and qtype == QT_FP16:
        raise ValueError(f"{fname}: ScalarQuantizer qtype {qtype} (QT_fp16) is not an 8-bit record: read it with read_ivf_sq (IVFSQIndex)")
    if served != "fp16" and qtype not in (QT_FP16, QT_8BIT, QT_8BIT_UNIFORM):
        raise ValueError(f"{fname}: ScalarQuantizer qtype {qtype} is not served over cells (only QT_8bit = {QT_8BIT}, QT_8bit_uniform = "
                         f"{QT_8BIT_UNIFORM} and QT_fp16 = {QT_FP16})")
    if served == "fp16" and qtype != QT_FP16:
        raise ValueError(f"{fname}: ScalarQuantizer qtype {qtype} is not served over cells (only QT_fp16 = {QT_FP16})")
    (n_trained,) = struct.unpack("<Q", take(8, "trained size"))
    want_code, want_trained = (2 * d, 0) if qtype == QT_FP16 else (d, _sq8_trained_len(qtype, d))
    if sq_d != d or sq_code != want_code or n_trained != want_trained:
        raise ValueError(f"{fname}: inconsistent IndexIVFScalarQuantizer quantiser (sq.d={sq_d}, sq.code_size={sq_code}, trained={n_trained}, "
                         f"qtype={qtype}; d={d})")
    trained = np.frombuffer(take(4 * n_trained, "trained"), dtype="<f4").copy()
    code_size, by_residual = struct.unpack("<QB", take(9, "code_size, by_residual"))
    if code_size != want_code or by_residual not in (0, 1):
        raise ValueError(f"{fname}: inconsistent IndexIVFScalarQuantizer quantiser (sq.d={sq_d}, sq.code_size={sq_code}, trained={n_trained}, "
                         f"code_size={code_size}, by_residual={by_residual}; d={d})")
    return dict(by_residual=bool(by_residual), qtype=int(qtype), trained=trained), int(want_code), f"d={d}"


_ROWS_UNFILLED = "{fname}: {ntotal} rows of {code_size} + 8 bytes do not fill the record (bytes={size})"
_IVF_FLAT = _IVFFamily(FOURCC_IVF_FLAT, "inverted-file index", "an inverted-file flat index", lambda take, fname, d, served: ({}, 4 * d, f"d={d}"),
                       " (file bytes={size})", "{fname}: the list sizes sum to {ntotal}, the header says ntotal={ntotal} (file bytes={size})")
_IVF_PQ = _IVFFamily(FOURCC_IVF_PQ, "inverted-file PQ index", "an inverted-file product-quantiser index", _read_ivf_pq_middle, "", _ROWS_UNFILLED)
_IVF_SQ = _IVFFamily(FOURCC_IVF_SQ, "inverted-file scalar-quantiser index", "an inverted-file scalar-quantiser index", _read_ivf_sq_middle, "",
                     _ROWS_UNFILLED)
_IVF_BASES = {fam.fourcc: fam for fam in (_IVF_PQ, _IVF_SQ)}      # the records index_record_end knows: a refine index can hold them as its base


def _read_ivf_head(f, fname: str, size: int, fam: _IVFFamily, served: Optional[str] = None):
    """An inverted-file record from the file position up to its list sizes (`size`: the bytes the record may fill) -> (dict(d, nlist, nprobe,
    ntotal, is_trained, the family's fields, centroids), sizes, code_size, the record's bytes before the first cell's rows)."""
    start = f.tell()

    def take(n: int, what: str) -> bytes:
        b = f.read(n) if f.tell() - start + n <= size else b""
        if len(b) != n:
            raise ValueError(f"{fname}: truncated {fam.noun} ({what})")
        return b
    d, ntotal, is_trained, nlist, nprobe, centroids = _read_ivf_preamble(f, take, fname, size, fam)
    fields, code_size, versus = fam.middle(take, fname, d, served)
    sizes = _read_ilar(take, fname, nlist, ntotal, code_size, versus, fam.sum_tail.format(size=size))
    st = dict(d=d, nlist=int(nlist), nprobe=int(nprobe), ntotal=ntotal, is_trained=bool(is_trained), **fields, centroids=centroids)
    return st, sizes, code_size, f.tell() - start


def _read_ivf(fname: str, fam: _IVFFamily, dtype, rows_key: str, offset: int = 0, end: Optional[int] = None, served: Optional[str] = None) -> dict:
    """The record at [offset, end) (default: to the end of the file), which it must fill exactly -> _read_ivf_head's dict with list_off, the
    rows (`dtype`, under rows_key) and row_ids of _read_ivf_cells."""
    size = _end(fname, end) - offset
    with open(fname, "rb") as f:
        f.seek(offset)
        st, sizes, code_size, data = _read_ivf_head(f, fname, size, fam, served)
        if data + st["ntotal"] * (code_size + 8) != size:
            raise ValueError(fam.unfilled.format(fname=fname, ntotal=st["ntotal"], code_size=code_size, size=size))
        st["list_off"], st[rows_key], st["row_ids"] = _read_ivf_cells(f, sizes, dtype, code_size // np.dtype(dtype).itemsize)
    return st


def write_ivf_flat(fname: str, centroids: np.ndarray, list_sizes, rows, row_ids, nprobe: int = 1, is_trained: bool = True) -> None:
    """centroids fp32 [nlist, d] ([0, d] when untrained); list_sizes [nlist]; rows: the fp32 rows in CELL ORDER, anything whose slice
    rows[a:b] np.asarray turns into [b - a, d] (read one cell at a time: the index comes off the GPU in pieces); row_ids int64 [ntotal], the
    original row (faiss's id) of each stored position.  Written as faiss's 'IwFl' record (the layout at the head of this file; faiss is not
    installed here, so the bytes are unverified against a Faiss build).  Built as fname.tmp and renamed over fname."""
    sizes, ids, cent, d, ntotal = _ivf_write_args("write_ivf_flat", centroids, list_sizes, row_ids)
    if ids.shape[0] != ntotal or (sizes < 0).any():
        raise ValueError(f"write_ivf_flat: {ids.shape[0]} row ids, the list sizes sum to {ntotal}")

    def cell_bytes(a: int, b: int) -> bytes:
        block = np.ascontiguousarray(np.asarray(rows[a:b]), dtype="<f4")
        if block.shape != (b - a, d):
            raise ValueError(f"write_ivf_flat: rows[{a}:{b}] has shape {block.shape}, expected {(b - a, d)}")
        return block.tobytes()
    _write_ivf_cells(fname, _ivf_preamble_bytes(FOURCC_IVF_FLAT, cent, sizes, nprobe, is_trained) + _ilar_bytes(sizes, 4 * d), sizes, cell_bytes, ids)


def read_ivf_flat(fname: str):
    """-> dict(d, nlist, nprobe, ntotal, is_trained, centroids fp32 [nlist, d] ([0, d] when untrained), list_off int64 [nlist + 1], rows fp32
    [ntotal, d] in cell order, row_ids int64 [ntotal]).  Both list-size forms ('full', 'sprs') are read; anything else is refused by name."""
    return _read_ivf(fname, _IVF_FLAT, "<f4", "rows")


def write_ivf_pq(fname: str, centroids: np.ndarray, pq_centroids: np.ndarray, list_sizes, codes, row_ids, nprobe: int = 1, by_residual: bool = True,
                 is_trained: bool = True, prefix: bytes = b"", append: bool = False) -> None:
    """centroids fp32 [nlist, d] ([0, d] when untrained); pq_centroids fp32 [M, 256, d / M]; list_sizes [nlist]; codes uint8 [ntotal, M]
    row-major in CELL ORDER; row_ids int64 [ntotal], the original row (faiss's id) of each stored position.  Written as faiss's 'IwPQ' record
    (the layout at the head of this file; faiss is not installed here, so the bytes are unverified against a Faiss build).  Built as
    fname.tmp and renamed over fname; `prefix` / `append` as in _write_index (the enclosing record of write_refine)."""
    sizes, ids, cent, d, ntotal = _ivf_write_args("write_ivf_pq", centroids, list_sizes, row_ids)
    pqc = np.ascontiguousarray(pq_centroids, dtype="<f4")
    if pqc.ndim != 3 or pqc.shape[1] != 256 or pqc.shape[0] * pqc.shape[2] != d:
        raise ValueError(f"write_ivf_pq: codebooks {pqc.shape} are not [M, 256, d / M] for d={d}")
    M = pqc.shape[0]
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if ids.shape[0] != ntotal or (sizes < 0).any() or codes.shape != (ntotal, M):
        raise ValueError(f"write_ivf_pq: {ids.shape[0]} row ids and codes {codes.shape}, the list sizes sum to {ntotal} (M={M})")
    head = _ivf_preamble_bytes(FOURCC_IVF_PQ, cent, sizes, nprobe, is_trained)
    head += struct.pack("<BQ", int(bool(by_residual)), M)              # by_residual, code_size
    head += _PQ.pack(d, M, 8) + struct.pack("<Q", pqc.size) + pqc.tobytes()
    _write_ivf_cells(fname, head + _ilar_bytes(sizes, M), sizes, lambda a, b: codes[a:b].tobytes(), ids, prefix, append)


def read_ivf_pq(fname: str, offset: int = 0, end: Optional[int] = None):
    """-> dict(d, nlist, nprobe, ntotal, is_trained, by_residual, M, centroids fp32 [nlist, d] ([0, d] when untrained), pq_centroids fp32
    [M, 256, d / M], list_off int64 [nlist + 1], codes uint8 [ntotal, M] in cell order, row_ids int64 [ntotal]).  offset: where the record starts;
    it runs to `end` (default: the end of the file).  Both list-size forms ('full', 'sprs') are read; anything else is refused by name."""
    return _read_ivf(fname, _IVF_PQ, np.uint8, "codes", offset, end)


def write_ivf_sq(fname: str, centroids: np.ndarray, list_sizes, codes, row_ids, nprobe: int = 1, by_residual: bool = True, is_trained: bool = True,
                 prefix: bytes = b"", append: bool = False) -> None:
    """centroids fp32 [nlist, d] ([0, d] when untrained); list_sizes [nlist]; codes fp16 [ntotal, d] row-major in CELL ORDER; row_ids int64
    [ntotal], the original row (faiss's id) of each stored position.  Written as faiss's 'IwSq' record (the layout at the head of this file;
    faiss is not installed here, so the bytes are unverified against a Faiss build).  Built as fname.tmp and renamed over fname; `prefix` /
    `append` as in _write_index (the enclosing record of write_refine)."""
    sizes, ids, cent, d, ntotal = _ivf_write_args("write_ivf_sq", centroids, list_sizes, row_ids)
    codes = np.asarray(codes)
    if codes.dtype != np.float16 or ids.shape[0] != ntotal or (sizes < 0).any() or codes.shape != (ntotal, d):
        raise ValueError(f"write_ivf_sq: {ids.shape[0]} row ids and codes {codes.dtype} {codes.shape}, the list sizes sum to {ntotal} (fp16, d={d})")
    codes = np.ascontiguousarray(codes, dtype="<f2")
    head = _ivf_preamble_bytes(FOURCC_IVF_SQ, cent, sizes, nprobe, is_trained)
    head += _SQ.pack(QT_FP16, 0, 0.0, d, 2 * d) + struct.pack("<Q", 0)  # the ScalarQuantizer, its empty `trained`
    head += struct.pack("<QB", 2 * d, int(bool(by_residual)))          # code_size, by_residual
    _write_ivf_cells(fname, head + _ilar_bytes(sizes, 2 * d), sizes, lambda a, b: codes[a:b].tobytes(), ids, prefix, append)


def read_ivf_sq(fname: str, offset: int = 0, end: Optional[int] = None):
    """-> dict(d, nlist, nprobe, ntotal, is_trained, by_residual, centroids fp32 [nlist, d] ([0, d] when untrained), list_off int64 [nlist + 1],
    codes fp16 [ntotal, d] in cell order, row_ids int64 [ntotal]).  offset: where the record starts; it runs to `end` (default: the end of the
    file).  Both list-size forms ('full', 'sprs') are read; another qtype, a direct map and other inverted lists are refused by name."""
    st = _read_ivf(fname, _IVF_SQ, "<f2", "codes", offset, end, served="fp16")
    del st["qtype"], st["trained"]
    return st


def write_ivf_sq8(fname: str, centroids: np.ndarray, trained: np.ndarray, qtype: int, list_sizes, codes, row_ids, nprobe: int = 1, by_residual: bool = True,
                  is_trained: bool = True, prefix: bytes = b"", append: bool = False) -> None:
    """centroids fp32 [nlist, d] ([0, d] when untrained); trained fp32 vmin ++ vdiff (2 d floats for qtype QT_8bit = 0, 2 for QT_8bit_uniform = 2);
    list_sizes [nlist]; codes uint8 [ntotal, d] row-major in CELL ORDER; row_ids int64 [ntotal], the original row (faiss's id) of each stored
    position.  Written as faiss's 'IwSq' record with an 8-bit ScalarQuantizer (the layout at the head of this file; faiss is not installed here,
    so the bytes are unverified against a Faiss build).  Built as fname.tmp and renamed over fname; `prefix` / `append` as in _write_index."""
    sizes, ids, cent, d, ntotal = _ivf_write_args("write_ivf_sq8", centroids, list_sizes, row_ids)
    t = np.ascontiguousarray(trained, dtype="<f4").reshape(-1)
    if t.size != _sq8_trained_len(qtype, d):
        raise ValueError(f"write_ivf_sq8: {t.size} trained floats, expected {_sq8_trained_len(qtype, d)}")
    codes = np.asarray(codes)
    if codes.dtype != np.uint8 or ids.shape[0] != ntotal or (sizes < 0).any() or codes.shape != (ntotal, d):
        raise ValueError(f"write_ivf_sq8: {ids.shape[0]} row ids and codes {codes.dtype} {codes.shape}, the list sizes sum to {ntotal} (uint8, d={d})")
    codes = np.ascontiguousarray(codes)
    head = _ivf_preamble_bytes(FOURCC_IVF_SQ, cent, sizes, nprobe, is_trained)
    head += _SQ.pack(qtype, 0, 0.0, d, d) + struct.pack("<Q", t.size) + t.tobytes()   # the ScalarQuantizer and its `trained`
    head += struct.pack("<QB", d, int(bool(by_residual)))              # code_size, by_residual
    _write_ivf_cells(fname, head + _ilar_bytes(sizes, d), sizes, lambda a, b: codes[a:b].tobytes(), ids, prefix, append)


def read_ivf_sq8(fname: str, offset: int = 0, end: Optional[int] = None):
    """-> dict(d, nlist, nprobe, ntotal, is_trained, by_residual, qtype (0 / 2), trained fp32 [2 d] or [2], centroids fp32 [nlist, d] ([0, d] when
    untrained), list_off int64 [nlist + 1], codes uint8 [ntotal, d] in cell order, row_ids int64 [ntotal]).  offset: where the record starts; it
    runs to `end` (default: the end of the file).  Both list-size forms ('full', 'sprs') are read; another qtype (QT_fp16 = 4: that record is
    read_ivf_sq's), a direct map and other inverted lists are refused by name."""
    return _read_ivf(fname, _IVF_SQ, np.uint8, "codes", offset, end, served="8bit")


def ivf_sq_qtype(fname: str, offset: int = 0, end: Optional[int] = None) -> int:
    """The ScalarQuantizer qtype of an 'IwSq' record (faiss's enum: 0 8bit, 2 8bit_uniform, 4 fp16, ...), as sq_qtype for 'IxSQ': which of
    read_ivf_sq (4) and read_ivf_sq8 (0, 2) the record needs.  The record is read up to its quantiser and no further."""
    size = _end(fname, end) - offset
    with open(fname, "rb") as f:
        f.seek(offset)
        if size < 2 * _HEADER.size + 16 + 8:
            raise ValueError(f"{fname}: too short for an inverted-file scalar-quantiser index header")
        d, _, _, _ = _read_header(f, fname, FOURCC_IVF_SQ, "an inverted-file scalar-quantiser index")
        f.seek(16, 1)                                                     # nlist, nprobe
        _, qn, _, _ = _read_header(f, fname, FOURCC_FLAT_IP, "the flat quantiser of an inverted-file scalar-quantiser index")
        pos = f.tell() - offset + 8 + 4 * max(qn, 0) * max(d, 0) + 9      # the centroids, the direct map
        if pos + 4 > size:
            raise ValueError(f"{fname}: truncated inverted-file scalar-quantiser index (scalar quantiser)")
        f.seek(offset + pos)
        return struct.unpack("<i", f.read(4))[0]


def save_dict_to_tsv(mapping: dict, output_path: str, keys: Optional[list] = None) -> None:
    """retriever/faiss_search.py:28-33."""
    with open(output_path, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t", quoting=csv.QUOTE_MINIMAL)
        if keys:
            w.writerow(keys)
        for k, v in mapping.items():
            w.writerow([k, v])


def load_tsv_to_dict(input_path: str, header: bool = True) -> dict:
    """retriever/faiss_search.py:35-43."""
    out = {}
    with open(input_path, encoding="utf-8", newline="") as f:
        r = csv.reader(f, delimiter="\t", quoting=csv.QUOTE_MINIMAL)
        if header:
            next(r)
        for row in r:
            out[row[0]] = int(row[1])
    return out
