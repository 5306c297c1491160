"""Numpy yardstick of the inverted-file fp16 scalar-quantised index (lightretriever_amd/ivfsq.py, lrx_ivf_sq_fp16_ip_search),
built on ivf_yardstick (cells, k-means, probe lists):

    code    fp16(v), round-to-nearest-even, saturating at +-65504 (a NaN becomes -65504); v = x, or with by_residual fl32(x - centroid[cell])
    score(query i, position p in the probed cell probes[i][j])
            (float)(B + sum_e (double)q_e * (double)(float)code_e),   B = by_residual ? (double)probe_scores[i][j] : 0
            the sum in exact_dot's order: lane `sub` of a half-wave takes elements 4 sub + 128 u + 0..3 of each 2048-element block, fp64
            accumulation, then the xor tree 16, 8, 4, 2, 1
    top-k   score descending, ties to the lower ORIGINAL row, (-FLT_MAX, -1) padding

a brute-force search with that sum, the codes, their decode, an exact rerank of given candidates and the 'IwSq' file written field by field --
for clarity, not speed.  The GPU tests compare the library with it; the CPU tests check it on its own."""
import struct

import numpy as np

import ivf_yardstick as IV

FLT_MAX = np.finfo(np.float32).max
F16_MAX = np.float32(65504.0)


def encode(x, cent=None, cells=None) -> np.ndarray:
    """fp16 [n, d]: the codes of the rows x -- of their residuals to cent[cells] (one fp32 subtraction) when cent is given."""
    v = np.asarray(x, np.float32)
    if cent is not None:
        v = (v - np.asarray(cent, np.float32)[np.asarray(cells, np.int64)]).astype(np.float32)
    v = np.where(np.isnan(v), -F16_MAX, np.clip(v, -F16_MAX, F16_MAX)).astype(np.float32)
    return v.astype(np.float16)                                               # numpy rounds to nearest even, subnormals included


def decode(codes, cent=None, cells=None) -> np.ndarray:
    """fp32 [n, d]: float(code), plus cent[cells] (one fp32 add) when cent is given."""
    v = np.asarray(codes, np.float16).astype(np.float32)
    if cent is not None:
        v = (v + np.asarray(cent, np.float32)[np.asarray(cells, np.int64)]).astype(np.float32)
    return v


def ordered_sums(q, codes) -> np.ndarray:
    """fp64 [n]: sum_e q_e * float(code_e) per code row, added in exact_dot's order (the head of this file).  The products of two fp32
    numbers are exact in fp64, so only the order of the additions matters."""
    q, c = np.asarray(q, np.float32).astype(np.float64), np.asarray(codes, np.float16).astype(np.float64)
    n, d = c.shape
    nb = -(-d // 2048)
    p = np.zeros((n, nb * 2048), np.float64)                                  # (an element past d adds +0.0: the sum is never -0.0)
    p[:, :d] = c * q[None, :]
    p = p.reshape(n, nb, 16, 32, 4)                                           # element = 2048 block + 128 u + 4 sub + e
    term = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]                  # [n, block, u, sub]
    acc = np.zeros((n, 32), np.float64)
    for b in range(nb):
        for u in range(16):
            acc = acc + term[:, b, u, :]
    for o in (16, 8, 4, 2, 1):
        acc = acc + acc[:, np.arange(32) ^ o]
    return acc[:, 0]


def row_scores(q, codes, base=0.0) -> np.ndarray:
    """fp32 [n]: (float)(base + the ordered sum): one rounding.  base: one value, or one per row."""
    if len(codes) == 0:
        return np.zeros(0, np.float32)
    return (np.asarray(base, np.float64) + ordered_sums(q, codes)).astype(np.float32)


def search(q, codes, list_off, row_ids, probes, probe_scores, by_residual, k, id_base=0, row_map=None, max_scan_rows=None):
    """(D f32[Q,k], I i64[Q,k]): per query the positions of the cells probes[i] names (codes fp16 [n, d] stored cell by cell, cell c = positions
    [list_off[c], list_off[c + 1]), row_ids: position -> original row, None = the position; an entry < 0 or >= nlist is skipped, a cell named
    twice counts once, with the base term of its FIRST occurrence), scored as the head of this file says, the best k by score descending, ties
    to the lower ORIGINAL row, (-FLT_MAX, -1) padding.  A query whose cells hold more than max_scan_rows (when given) is all padding.  Ids:
    id_base + row, or row_map[row]."""
    q, codes = np.asarray(q, np.float32), np.asarray(codes, np.float16)
    list_off, probes = np.asarray(list_off, np.int64), np.asarray(probes, np.int64)
    nlist = len(list_off) - 1
    row_ids = np.arange(len(codes), dtype=np.int64) if row_ids is None else np.asarray(row_ids, np.int64)
    Q = q.shape[0]
    D = np.full((Q, k), -FLT_MAX, np.float32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        seen, pos, base = set(), [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
        for j, c in enumerate(probes[i].tolist()):
            if 0 <= c < nlist and c not in seen:
                seen.add(c)
                pos.append(np.arange(list_off[c], list_off[c + 1]))
                base.append(np.full(pos[-1].size, probe_scores[i][j] if by_residual else 0.0, np.float32))
        pos, base = np.concatenate(pos), np.concatenate(base)
        sc, rows = row_scores(q[i], codes[pos], base), row_ids[pos]            # one call for the query: a row's score depends on its own base alone
        if max_scan_rows is not None and rows.size > max_scan_rows:
            continue
        order = np.lexsort((rows, -sc.astype(np.float64)))[:k]
        D[i, :order.size] = sc[order]
        I[i, :order.size] = (id_base + rows[order]) if row_map is None else np.asarray(row_map, np.int64)[rows[order]]
    return D, I


def rerank(q, X, cand, k):
    """(D f32[Q,k], I i64[Q,k]): the candidate rows cand[i] (< 0 skipped) scored exactly over the fp32 rows X (the flat index's score), the best
    k by score descending, ties to the lower row, (-FLT_MAX, -1) padding."""
    q, X, cand = np.asarray(q, np.float32), np.asarray(X, np.float32), np.asarray(cand, np.int64)
    Q = q.shape[0]
    D = np.full((Q, k), -FLT_MAX, np.float32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        rows = cand[i][cand[i] >= 0]
        sc = IV.exact_scores(q[i], X[rows])
        order = np.lexsort((rows, -sc.astype(np.float64)))[:k]
        D[i, :order.size] = sc[order]
        I[i, :order.size] = rows[order]
    return D, I


def file_bytes(centroids, list_sizes, codes, row_ids, nprobe=1, by_residual=True, is_trained=True) -> bytes:
    """faiss's 'IwSq' record, field by field (index_io.py's head describes it)."""
    cent = np.ascontiguousarray(centroids, "<f4")
    sizes = [int(s) for s in list_sizes]
    nlist, d, ntotal = len(sizes), cent.shape[1], sum(sizes)
    codes, row_ids = np.ascontiguousarray(np.asarray(codes, np.float16), "<f2").reshape(ntotal, d), np.ascontiguousarray(row_ids, "<i8")

    def header(fourcc, n, trained):
        return struct.pack("<4siqqqBi", fourcc, d, n, 1 << 20, 1 << 20, int(trained), 0)
    out = [header(b"IwSq", ntotal, is_trained), struct.pack("<QQ", nlist, nprobe)]
    out += [header(b"IxFI", cent.shape[0], True), struct.pack("<Q", cent.size), cent.tobytes()]
    out += [struct.pack("<B", 0), struct.pack("<Q", 0)]                                  # direct map: NoMap, empty vector
    out += [struct.pack("<iifQQ", 4, 0, 0.0, d, 2 * d), struct.pack("<Q", 0)]            # the ScalarQuantizer (QT_fp16), its empty `trained`
    out += [struct.pack("<Q", 2 * d), struct.pack("<B", int(by_residual))]               # code_size, by_residual
    out += [b"ilar", struct.pack("<QQ", nlist, 2 * d)]
    non0 = [c for c in range(nlist) if sizes[c]]
    if len(non0) > nlist // 2:
        out += [b"full", struct.pack("<Q", nlist)] + [struct.pack("<Q", s) for s in sizes]
    else:
        out += [b"sprs", struct.pack("<Q", 2 * len(non0))] + [struct.pack("<QQ", c, sizes[c]) for c in non0]
    a = 0
    for c in non0:
        out += [codes[a:a + sizes[c]].tobytes(), row_ids[a:a + sizes[c]].tobytes()]
        a += sizes[c]
    return b"".join(out)
