"""Numpy yardstick of the inverted-file product-quantised index (lightretriever_amd/ivfpq.py, lrx_ivf_pq_ip_search), built on
ivf_yardstick (cells, k-means, probe lists) and pq_yardstick (codes, lookup tables, PQ k-means):

    score(query i, position p in the probed cell probes[i][j])
        acc = by_residual ? probe_scores[i][j] : 0.f;   acc = acc + LUT[i][m][code_m(p)]   for m = 0 .. M - 1, one fp32 add each
    top-k   score descending, ties to the lower ORIGINAL row, (-FLT_MAX, -1) padding

a brute-force search with those sequential adds, the index's training and the 'IwPQ' file written field by field -- for clarity, not speed.
The GPU tests compare the library with it; the CPU tests check it on its own."""
import struct

import numpy as np

import ivf_yardstick as IV
import pq_yardstick as PQ

FLT_MAX = np.finfo(np.float32).max


def row_scores(L, codes, base):
    """L fp32 [M, 256] (one query's table), codes uint8 [n, M], base fp32 (one value, or one per row) -> fp32 [n]: base, then the M table
    entries in ascending m."""
    acc = np.broadcast_to(np.asarray(base, np.float32), codes.shape[:1]).copy()
    for m in range(L.shape[0]):
        acc = (acc + L[m, codes[:, m]]).astype(np.float32)
    return acc


def search(q, pq_centroids, codes, list_off, row_ids, probes, probe_scores, by_residual, k, id_base=0, row_map=None, max_scan_rows=None):
    """(D f32[Q,k], I i64[Q,k]): per query the positions of the cells probes[i] names (codes uint8 [n, M] stored cell by cell, cell c =
    positions [list_off[c], list_off[c + 1]), row_ids: position -> original row, None = the position; an entry < 0 or >= nlist is skipped, a
    cell named twice counts once, with the base term of its FIRST occurrence), scored as the head of this file says, the best k by score
    descending, ties to the lower ORIGINAL row, (-FLT_MAX, -1) padding.  A query whose cells hold more than max_scan_rows (when given) is all
    padding.  Ids: id_base + row, or row_map[row]."""
    q, C, codes = np.asarray(q, np.float32), np.asarray(pq_centroids, np.float32), np.asarray(codes, np.uint8)
    list_off, probes = np.asarray(list_off, np.int64), np.asarray(probes, np.int64)
    nlist = len(list_off) - 1
    row_ids = np.arange(len(codes), dtype=np.int64) if row_ids is None else np.asarray(row_ids, np.int64)
    L = PQ.lut(q, C)
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
        sc, rows = row_scores(L[i], codes[pos], base), row_ids[pos]            # one call for the query: a row's score depends on its own base alone
        if max_scan_rows is not None and rows.size > max_scan_rows:
            continue
        order = np.lexsort((rows, -sc.astype(np.float64)))[:k]
        D[i, :order.size] = sc[order]
        I[i, :order.size] = (id_base + rows[order]) if row_map is None else np.asarray(row_map, np.int64)[rows[order]]
    return D, I


def decode(codes, pq_centroids):
    """codes uint8 [n, M], pq_centroids [M, 256, dsub] -> fp32 [n, M * dsub]: the centroid of every code."""
    C = np.asarray(pq_centroids, np.float32)
    M = C.shape[0]
    return C[np.arange(M)[None, :], np.asarray(codes).astype(np.int64)].reshape(len(codes), -1)


def residuals(x, cent, cells):
    """x - centroid[cell]: one fp32 subtraction per element."""
    return (np.asarray(x, np.float32) - np.asarray(cent, np.float32)[cells]).astype(np.float32)


def train(x, nlist, M, by_residual=True, niter=None, seed=None):
    """(centroids fp32 [nlist, d], pq_centroids fp32 [M, 256, d / M]): the index's training -- the coarse k-means of ivf_yardstick, then
    pq_yardstick's k-means over the residuals of ALL rows to the centroid of their cell (the best centroid by inner product), or over the rows
    themselves.  niter: of both k-means (default: 10 and 25)."""
    x = np.asarray(x, np.float32)
    if x.shape[0] < max(nlist, PQ.KSUB):
        raise ValueError(f"{x.shape[0]} training rows < max(nlist={nlist}, {PQ.KSUB})")
    seed = IV.SEED if seed is None else seed
    cent = IV.kmeans(x, nlist, IV.NITER if niter is None else niter, seed)
    r = residuals(x, cent, IV.assign_cells(x, cent)) if by_residual else x
    return cent, PQ.kmeans(r, M, 25 if niter is None else niter, seed)


def file_bytes(centroids, pq_centroids, list_sizes, codes, row_ids, nprobe=1, by_residual=True, is_trained=True) -> bytes:
    """faiss's 'IwPQ' record, field by field (index_io.py's head describes it)."""
    cent = np.ascontiguousarray(centroids, "<f4")
    pqc = np.ascontiguousarray(pq_centroids, "<f4")
    sizes = [int(s) for s in list_sizes]
    nlist, d, ntotal, M = len(sizes), cent.shape[1], sum(sizes), pqc.shape[0]
    codes, row_ids = np.ascontiguousarray(codes, np.uint8).reshape(ntotal, M), np.ascontiguousarray(row_ids, "<i8")

    def header(fourcc, n, trained):
        return struct.pack("<4siqqqBi", fourcc, d, n, 1 << 20, 1 << 20, int(trained), 0)
    out = [header(b"IwPQ", ntotal, is_trained), struct.pack("<QQ", nlist, nprobe)]
    out += [header(b"IxFI", cent.shape[0], True), struct.pack("<Q", cent.size), cent.tobytes()]
    out += [struct.pack("<B", 0), struct.pack("<Q", 0)]                                  # direct map: NoMap, empty vector
    out += [struct.pack("<B", int(by_residual)), struct.pack("<Q", M)]                   # by_residual, code_size
    out += [struct.pack("<QQQ", d, M, 8), struct.pack("<Q", pqc.size), pqc.tobytes()]    # the ProductQuantizer
    out += [b"ilar", struct.pack("<QQ", nlist, M)]
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
