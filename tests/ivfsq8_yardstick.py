"""Numpy yardstick of the inverted-file 8-bit scalar-quantised index (lightretriever_amd/ivfsq8.py, lrx_ivf_sq8_ip_search),
built on ivf_yardstick (cells, k-means, probe lists) and sq8_yardstick (the quantiser: range, codes, decode):

    code    sq8_yardstick.encode(v, trained); v = x, or with centroids fl32(x - centroid[cell]); a cell outside [0, nlist): zeros
    decode  y = sq8_yardstick.decode(code, trained), plus centroid[cell] (one fp32 add) with centroids; a cell outside [0, nlist): zeros
    score(query i, position p in the probed cell probes[i][j])
            (float)(B + sum_e (double)q_e * (double)y_e) over the row DECODED WITHOUT its centroid,  B = by_residual ? (double)probe_scores[i][j] : 0
            the sum in exact_dot's order: lane `sub` of a half-wave takes elements 4 sub + 128 u + 0..3 of each 2048-element block, fp64
            accumulation, then the xor tree 16, 8, 4, 2, 1
    top-k   score descending, ties to the lower ORIGINAL row, (-FLT_MAX, -1) padding
    range   faiss's train_encoder: every training row to its coarse top-1 cell, the residual (the row itself without by_residual), then
            sq8_yardstick.train over the residuals

a brute-force search with that sum, an exact rerank of given candidates and the 'IwSq' file with an 8-bit quantiser written field by field --
for clarity, not speed.  The GPU tests compare the library with it; the CPU tests check it on its own."""
import struct

import numpy as np

import ivf_yardstick as IV
import sq8_yardstick as S8
from ivfsq_yardstick import rerank  # noqa: F401  (re-exported: the exact rerank of given candidates over fp32 rows is the same)

FLT_MAX = np.finfo(np.float32).max
F32 = np.float32
QT_8BIT, QT_8BIT_UNIFORM = 0, 2
# (vmin, vdiff) whose 256 decoded values are exactly -32 + c / 4, -64 + c / 2 and -128 + c (test_ivfsq8_index_host.py checks it)
GRID_RANGES = ((-32.125, 63.75, 0.25), (-64.25, 127.5, 0.5), (-128.5, 255.0, 1.0))


def _ok(n, cent, cells, nlist):
    """Which of n rows name a cell of their own: all of them without cells; nlist defaults to the number of centroids."""
    if cells is None:
        return np.ones(n, bool)
    nlist = len(cent) if nlist is None else nlist
    cells = np.asarray(cells, np.int64)
    return (cells >= 0) & (cells < nlist)


def encode(x, trained, cent=None, cells=None, nlist=None) -> np.ndarray:
    """uint8 [n, d]: the codes of the rows x -- of their residuals to cent[cells] (one fp32 subtraction) when cent is given; zeros where cells
    (when given) names no cell of [0, nlist)."""
    v = np.asarray(x, F32)
    ok = _ok(len(v), cent, cells, nlist)
    if cent is not None:
        c = np.where(ok, np.asarray(cells, np.int64), 0)
        v = (v - np.asarray(cent, F32)[c]).astype(F32)
    codes = S8.encode(v, trained)
    codes[~ok] = 0
    return codes


def decode(codes, trained, cent=None, cells=None, nlist=None) -> np.ndarray:
    """fp32 [n, d]: the decoded codes, plus cent[cells] (one fp32 add) when cent is given; zeros where cells (when given) names no cell of
    [0, nlist)."""
    y = S8.decode(np.asarray(codes, np.uint8), trained)
    ok = _ok(len(y), cent, cells, nlist)
    if cent is not None:
        c = np.where(ok, np.asarray(cells, np.int64), 0)
        y = (y + np.asarray(cent, F32)[c]).astype(F32)
    y[~ok] = 0
    return y


def ordered_sums(q, y) -> np.ndarray:
    """fp64 [n]: sum_e q_e * y_e per fp32 row of y, added in exact_dot's order (the head of this file).  The products of two fp32 numbers are
    exact in fp64, so only the order of the additions matters."""
    q, y = np.asarray(q, F32).astype(np.float64), np.asarray(y, F32).astype(np.float64)
    n, d = y.shape
    nb = -(-d // 2048)
    p = np.zeros((n, nb * 2048), np.float64)                                  # (an element past d adds +0.0: the sum is never -0.0)
    p[:, :d] = y * q[None, :]
    p = p.reshape(n, nb, 16, 32, 4)                                           # element = 2048 block + 128 u + 4 sub + e
    term = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]                  # [n, block, u, sub]
    acc = np.zeros((n, 32), np.float64)
    for b in range(nb):
        for u in range(16):
            if b * 2048 + u * 128 < d:                                        # (a lane past d skips the step; the others add their term)
                live = (b * 2048 + u * 128 + 4 * np.arange(32)) < d
                acc = np.where(live[None, :], acc + term[:, b, u, :], acc)
    for o in (16, 8, 4, 2, 1):
        acc = acc + acc[:, np.arange(32) ^ o]
    return acc[:, 0]


def row_scores(q, y, base=0.0) -> np.ndarray:
    """fp32 [n]: (float)(base + the ordered sum): one rounding.  base: one value, or one per row."""
    if len(y) == 0:
        return np.zeros(0, F32)
    return (np.asarray(base, np.float64) + ordered_sums(q, y)).astype(F32)


def search(q, codes, trained, list_off, row_ids, probes, probe_scores, by_residual, k, id_base=0, row_map=None, max_scan_rows=None):
    """(D f32[Q,k], I i64[Q,k]): per query the positions of the cells probes[i] names (codes uint8 [n, d] stored cell by cell, cell c =
    positions [list_off[c], list_off[c + 1]), row_ids: position -> original row, None = the position; an entry < 0 or >= nlist is skipped, a cell
    named twice counts once, with the base term of its FIRST occurrence), scored as the head of this file says, the best k by score descending,
    ties to the lower ORIGINAL row, (-FLT_MAX, -1) padding.  A query whose cells hold more than max_scan_rows (when given) is all padding."""
    q, codes = np.asarray(q, F32), np.asarray(codes, np.uint8)
    list_off, probes = np.asarray(list_off, np.int64), np.asarray(probes, np.int64)
    nlist = len(list_off) - 1
    row_ids = np.arange(len(codes), dtype=np.int64) if row_ids is None else np.asarray(row_ids, np.int64)
    y = S8.decode(codes, trained) if len(codes) else np.zeros(codes.shape, F32)
    Q = q.shape[0]
    D = np.full((Q, k), -FLT_MAX, F32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        seen, pos, base = set(), [np.zeros(0, np.int64)], [np.zeros(0, F32)]
        for j, c in enumerate(probes[i].tolist()):
            if 0 <= c < nlist and c not in seen:
                seen.add(c)
                pos.append(np.arange(list_off[c], list_off[c + 1]))
                base.append(np.full(pos[-1].size, probe_scores[i][j] if by_residual else 0.0, F32))
        pos, base = np.concatenate(pos), np.concatenate(base)
        sc, rows = row_scores(q[i], y[pos], base), row_ids[pos]                # one call for the query: a row's score depends on its own base alone
        if max_scan_rows is not None and rows.size > max_scan_rows:
            continue
        order = np.lexsort((rows, -sc.astype(np.float64)))[:k]
        D[i, :order.size] = sc[order]
        I[i, :order.size] = (id_base + rows[order]) if row_map is None else np.asarray(row_map, np.int64)[rows[order]]
    return D, I


def train_range(x, cent, by_residual: bool, uniform: bool) -> np.ndarray:
    """trained = vmin ++ vdiff of the training rows' residuals to their coarse top-1 centroids (of the rows themselves without by_residual)."""
    x = np.asarray(x, F32)
    if by_residual:
        x = (x - np.asarray(cent, F32)[IV.assign_cells(x, cent)]).astype(F32)
    return S8.train(x, uniform)


def file_bytes(centroids, trained, qtype, list_sizes, codes, row_ids, nprobe=1, by_residual=True, is_trained=True) -> bytes:
    """faiss's 'IwSq' record with an 8-bit ScalarQuantizer, field by field (index_io.py's head describes it)."""
    cent = np.ascontiguousarray(centroids, "<f4")
    sizes = [int(s) for s in list_sizes]
    nlist, d, ntotal = len(sizes), cent.shape[1], sum(sizes)
    codes, row_ids = np.ascontiguousarray(np.asarray(codes, np.uint8)).reshape(ntotal, d), np.ascontiguousarray(row_ids, "<i8")
    t = np.ascontiguousarray(trained, "<f4").reshape(-1)

    def header(fourcc, n, trained_flag):
        return struct.pack("<4siqqqBi", fourcc, d, n, 1 << 20, 1 << 20, int(trained_flag), 0)
    out = [header(b"IwSq", ntotal, is_trained), struct.pack("<QQ", nlist, nprobe)]
    out += [header(b"IxFI", cent.shape[0], True), struct.pack("<Q", cent.size), cent.tobytes()]
    out += [struct.pack("<B", 0), struct.pack("<Q", 0)]                                  # direct map: NoMap, empty vector
    out += [struct.pack("<iifQQ", qtype, 0, 0.0, d, d), struct.pack("<Q", t.size), t.tobytes()]   # the ScalarQuantizer, its `trained`
    out += [struct.pack("<Q", d), struct.pack("<B", int(by_residual))]                   # code_size, by_residual
    out += [b"ilar", struct.pack("<QQ", nlist, d)]
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
