"""Numpy yardstick of the range search over the probed cells (lrx_ivf_*_ip_range_search, range_search_probed / range_search_preassigned of the
four inverted-file indexes), restating the contract of include/lrx.h on top of the four families' own yardsticks:

    hit     a row the family's top-k search of the same arguments scans -- the row lies in a cell the query's probe row names; an entry < 0 or
            >= nlist is skipped; a cell named twice is scanned once; a query whose cells hold more than max_scan_rows scans nothing -- whose
            score, the fp32 value that search reports for the pair, is STRICTLY greater than radius as an fp32 comparison (-0.0 == +0.0, a
            score equal to the radius is no hit, +inf: none, -inf: every scanned row)
    order   SEGMENT order: the query's cells in the order of its probe row (after the skips), inside a cell by stored position
    layout  lims int64 [Q + 1], lims[0] = 0; D fp32 / I int64 [lims[Q]]; I = id_base + row, or row_map[row]

The scores come from the family's `search` with k = n (every scanned row, so nothing is cut); the order is rebuilt here from probes, list_off
and row_ids.  Written for clarity, not speed.  The GPU tests compare the library with it; the CPU tests check it against a brute-force loop."""
import numpy as np


def scanned_positions(probe_row, list_off, max_scan_rows=None) -> np.ndarray:
    """int64: the stored positions one query scans, in segment order (empty when they are more than max_scan_rows)."""
    list_off = np.asarray(list_off, np.int64)
    nlist = len(list_off) - 1
    cells, seen = [], set()
    for c in np.asarray(probe_row, np.int64).tolist():
        if 0 <= c < nlist and c not in seen:
            seen.add(c)
            cells.append(c)
    pos = np.concatenate([np.arange(list_off[c], list_off[c + 1], dtype=np.int64) for c in cells] + [np.zeros(0, np.int64)])
    if max_scan_rows is not None and pos.size > max_scan_rows:
        return np.zeros(0, np.int64)
    return pos


def expected(search_fn, head, probes, list_off, row_ids, radius, id_base=0, row_map=None, max_scan_rows=None, probe_scores=None, by_residual=None):
    """(lims i64[Q + 1], D f32[lims[Q]], I i64[lims[Q]]) of the range search.
    search_fn: the family's yardstick search -- ivf_yardstick.search (by_residual None: it takes no probe scores), ivfsq_yardstick.search,
    ivfsq8_yardstick.search or ivfpq_yardstick.search; head: its arguments in front of list_off, (q, X) / (q, codes) / (q, codes, trained) /
    (q, pq_centroids, codes), the rows by stored position."""
    probes, list_off = np.asarray(probes, np.int64), np.asarray(list_off, np.int64)
    n = int(list_off[-1])
    row_ids = np.arange(n, dtype=np.int64) if row_ids is None else np.asarray(row_ids, np.int64)
    radius = np.float32(radius)
    Q = probes.shape[0]
    k = max(n, 1)
    if by_residual is None:
        Dk, Ik = search_fn(*head, list_off, row_ids, probes, k, max_scan_rows=max_scan_rows)
    else:
        Dk, Ik = search_fn(*head, list_off, row_ids, probes, probe_scores, by_residual, k, max_scan_rows=max_scan_rows)
    Dk, Ik = np.asarray(Dk, np.float32), np.asarray(Ik, np.int64)
    lims = np.zeros(Q + 1, np.int64)
    D, I = [], []
    for i in range(Q):
        valid = Ik[i] >= 0
        score_of = dict(zip(Ik[i][valid].tolist(), Dk[i][valid]))         # original row -> the score search reports
        rows = row_ids[scanned_positions(probes[i], list_off, max_scan_rows)]
        assert rows.size == len(score_of), "the family's search and the segment disagree on the scanned rows"
        sc = np.array([score_of[r] for r in rows.tolist()], np.float32)
        keep = sc > radius                                                  # fp32 > fp32
        D.append(sc[keep])
        I.append((id_base + rows[keep]) if row_map is None else np.asarray(row_map, np.int64)[rows[keep]])
        lims[i + 1] = lims[i] + int(keep.sum())
    return lims, np.concatenate(D + [np.zeros(0, np.float32)]).astype(np.float32), np.concatenate(I + [np.zeros(0, np.int64)]).astype(np.int64)


def scanned_rows(probes, list_off, max_scan_rows=None) -> np.ndarray:
    """int64 [Q]: how many rows each query scans."""
    return np.array([scanned_positions(p, list_off, max_scan_rows).size for p in np.asarray(probes, np.int64)], np.int64)


def some_query_is_partial(lims, scanned) -> bool:
    """At least one query has a hit count strictly between 0 and the rows it scans: the result is neither empty nor everything."""
    hits = np.diff(np.asarray(lims, np.int64))
    return bool(((hits > 0) & (hits < np.asarray(scanned, np.int64))).any())
