"""The plans of tests/test_gpu_ivf_plan_scale.py, in plain numpy: cell sizes that put cells on the run and wave boundaries of k_ivf_items, probe
matrices that cross the thread runs and waves of k_ivf_plan (random prefixes, crafted skip patterns), and one call of a family's yardstick
search shared by every comparison of a case.  A helper module: it holds no tests (tests/test_ivf_plan_scale_host.py checks it)."""
import numpy as np

import ivf_range_yardstick as R

NLIST = 2500                                 # k_ivf_items: 1024 threads over nlist + 1 entries -> runs of 3 cells
NPROBE_MAX = 2048                            # k_ivf_plan: 256 threads -> runs of 8 entries, a wave owns 512
# larger cells on the thread-run (2 | 3), wave (191 | 192) and 1024-cell boundaries of k_ivf_items and at its last cell; sizes around the group
# sizes of the scans (128 rows, the fp16 / 8-bit scans' too at d = 64) and the 1024-word tiles of the PQ scan and the range fill
BIG_CELLS = {2: 127, 3: 128, 191: 129, 192: 257, 1023: 1025, 1024: 128, 2499: 129}
N_EMPTY = 200


def scale_sizes(nlist=NLIST, big=None, n_empty=N_EMPTY, seed=0):
    """Rows per cell: 1 to 3, `n_empty` random cells and cell 0 empty, then the cells of `big` (default BIG_CELLS) at their sizes."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 4, nlist)
    sizes[rng.permutation(nlist)[:n_empty]] = 0
    sizes[0] = 0
    for c, s in (BIG_CELLS if big is None else big).items():
        sizes[c] = s
    return [int(s) for s in sizes]


def edge_sizes(nlist, seed=0):
    """Rows per cell of the small stores around k_ivf_items' 1024 threads: 0 to 2, cell 0 empty, 129 rows in the last cell."""
    rng = np.random.default_rng(seed + nlist)
    sizes = rng.integers(0, 3, nlist)
    sizes[0] = 0
    sizes[nlist - 1] = 129
    return [int(s) for s in sizes]


def prefix_probes(rng, Q, nprobe, among):
    """int64 [Q, nprobe]: each row the first nprobe cells of its own random permutation of `among` (no repeats inside a row)."""
    among = np.asarray(among, np.int64)
    assert nprobe <= among.size
    return np.stack([rng.permutation(among)[:nprobe] for _ in range(Q)]).astype(np.int64)


def with_cell(probes, cell, rows, rng):
    """A copy of probes in which each row of `rows` names `cell` (written over a random entry where the row does not name it yet)."""
    out = np.array(probes, np.int64)
    for i in rows:
        if not (out[i] == cell).any():
            out[i, int(rng.integers(0, out.shape[1]))] = cell
    return out


def largest_first(probes, list_off):
    """The rows of probes reordered so that row 0 scans strictly more rows than any other (asserted) -> (probes, the scanned rows per query)."""
    scanned = R.scanned_rows(probes, list_off)
    order = np.argsort(-scanned, kind="stable")
    probes, scanned = np.asarray(probes, np.int64)[order], scanned[order]
    assert scanned[0] > scanned[1] > 0
    return probes, scanned


def crafted_probes(sizes, seed=0):
    """int64 [7, 2048] over cells of the given sizes (nlist >= 2048 + a few): the skip patterns a .. g of test_crafted_skip_patterns, one per
    row.  A thread of k_ivf_plan owns 8 consecutive entries and a wave 512, so runs [8 t, 8 t + 8) and [512 w, 512 w + 512) are whole thread
    runs and whole waves.  Entries >= nlist are nlist, 2^40 and 2^62 in turn."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    nlist, P = sizes.size, NPROBE_MAX
    full, empty = np.flatnonzero(sizes > 0), np.flatnonzero(sizes == 0)
    assert empty.size >= 2 and full.size > P
    bad = np.array([nlist, 2 ** 40, 2 ** 62], np.int64)
    bads = lambda n: bad[np.arange(n) % 3]
    nothing = lambda n: np.concatenate([np.full(n, -1), rng.choice(empty, n), bads(n)]).astype(np.int64)[rng.permutation(3 * n)[:n]]
    out = np.empty((7, P), np.int64)
    # a. whole thread runs of -1, of entries >= nlist and of repeats -- inside a wave, and on both sides of the wave boundary at 512
    a = prefix_probes(rng, 1, P, np.arange(nlist))[0]
    a[8:16], a[24:32], a[40:48] = -1, bads(8), a[0:8]
    a[504:512], a[512:520], a[1016:1024], a[1024:1032] = -1, bads(8), a[496:504], bads(8)
    out[0] = a
    # b. a whole wave skipped: -1, entries >= nlist and repeats of the wave before it, a third each
    b = prefix_probes(rng, 1, P, np.arange(nlist))[0]
    b[512:1024] = np.concatenate([np.full(171, -1), bads(171), b[0:170]])[rng.permutation(512)]
    out[1] = b
    # c. one cell of several rows named first at entry 0, then again in its own thread's run, the next thread's, at the end of its wave, at
    # the start of the next and at the last entry of all
    x = int(full[np.argmax(sizes[full] >= 100)])
    c = prefix_probes(rng, 1, P, np.setdiff1d(np.arange(nlist), [x]))[0]
    c[[0, 7, 8, 511, 512, 2047]] = x
    out[2] = c
    # d. an empty cell and an entry >= nlist, each named twice, in different waves
    e0 = int(empty[0])
    d = prefix_probes(rng, 1, P, np.setdiff1d(np.arange(nlist), [e0]))[0]
    d[[5, 700]], d[[9, 1500]] = e0, 2 ** 40
    out[3] = d
    # e / f. one non-empty cell alone, at the last entry / at the first; g. nothing valid
    y = int(full[-1])
    out[4] = nothing(P)
    out[4, P - 1] = y
    out[5] = nothing(P)
    out[5, 0] = y
    out[6] = nothing(P)
    return out


class CachedSearch:
    """ONE call of a family's yardstick search (ivf_yardstick.search for by_residual None, else ivfsq / ivfsq8 / ivfpq_yardstick.search) at k = n
    -- every scanned row of every query, sorted -- from which a case takes all its references: the top k for any k <= n is the head of that
    result (the same order, the same padding), and the range search is ivf_range_yardstick.expected over it."""

    def __init__(self, search_fn, head, list_off, row_ids, probes, probe_scores=None, by_residual=None, max_scan_rows=None):
        self.head, self.list_off, self.row_ids, self.probes = head, np.asarray(list_off, np.int64), row_ids, np.asarray(probes, np.int64)
        self.probe_scores, self.by_residual, self.max_scan_rows = probe_scores, by_residual, max_scan_rows
        self.k = max(int(self.list_off[-1]), 1)
        mid = () if by_residual is None else (probe_scores, by_residual)
        self._ranges = {}
        self.D, self.I = search_fn(*head, self.list_off, row_ids, self.probes, *mid, self.k, max_scan_rows=max_scan_rows)

    def _again(self, *args, max_scan_rows=None):
        assert args[-1] == self.k and max_scan_rows == self.max_scan_rows
        return self.D, self.I

    def topk(self, k):
        assert 1 <= k <= self.k
        return self.D[:, :k], self.I[:, :k]

    def range(self, radius):
        key = float(np.float32(radius))
        if key not in self._ranges:
            self._ranges[key] = self._range(radius)
        return self._ranges[key]

    def _range(self, radius):
        return R.expected(self._again, self.head, self.probes, self.list_off, self.row_ids, radius, max_scan_rows=self.max_scan_rows,
                          probe_scores=self.probe_scores, by_residual=self.by_residual)

    def scanned(self):
        return R.scanned_rows(self.probes, self.list_off, self.max_scan_rows)

    def median(self):
        """The median score over every scanned (query, row) pair."""
        return float(np.median(self.range(-np.inf)[1]))
