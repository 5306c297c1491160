"""CPU: the range search over the probed cells of the four inverted-file indexes (lrx_ivf_*_ip_range_search, torch.ops.lrx.ivf_*_ip_range_search,
range_search_probed / range_search_preassigned) as far as no GPU is needed -- the exported symbols and the op schemas, every
argument refusal of the four C entry points through fake pointers, the workspace against the sibling search's, the numpy yardstick
(tests/ivf_range_yardstick.py) against a brute-force loop, and the four plain range_search methods, which still refuse."""
import ctypes

import numpy as np
import pytest

from lightretriever_amd import _lib

import ivf_range_yardstick as R
import ivf_yardstick as IV
import ivfpq_yardstick as YPQ
import ivfsq8_yardstick as YS8
import ivfsq_yardstick as YSQ

FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work
NAN = float("nan")
FAMILIES = ("flat", "sq_fp16", "sq8", "pq")


# ---- symbols and schemas ---------------------------------------------------------------------------------------------------------------
def test_the_eight_symbols_are_exported_and_bound():
    l = _lib.lib()
    for fam in FAMILIES:
        for name in (f"lrx_ivf_{fam}_ip_range_search", f"lrx_ivf_{fam}_ip_range_workspace_bytes"):
            assert callable(getattr(l, name)) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[f"lrx_ivf_{fam}_ip_range_search"]
        top = _lib.SIGNATURES[f"lrx_ivf_{fam}_ip_search"][1]
        assert res is ctypes.c_int32 and len(args) == len(top) + 2        # k -> radius; (scores, ids) -> (lims, scores, ids, capacity)
        assert args.count(ctypes.c_float) == 1
        assert len(_lib.SIGNATURES[f"lrx_ivf_{fam}_ip_range_workspace_bytes"][1]) == len(_lib.SIGNATURES[f"lrx_ivf_{fam}_ip_workspace_bytes"][1]) - 1
    assert l.lrx_abi_version() == 9


def test_the_four_ops_are_registered_with_radius_in_the_place_of_k():
    import torch
    from lightretriever_amd import ops, torch_ops
    for fam in FAMILIES:
        name = f"ivf_{fam}_ip_range_search"
        assert name in torch_ops.OPS and callable(getattr(ops, name))
        schema = str(getattr(torch.ops.lrx, name).default._schema)
        top = str(getattr(torch.ops.lrx, f"ivf_{fam}_ip_topk").default._schema)
        assert schema.startswith(f"lrx::{name}(Tensor q, ")
        assert schema.endswith("-> (Tensor, Tensor, Tensor)")
        want = top.replace(f"ivf_{fam}_ip_topk", name).replace("int k,", "float radius,").replace("-> (Tensor, Tensor)", "-> (Tensor, Tensor, Tensor)")
        assert schema == want, (schema, want)


# ---- the C entry points, without a GPU -----------------------------------------------------------------------------------------------------
def _call(l, fam, rows=FAKE, n_rows=1000, dim=64, nlist=16, n_queries=4, nprobe=4, ld_probe=None, by_residual=1, max_scan=500, radius=0.5, lims=FAKE,
          capacity=100, ws_bytes=1 << 30, probe_scores=FAKE, out=FAKE, M=8, qtype=0, trained=FAKE, ldx=None):
    ld = nprobe if ld_probe is None else ld_probe
    tail = (max_scan, radius, 0, lims, out, out, capacity, None, FAKE, ws_bytes, None)
    if fam == "flat":
        return l.lrx_ivf_flat_ip_range_search(rows, n_rows, dim if ldx is None else ldx, dim, FAKE, FAKE, nlist, FAKE, n_queries, FAKE, nprobe, ld, *tail)
    mid = (FAKE, FAKE, nlist, FAKE, n_queries, FAKE, probe_scores, nprobe, ld, by_residual)
    if fam == "sq_fp16":
        return l.lrx_ivf_sq_fp16_ip_range_search(rows, n_rows, dim, *mid, *tail)
    if fam == "sq8":
        return l.lrx_ivf_sq8_ip_range_search(rows, n_rows, dim, trained, qtype, *mid, *tail)
    return l.lrx_ivf_pq_ip_range_search(rows, n_rows, FAKE, dim, M, *mid, *tail)


COMMON = [(dict(radius=NAN), b"radius is NaN"), (dict(capacity=-1), b"capacity=-1"), (dict(lims=None), b"null lims"), (dict(nprobe=0), b"nprobe=0"),
          (dict(nprobe=17), b"nprobe=17"), (dict(nlist=4096, nprobe=2049), b"nprobe=2049"), (dict(nprobe=4, ld_probe=3), b"ld_probe=3"),
          (dict(nlist=0), b"nlist=0"), (dict(max_scan=-1), b"max_scan_rows=-1"), (dict(max_scan=1 << 31), b"max_scan_rows=2147483648"),
          (dict(n_rows=1 << 32), b"rows=4294967296"), (dict(n_queries=-1), b"n_queries=-1"), (dict(out=None), b"null pointer")]
CELL_MAJOR_DIM = [(dict(dim=48), b"dim=48"), (dict(dim=0), b"dim=0"), (dict(dim=8224), b"dim=8224")]
CODED = [(dict(probe_scores=None), b"by_residual=1 needs probe_scores")]
OWN = {"flat": CELL_MAJOR_DIM + [(dict(ldx=60), b"ldx=60"), (dict(rows=ctypes.c_void_p(264)), b"16-byte aligned")],
       "sq_fp16": CELL_MAJOR_DIM + CODED + [(dict(rows=ctypes.c_void_p(264)), b"codes must be 16-byte aligned")],
       "sq8": CELL_MAJOR_DIM + CODED + [(dict(rows=ctypes.c_void_p(264)), b"codes must be 16-byte aligned"), (dict(qtype=1), b"qtype=1"),
                                        (dict(trained=None), b"trained")],
       "pq": CODED + [(dict(dim=60), b"dim=60 is not a multiple of M=8"), (dict(M=0), b"M=0")]}


@pytest.mark.parametrize("fam, kw, msg", [(f, kw, msg) for f in FAMILIES for kw, msg in COMMON + OWN[f]])
def test_argument_errors_are_reported_without_a_gpu(fam, kw, msg):
    l = _lib.lib()
    assert _call(l, fam, **kw) == -1, kw             # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert f"ivf_{fam}_ip_range_search".encode() in l.lrx_last_error()


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_nan_radius_is_refused_before_a_short_workspace_and_no_k_is_asked_for(fam):
    l = _lib.lib()
    assert _call(l, fam, radius=NAN, ws_bytes=0) == -1 and b"radius is NaN" in l.lrx_last_error()
    assert _call(l, fam, ws_bytes=16) == -3 and b"workspace" in l.lrx_last_error()         # LRX_ERR_WORKSPACE: every argument check passed
    assert b"k=" not in l.lrx_last_error()
    assert _call(l, fam, radius=float("inf"), ws_bytes=16) == -3 and _call(l, fam, radius=float("-inf"), ws_bytes=16) == -3
    assert _call(l, fam, capacity=0, out=None, ws_bytes=16) == -3                          # capacity 0 needs no output arrays


def _ws(l, fam, n_rows, nlist, dim, Q, nprobe, max_scan, k=None, M=8):
    """The range workspace (k None) or the sibling search's."""
    args = (n_rows, nlist, dim) + ((M,) if fam == "pq" else ()) + (Q, nprobe) + (() if k is None else (k,)) + (max_scan,)
    return getattr(l, f"lrx_ivf_{fam}_ip_range_workspace_bytes" if k is None else f"lrx_ivf_{fam}_ip_workspace_bytes")(*args)


@pytest.mark.parametrize("fam", FAMILIES)
def test_the_workspace_is_the_siblings_plus_the_hit_counts_of_a_chunk(fam):
    l = _lib.lib()
    for n_rows, nlist, dim, Q, nprobe, max_scan in ((1000, 16, 64, 4, 4, 500), (1 << 20, 1024, 2048, 1000, 128, 200000), (0, 1, 32, 1, 1, 0),
                                                    (5000, 64, 256, 5000, 64, 5000), (1 << 20, 1024, 64, 100, 128, 1 << 20)):
        r = _ws(l, fam, n_rows, nlist, dim, Q, nprobe, max_scan)
        for k in (1, 100, 2048):
            s = _ws(l, fam, n_rows, nlist, dim, Q, nprobe, max_scan, k=k)
            chunk = min(Q, 1024, max((768 << 20) // (8 * max(max_scan, 1)), 1))
            assert s + 4 * chunk <= r <= s + 4 * chunk + 256, (fam, r, s, chunk)
        need = r
        assert _call(l, fam, n_rows=n_rows, nlist=nlist, dim=dim, n_queries=Q, nprobe=nprobe, max_scan=max_scan, ws_bytes=need - 1) == -3
    # monotone in n_queries up to a chunk (and never decreasing after)
    sizes = [_ws(l, fam, 100000, 64, 128, Q, 8, 20000) for Q in (1, 2, 3, 64, 65, 1000, 1024, 1025, 5000)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[3] < sizes[6] == sizes[7] == sizes[8]


# ---- the yardstick against a brute-force loop ---------------------------------------------------------------------------------------------------
SIZES = [0, 1, 7, 9, 40, 3, 25]


def _cells(seed=0, d=32):
    rng = np.random.default_rng(seed)
    nlist, n = len(SIZES), sum(SIZES)
    cells = rng.permutation(np.repeat(np.arange(nlist), SIZES))
    x = rng.integers(-3, 4, (n, d)).astype(np.float32)
    q = rng.integers(-3, 4, (5, d)).astype(np.float32)
    row_ids, list_off = IV.cell_order(cells, nlist)
    return rng, x, q, cells, row_ids, list_off


def _brute(score, probes, list_off, row_ids, radius, id_base=0, row_map=None, max_scan_rows=None):
    """The contract, entry by entry: score(i, position, j) -> the fp32 score of stored position `position` for query i probed through entry j."""
    nlist = len(list_off) - 1
    lims, D, I = [0], [], []
    for i, row in enumerate(probes):
        seen, seg = [], []
        for j, c in enumerate(row):
            if c < 0 or c >= nlist or c in seen:
                continue
            seen.append(c)
            seg += [(p, j) for p in range(list_off[c], list_off[c + 1])]
        if max_scan_rows is not None and len(seg) > max_scan_rows:
            seg = []
        for p, j in seg:
            s = np.float32(score(i, p, j))
            if s > np.float32(radius):
                D.append(s)
                I.append(row_map[row_ids[p]] if row_map is not None else id_base + row_ids[p])
        lims.append(len(D))
    return np.array(lims, np.int64), np.array(D, np.float32), np.array(I, np.int64)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and np.array_equal(a[2], b[2])


PROBES = np.array([[4, 2, 6], [3, 3, 0], [-1, 5, 7], [2 ** 40, 1, 4], [6, 4, 6]], np.int64)


def test_the_flat_yardstick_equals_the_brute_force_loop():
    rng, x, q, cells, row_ids, list_off = _cells()
    stored = x[row_ids]
    score = lambda i, p, j: IV.exact_scores(q[i], stored[p:p + 1])[0]
    all_scores = np.concatenate([IV.exact_scores(q[i], stored) for i in range(len(q))])
    rm = np.arange(len(x)) * 5 + 2
    for radius in (float(np.median(all_scores)), float(all_scores.max()), -np.inf, np.inf, 0.0, -0.0):
        for kw in (dict(), dict(id_base=1000), dict(row_map=rm), dict(max_scan_rows=60)):
            got = R.expected(IV.search, (q, stored), PROBES, list_off, row_ids, radius, **kw)
            assert _same(got, _brute(score, PROBES, list_off, row_ids, radius, **kw)), (radius, kw)
    lims, D, I = R.expected(IV.search, (q, stored), PROBES, list_off, row_ids, float(np.median(all_scores)))
    scanned = R.scanned_rows(PROBES, list_off)
    assert scanned.tolist() == [72, 9, 3, 41, 65] and R.some_query_is_partial(lims, scanned)
    assert (D > np.float32(np.median(all_scores))).all()
    # segment order: query 0 probes cells 4, 2, 6 -- its ids come cell by cell, ascending original row inside a cell, not ascending overall
    ids0 = I[lims[0]:lims[1]]
    c0 = cells[ids0]
    assert [c for n, c in enumerate(c0) if n == 0 or c != c0[n - 1]] == [4, 2, 6]
    assert all((np.diff(ids0[c0 == c]) > 0).all() for c in (4, 2, 6)) and not (np.diff(ids0) > 0).all()
    # strictness at an attained score; +inf: nothing; -inf: every scanned row; a query over max_scan_rows: nothing
    top = float(all_scores.max())
    assert len(R.expected(IV.search, (q, stored), PROBES, list_off, row_ids, top)[1]) == 0
    assert R.expected(IV.search, (q, stored), PROBES, list_off, row_ids, np.inf)[0][-1] == 0
    assert np.array_equal(np.diff(R.expected(IV.search, (q, stored), PROBES, list_off, row_ids, -np.inf)[0]), scanned)
    assert np.diff(R.expected(IV.search, (q, stored), PROBES, list_off, row_ids, -np.inf, max_scan_rows=64)[0]).tolist() == [0, 9, 3, 41, 0]
    assert np.array_equal(R.scanned_rows(PROBES, list_off, 64), [0, 9, 3, 41, 0])
    # signed zero: an all-zero query scores 0.0 everywhere; 0.0 and -0.0 are one radius
    z = np.zeros_like(q)
    for radius, hits in ((0.0, 0), (-0.0, 0), (-1.0, int(scanned.sum()))):
        assert R.expected(IV.search, (z, stored), PROBES, list_off, row_ids, radius)[0][-1] == hits


def test_the_coded_yardsticks_equal_the_brute_force_loop_and_a_repeat_keeps_its_first_base():
    rng, x, q, cells, row_ids, list_off = _cells(seed=1)
    n, d, nlist = len(x), x.shape[1], len(SIZES)
    base = (rng.integers(-12, 13, PROBES.shape) / 4.0).astype(np.float32)
    base[4, 2] = 1e30                                                     # the repeat of cell 6 in query 4: never used
    # fp16 codes
    codes = YSQ.encode(x[row_ids])
    sq = lambda i, p, j: YSQ.row_scores(q[i], codes[p:p + 1], float(base[i, j]))[0]
    # 8-bit codes on the exact grid
    trained = np.array(YS8.GRID_RANGES[1][:2] * 1, np.float32).repeat(d)
    c8 = rng.integers(0, 256, (n, d)).astype(np.uint8)
    y8 = YS8.decode(c8, trained)
    s8 = lambda i, p, j: YS8.row_scores(q[i], y8[p:p + 1], float(base[i, j]))[0]
    # PQ codes
    M = 4
    C = rng.integers(-2, 3, (M, 256, d // M)).astype(np.float32)
    cpq = rng.integers(0, 256, (n, M)).astype(np.uint8)
    import pq_yardstick as PQ
    L = PQ.lut(q, C)
    spq = lambda i, p, j: YPQ.row_scores(L[i], cpq[p:p + 1], np.float32(base[i, j]))[0]
    for search_fn, head, score in ((YSQ.search, (q, codes), sq), (YS8.search, (q, c8, trained), s8), (YPQ.search, (q, C, cpq), spq)):
        every = R.expected(search_fn, head, PROBES, list_off, row_ids, -np.inf, probe_scores=base, by_residual=True)
        assert np.array_equal(np.diff(every[0]), R.scanned_rows(PROBES, list_off)) and (every[1] < 1e20).all()
        radius = float(np.median(every[1]))
        for kw in (dict(), dict(id_base=7, max_scan_rows=60)):
            got = R.expected(search_fn, head, PROBES, list_off, row_ids, radius, probe_scores=base, by_residual=True, **kw)
            assert _same(got, _brute(score, PROBES, list_off, row_ids, radius, **kw)), (search_fn.__module__, kw)
        assert R.some_query_is_partial(got[0], R.scanned_rows(PROBES, list_off, 60))


# ---- the pinned refusals stay -----------------------------------------------------------------------------------------------------------------
def test_the_plain_range_search_still_refuses_and_the_new_names_exist():
    from lightretriever_amd import IVFFlatIndex, IVFPQIndex, IVFSQ8Index, IVFSQIndex
    from lightretriever_amd.retriever import FaissIndex
    for cls in (IVFFlatIndex, IVFPQIndex, IVFSQIndex, IVFSQ8Index):
        with pytest.raises(NotImplementedError, match="range_search"):
            cls.range_search(cls.__new__(cls), None, 0.0)
        assert callable(cls.range_search_probed) and callable(cls.range_search_preassigned)
        assert "range_search_preassigned" in cls.__doc__ and "stays refused" in cls.__doc__
    assert callable(FaissIndex.range_search_probed)
