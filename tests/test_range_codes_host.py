"""CPU: the range-search entry points of the fp16-SQ, PQ and impact indexes are declared, exported and bound, size their workspaces
sensibly and reject bad arguments with a message before any device work; SQ8Index.range_search names its follow-up; the numpy yardstick
(tests/range_codes_yardstick.py) agrees with a brute-force double loop."""
import ctypes
import math
import os

import numpy as np
import pytest

import impact_yardstick as IY
import range_codes_yardstick as RY
from lightretriever_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lrx_sq_fp16_ip_range_workspace_bytes", "lrx_sq_fp16_ip_range_search", "lrx_pq_ip_range_workspace_bytes", "lrx_pq_ip_range_search",
           "lrx_range_impact_workspace_bytes", "lrx_range_impact_search")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "lrx.h")).read()
    l = ctypes.CDLL(build.build(verbose=False))
    for s in SYMBOLS:
        assert s + "(" in hdr, s
        assert hasattr(l, s), s
        assert s in _lib.SIGNATURES, s
    assert "#define LRX_ABI_VERSION 9" in hdr
    assert os.path.exists(build.build_torch_ops(verbose=False))
    from lightretriever_amd import torch_ops
    for op in ("sq_fp16_ip_range_search", "pq_ip_range_search", "impact_range_search"):
        assert op in torch_ops.OPS


def test_workspaces_are_monotone_in_queries_and_rows():
    l = _lib.lib()
    sq = lambda n, q: int(l.lrx_sq_fp16_ip_range_workspace_bytes(n, 128, q))
    pq = lambda n, q, rc=0: int(l.lrx_pq_ip_range_workspace_bytes(n, 32, 8, q, rc))
    im = lambda n, q, rc=0: int(l.lrx_range_impact_workspace_bytes(n, q, rc))
    for ws in (sq, pq, im):
        sizes_q = [ws(100_000, q) for q in (1, 2, 16, 64, 256, 1000)]
        sizes_n = [ws(n, 16) for n in (1, 1000, 20_000, 100_000, 5_000_000)]
        assert sizes_q[0] > 0 and sizes_q == sorted(sizes_q) and sizes_q[2] > sizes_q[0], sizes_q
        assert sizes_n == sorted(sizes_n) and sizes_n[-1] > sizes_n[0], sizes_n
    # the fp16-SQ chain walks 256 queries per chunk: the workspace stops growing there
    assert sq(100_000, 1000) == sq(100_000, 256) > sq(100_000, 200)
    # the scan-driver formats keep the per-segment counts of ALL queries of a call: they keep growing, and a smaller row chunk shrinks the matrix
    assert pq(100_000, 2000) > pq(100_000, 1000) and im(100_000, 2000) > im(100_000, 1000)
    assert pq(100_000, 16, 1024) < pq(100_000, 16) and im(100_000, 16, 1024) < im(100_000, 16)


FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work


def _sq(l, *, radius=0.5, capacity=10, out=FAKE, dim=64, n_rows=1000, bounds=FAKE):
    return l.lrx_sq_fp16_ip_range_search(FAKE, n_rows, dim, bounds, FAKE, 4, radius, 0, FAKE, out, out, capacity, FAKE, 1 << 30, None)


def _pq(l, *, radius=0.5, capacity=10, out=FAKE, row_chunk=0, n_rows=1000, M=8):
    return l.lrx_pq_ip_range_search(FAKE, n_rows, FAKE, 32, M, FAKE, 4, radius, 0, FAKE, out, out, capacity, FAKE, 1 << 30, None, row_chunk)


def _impact(l, *, radius=0.5, capacity=10, out=FAKE, row_chunk=0, n_rows=1000, window_rows=0):
    return l.lrx_range_impact_search(FAKE, FAKE, 10, n_rows, FAKE, FAKE, FAKE, 4, radius, 0, FAKE, out, out, capacity, FAKE, 1 << 30, window_rows,
                                     None, row_chunk)


@pytest.mark.parametrize("call,cases", [
    (_sq, [(dict(radius=math.nan), b"NaN"), (dict(capacity=-1), b"capacity"), (dict(out=None), b"null outputs"), (dict(dim=96), b"dim=96"),
           (dict(bounds=None), b"row_bounds"), (dict(n_rows=-5), b"rows")]),
    (_pq, [(dict(radius=math.nan), b"NaN"), (dict(capacity=-1), b"capacity"), (dict(out=None), b"null outputs"), (dict(row_chunk=100), b"row_chunk=100"),
           (dict(row_chunk=-128), b"row_chunk=-128"), (dict(M=5), b"M=5"), (dict(n_rows=-5), b"rows")]),
    (_impact, [(dict(radius=math.nan), b"NaN"), (dict(capacity=-1), b"capacity"), (dict(out=None), b"null outputs"), (dict(row_chunk=130), b"row_chunk=130"),
               (dict(window_rows=100), b"window_rows=100"), (dict(n_rows=1 << 31), b"int32 row")]),
])
def test_argument_errors_are_reported_without_a_gpu(call, cases):
    l = _lib.lib()
    for kw, msg in cases:
        assert call(l, **kw) == -1, kw                # LRX_ERR_INVALID
        assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())


def test_short_workspace_is_refused():
    l = _lib.lib()
    for name, rc in (("sq", l.lrx_sq_fp16_ip_range_search(FAKE, 1000, 64, FAKE, FAKE, 4, 0.5, 0, FAKE, FAKE, FAKE, 10, FAKE, 16, None)),
                     ("pq", l.lrx_pq_ip_range_search(FAKE, 1000, FAKE, 32, 8, FAKE, 4, 0.5, 0, FAKE, FAKE, FAKE, 10, FAKE, 16, None, 0)),
                     ("impact", l.lrx_range_impact_search(FAKE, FAKE, 10, 1000, FAKE, FAKE, FAKE, 4, 0.5, 0, FAKE, FAKE, FAKE, 10, FAKE, 16, 0, None, 0))):
        assert rc == -3, name                            # LRX_ERR_WORKSPACE


def test_sq8_range_search_names_the_follow_up():
    from lightretriever_amd.index import SQ8Index
    idx = SQ8Index.__new__(SQ8Index)                 # (no GPU here: the refusal needs no state)
    with pytest.raises(NotImplementedError, match="band rescoring"):
        idx.range_search(np.zeros((1, 64), np.float32), 0.0)


def test_binary_range_search_stays_refused():
    from lightretriever_amd.retriever import FaissBinaryIndex
    with pytest.raises(NotImplementedError):
        FaissBinaryIndex.range_search(FaissBinaryIndex.__new__(FaissBinaryIndex), None, 0.0)


def test_yardstick_agrees_with_a_double_loop_on_50_rows():
    rng = np.random.default_rng(3)
    n, d, Q = 50, 64, 4
    q = rng.standard_normal((Q, d)).astype(np.float32)
    codes = rng.standard_normal((n, d)).astype(np.float16)
    S = RY.sq_fp16_scores(q, codes)
    assert S.dtype == np.float32 and S.shape == (Q, n)
    for qi in range(Q):                               # the score itself: one fp64 dot per row, rounded once
        for r in (0, 17, n - 1):
            assert S[qi, r] == np.float32(np.dot(q[qi].astype(np.float64), codes[r].astype(np.float64)))
    srt = np.sort(S.ravel())
    for radius in (-np.inf, np.inf, float(srt[len(srt) // 2]), float(srt[-1]), float(srt[0]), 0.0):
        got, want = RY.range_dense(S, radius, id_base=7), RY.brute_force(S.tolist(), radius, id_base=7)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    # strictly greater: the row that holds the radius itself is out, everything above it is in
    lims, D, I = RY.range_dense(S[:1], float(srt[-1]))
    assert lims.tolist() == [0, 0] and D.size == 0
    assert RY.range_dense(S, np.inf)[0].tolist() == [0] * (Q + 1) and RY.range_dense(S, -np.inf)[0][-1] == Q * n

    # PQ: the score function is pq_yardstick's; the keep rule is the same
    C = rng.standard_normal((4, 256, 4)).astype(np.float32)
    pc = rng.integers(0, 256, size=(n, 4)).astype(np.uint8)
    qp = rng.standard_normal((3, 16)).astype(np.float32)
    Sp = RY.pq_scores(qp, C, pc)
    r = float(np.sort(Sp.ravel())[-20])
    for a, b in zip(RY.range_dense(Sp, r), RY.brute_force(Sp.tolist(), r)):
        assert np.array_equal(a, b)

    # impact: hits only, even under a negative radius
    docs = [(rng.choice(12, 3, replace=False), rng.integers(1, 9, 3)) for _ in range(n)]
    yard = IY.Yardstick(*IY.csr_of(docs))
    queries = [([0, 1], [1, 2]), ([5], [3]), ([], [])]
    Si = RY.impact_scores(yard, queries)
    assert Si.dtype == np.int64 and (Si[2] == 0).all() and (Si[0] == 0).any() and (Si[0] > 0).any()
    for radius in (-1.0, 0.0, 4.0, float(Si.max()), np.inf, -np.inf):
        got = RY.range_impact(Si, radius)
        want = RY.brute_force(Si.astype(np.float32).tolist(), radius, hits=(Si >= 1).tolist())
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    lims, D, I = RY.range_impact(Si, -1.0)
    assert lims[1] == (Si[0] >= 1).sum() and lims[3] == lims[2] and (D >= 1).all()
