"""CPU: the range-search entry points (lrx_flat_ip_range_workspace_bytes / lrx_flat_ip_range_search) are declared, exported and bound, size
their workspace sensibly and reject bad arguments with a message -- all before any device work."""
import ctypes
import math
import os

from lightretriever_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE_SYMBOLS = ("lrx_flat_ip_range_workspace_bytes", "lrx_flat_ip_range_search")


def test_range_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "lrx.h")).read()
    l = ctypes.CDLL(build.build(verbose=False))
    for s in RANGE_SYMBOLS:
        assert s + "(" in hdr, s
        assert hasattr(l, s), s
        assert s in _lib.SIGNATURES, s
    assert "#define LRX_ABI_VERSION 9" in hdr


def test_range_workspace_grows_with_rows_and_queries_up_to_one_chunk():
    l = _lib.lib()
    ws = lambda n, d, q, sh: int(l.lrx_flat_ip_range_workspace_bytes(n, d, q, sh))
    for sh in (0, 1):
        assert ws(100_000, 1024, 1, sh) > 0
        assert ws(200_000, 1024, 16, sh) > ws(100_000, 1024, 16, sh)
        assert ws(100_000, 1024, 64, sh) > ws(100_000, 1024, 16, sh)
    # with a shadow the list path walks 256 queries per chunk: the workspace grows up to 256 queries, then stays
    assert ws(100_000, 1024, 256, 1) > ws(100_000, 1024, 200, 1)
    assert ws(100_000, 1024, 1000, 1) == ws(100_000, 1024, 256, 1)
    # without one (score-matrix path) the chunk is 128 queries
    assert ws(100_000, 1024, 1000, 0) == ws(100_000, 1024, 128, 0) > ws(100_000, 1024, 100, 0)


def _call(l, *, bounds=True, dim=64, n_rows=1000, capacity=10, radius=0.5):
    fake = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work
    return l.lrx_flat_ip_range_search(fake, n_rows, dim, dim, None, fake if bounds else None, fake, 4, radius, 0, fake, fake, fake, capacity,
                                      fake, 1 << 30, None)


def test_range_argument_errors_are_reported_without_a_gpu():
    l = _lib.lib()
    cases = [(dict(bounds=False), b"row_bounds"), (dict(capacity=-1), b"capacity"), (dict(radius=math.nan), b"NaN"), (dict(dim=66), b"dim=66"),
             (dict(n_rows=-5), b"rows")]
    for kw, msg in cases:
        assert _call(l, **kw) == -1, kw                # LRX_ERR_INVALID
        assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())
