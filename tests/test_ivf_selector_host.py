"""CPU: the row selector of the four inverted-file indexes (lrx_selector_*, lrx_ivf_*_ip_search_sel / lrx_ivf_*_ip_range_search_sel,
torch.ops.lrx.ivf_*_sel, RowSelector) as far as no GPU is needed -- the exported symbols and their signatures against the plain
siblings', the op schemas, every argument refusal of the eight C entry points through fake pointers (the sibling's, under the entry's own
name, plus sel_rows), the selector entries' own refusals, and the numpy yardstick (tests/ivf_selector_yardstick.py) on hand-made cases."""
import ctypes

import numpy as np
import pytest

from lightretriever_amd import _lib

import ivf_selector_yardstick as S

FAKE = ctypes.c_void_p(256)                       # never dereferenced: every check below runs before any device work
NAN = float("nan")
FAMILIES = ("flat", "sq_fp16", "sq8", "pq")
KINDS = ("search", "range_search")
SELECTOR_ENTRIES = ("lrx_selector_fill", "lrx_selector_from_mask", "lrx_selector_set_rows", "lrx_selector_invert")


# ---- symbols and schemas ---------------------------------------------------------------------------------------------------------------
def test_the_twelve_symbols_are_exported_and_bound_and_the_abi_stays_9():
    l = _lib.lib()
    for name in SELECTOR_ENTRIES:
        assert callable(getattr(l, name)) and name in _lib.SIGNATURES
    for fam in FAMILIES:
        for kind in KINDS:
            plain, name = f"lrx_ivf_{fam}_ip_{kind}", f"lrx_ivf_{fam}_ip_{kind}_sel"
            assert callable(getattr(l, name)) and name in _lib.SIGNATURES
            res, args = _lib.SIGNATURES[name]
            pres, pargs = _lib.SIGNATURES[plain]
            # the sibling's list with (sel_bits, sel_rows) in front of (workspace, workspace_bytes, stream)
            assert res is pres and len(args) == len(pargs) + 2
            assert args[:len(pargs) - 3] == pargs[:-3] and args[-3:] == pargs[-3:]
            assert args[-5:-3] == [ctypes.c_void_p, ctypes.c_int64]
    assert l.lrx_abi_version() == 9 == _lib.ABI_VERSION


def test_the_header_declares_them_with_the_two_arguments_before_the_workspace():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lrx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for fam in FAMILIES:
        for kind in KINDS:
            m = re.search(r"\bint lrx_ivf_%s_ip_%s_sel\((.*?)\);" % (fam, kind), src, re.S)
            p = re.search(r"\bint lrx_ivf_%s_ip_%s\((.*?)\);" % (fam, kind), src, re.S)
            params = [" ".join(x.split()) for x in m.group(1).split(",")]
            plain = [" ".join(x.split()) for x in p.group(1).split(",")]
            assert params == plain[:-3] + ["const uint32_t* sel_bits", "int64_t sel_rows"] + plain[-3:], (fam, kind)
    assert "#define LRX_ABI_VERSION 9" in hdr


def test_the_eight_ops_are_registered_with_the_one_added_tensor():
    import torch
    from lightretriever_amd import ops, torch_ops
    for fam in FAMILIES:
        for plain in (f"ivf_{fam}_ip_topk", f"ivf_{fam}_ip_range_search"):
            name = plain + "_sel"
            assert name in torch_ops.OPS and callable(getattr(ops, name))
            schema = str(getattr(torch.ops.lrx, name).default._schema)
            want = str(getattr(torch.ops.lrx, plain).default._schema)
            assert schema.count("Tensor? sel, ") == 1
            assert schema.replace("Tensor? sel, ", "").replace(name + "(", plain + "(") == want, (schema, want)
            # ... at the end of the positional tensors: what follows it are the scalars, then the defaulted id_base / row_map
            head, tail = schema.split("Tensor? sel, ")
            assert head.endswith("Tensor probes, " if fam == "flat" else "Tensor? probe_scores, ")
            assert "Tensor" not in tail.split(") ->")[0].replace("Tensor? row_map=None", "")


# ---- the C entry points, without a GPU -----------------------------------------------------------------------------------------------------
def _call(l, fam, kind="search", rows=FAKE, n_rows=1000, dim=64, nlist=16, n_queries=4, nprobe=4, ld_probe=None, by_residual=1, max_scan=500, k=10,
          radius=0.5, lims=FAKE, capacity=100, ws_bytes=1 << 30, probe_scores=FAKE, out=FAKE, M=8, qtype=0, trained=FAKE, ldx=None, sel=FAKE,
          sel_rows=None):
    ld = nprobe if ld_probe is None else ld_probe
    sel_rows = n_rows if sel_rows is None else sel_rows
    if kind == "search":
        tail = (max_scan, k, 0, out, out, None, sel, sel_rows, FAKE, ws_bytes, None)
    else:
        tail = (max_scan, radius, 0, lims, out, out, capacity, None, sel, sel_rows, FAKE, ws_bytes, None)
    fn = getattr(l, f"lrx_ivf_{fam}_ip_{kind}_sel")
    if fam == "flat":
        return fn(rows, n_rows, dim if ldx is None else ldx, dim, FAKE, FAKE, nlist, FAKE, n_queries, FAKE, nprobe, ld, *tail)
    mid = (FAKE, FAKE, nlist, FAKE, n_queries, FAKE, probe_scores, nprobe, ld, by_residual)
    if fam == "sq_fp16":
        return fn(rows, n_rows, dim, *mid, *tail)
    if fam == "sq8":
        return fn(rows, n_rows, dim, trained, qtype, *mid, *tail)
    return fn(rows, n_rows, FAKE, dim, M, *mid, *tail)


COMMON = [(dict(nprobe=0), b"nprobe=0"), (dict(nprobe=17), b"nprobe=17"), (dict(nlist=4096, nprobe=2049), b"nprobe=2049"),
          (dict(nprobe=4, ld_probe=3), b"ld_probe=3"), (dict(nlist=0), b"nlist=0"), (dict(max_scan=-1), b"max_scan_rows=-1"),
          (dict(max_scan=1 << 31), b"max_scan_rows=2147483648"), (dict(n_rows=1 << 32), b"rows=4294967296"), (dict(n_queries=-1), b"n_queries=-1"),
          (dict(out=None), b"null pointer"), (dict(sel_rows=999), b"sel_rows=999"), (dict(sel_rows=0), b"sel_rows=0"), (dict(sel_rows=1024), b"sel_rows=1024")]
OF_KIND = {"search": [(dict(k=0), b"k=0"), (dict(k=2049), b"k=2049")],
           "range_search": [(dict(radius=NAN), b"radius is NaN"), (dict(capacity=-1), b"capacity=-1"), (dict(lims=None), b"null lims")]}
CELL_MAJOR_DIM = [(dict(dim=48), b"dim=48"), (dict(dim=0), b"dim=0"), (dict(dim=8224), b"dim=8224")]
CODED = [(dict(probe_scores=None), b"by_residual=1 needs probe_scores")]
OWN = {"flat": CELL_MAJOR_DIM + [(dict(ldx=60), b"ldx=60"), (dict(rows=ctypes.c_void_p(264)), b"16-byte aligned")],
       "sq_fp16": CELL_MAJOR_DIM + CODED + [(dict(rows=ctypes.c_void_p(264)), b"codes must be 16-byte aligned")],
       "sq8": CELL_MAJOR_DIM + CODED + [(dict(rows=ctypes.c_void_p(264)), b"codes must be 16-byte aligned"), (dict(qtype=1), b"qtype=1"),
                                        (dict(trained=None), b"trained")],
       "pq": CODED + [(dict(dim=60), b"dim=60 is not a multiple of M=8"), (dict(M=0), b"M=0")]}


@pytest.mark.parametrize("fam, kind, kw, msg", [(f, kd, kw, msg) for f in FAMILIES for kd in KINDS for kw, msg in COMMON + OF_KIND[kd] + OWN[f]])
def test_argument_errors_are_reported_without_a_gpu_under_the_entrys_own_name(fam, kind, kw, msg):
    l = _lib.lib()
    assert _call(l, fam, kind, **kw) == -1, kw             # LRX_ERR_INVALID
    assert msg in l.lrx_last_error(), (kw, l.lrx_last_error())
    assert f"ivf_{fam}_ip_{kind}_sel:".encode() in l.lrx_last_error()


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_short_workspace_is_reported_only_after_every_argument_check_passed(fam, kind):
    l = _lib.lib()
    assert _call(l, fam, kind, sel_rows=999, ws_bytes=0) == -1 and b"sel_rows=999" in l.lrx_last_error() and b"n_rows=1000" in l.lrx_last_error()
    assert _call(l, fam, kind, ws_bytes=16) == -3 and b"workspace" in l.lrx_last_error()           # LRX_ERR_WORKSPACE
    assert f"ivf_{fam}_ip_{kind}_sel:".encode() in l.lrx_last_error()
    # no selector: the plain entry under this name -- sel_rows is not looked at
    assert _call(l, fam, kind, sel=None, sel_rows=7, ws_bytes=16) == -3
    # the workspace is the sibling's own
    args = (1000, 16, 64) + ((8,) if fam == "pq" else ()) + (4, 4) + ((10,) if kind == "search" else ()) + (500,)
    need = getattr(l, f"lrx_ivf_{fam}_ip_workspace_bytes" if kind == "search" else f"lrx_ivf_{fam}_ip_range_workspace_bytes")(*args)
    assert _call(l, fam, kind, ws_bytes=need - 1) == -3
    # n_queries == 0 with a selector launches nothing for a top-k search (nothing to write)
    if kind == "search":
        assert _call(l, fam, kind, n_queries=0, ws_bytes=0) == 0


def test_the_selector_entries_refuse_bad_arguments_and_do_nothing_for_no_bits():
    l = _lib.lib()
    assert l.lrx_selector_fill(FAKE, -1, 0, None) == -1 and b"selector_fill: n_bits=-1" in l.lrx_last_error()
    assert l.lrx_selector_fill(FAKE, 1 << 32, 0, None) == -1 and b"n_bits=4294967296" in l.lrx_last_error()
    assert l.lrx_selector_fill(None, 10, 1, None) == -1 and b"selector_fill: null pointer" in l.lrx_last_error()
    assert l.lrx_selector_fill(None, 0, 1, None) == 0
    assert l.lrx_selector_from_mask(None, 10, FAKE, None) == -1 and b"selector_from_mask: null pointer" in l.lrx_last_error()
    assert l.lrx_selector_from_mask(FAKE, 10, None, None) == -1
    assert l.lrx_selector_from_mask(None, 0, None, None) == 0
    assert l.lrx_selector_from_mask(FAKE, -5, FAKE, None) == -1 and b"n_bits=-5" in l.lrx_last_error()
    assert l.lrx_selector_set_rows(FAKE, -1, 10, FAKE, None) == -1 and b"selector_set_rows: n=-1" in l.lrx_last_error()
    assert l.lrx_selector_set_rows(None, 3, 10, FAKE, None) == -1 and b"selector_set_rows: null pointer" in l.lrx_last_error()
    assert l.lrx_selector_set_rows(FAKE, 3, 10, None, None) == -1
    assert l.lrx_selector_set_rows(None, 0, 10, FAKE, None) == 0
    assert l.lrx_selector_invert(None, FAKE, 10, None) == -1 and b"selector_invert: null pointer" in l.lrx_last_error()
    assert l.lrx_selector_invert(FAKE, None, 10, None) == -1
    assert l.lrx_selector_invert(None, None, 0, None) == 0


# ---- the classes, as far as no GPU is needed ------------------------------------------------------------------------------------------------------
def test_the_search_methods_take_sel_and_the_wrapper_names_the_class_it_refuses():
    import inspect
    from lightretriever_amd import IVFFlatIndex, IVFPQIndex, IVFSQ8Index, IVFSQIndex, RowSelector
    from lightretriever_amd.retriever import FaissIndex
    from lightretriever_amd.selector import check_selector
    for cls in (IVFFlatIndex, IVFPQIndex, IVFSQIndex, IVFSQ8Index):
        for meth in ("search", "range_search_probed", "range_search_preassigned"):
            p = inspect.signature(getattr(cls, meth)).parameters
            assert "sel" in p and p["sel"].default is None, (cls, meth)
    for meth in ("search", "range_search_probed"):
        assert inspect.signature(getattr(FaissIndex, meth)).parameters["sel"].default is None

    class NotAnIVF:
        device = "cpu"
    fi = FaissIndex(NotAnIVF())
    with pytest.raises(TypeError, match="NotAnIVF"):
        fi.search(np.zeros((1, 32), np.float32), 1, sel=object())
    with pytest.raises(TypeError, match="NotAnIVF"):
        fi.range_search_probed(np.zeros((1, 32), np.float32), 0.0, sel=object())
    assert check_selector(None, 5, "cuda:0", "x") is None
    with pytest.raises(TypeError, match="RowSelector"):
        check_selector(np.ones(5, bool), 5, "cuda:0", "IVFFlatIndex.search")
    assert callable(RowSelector.from_mask) and callable(RowSelector.from_rows) and callable(RowSelector.from_range)


# ---- the yardstick on hand-made cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65])
def test_pack_and_unpack_by_hand(n):
    rng = np.random.default_rng(n)
    for mask in (np.zeros(n, bool), np.ones(n, bool), np.arange(n) % 2 == 0, np.arange(n) == n - 1, rng.random(n) < 0.5):
        w = S.pack(mask)
        assert w.dtype == np.int32 and w.shape == ((n + 31) // 32,) and S.tail_is_clear(w, n)
        assert np.array_equal(S.unpack(w, n), mask)
        for r in range(n):
            assert ((int(w.view(np.uint32)[r >> 5]) >> (r & 31)) & 1) == int(mask[r])
        assert sum(bin(int(x)).count("1") for x in w.view(np.uint32)) == int(mask.sum())
    full = S.pack(np.ones(n, bool)).view(np.uint32)
    assert int(full[-1]) == (0xFFFFFFFF if n % 32 == 0 else (1 << (n % 32)) - 1) and all(int(x) == 0xFFFFFFFF for x in full[:-1])


def test_pack_of_known_words():
    assert S.pack([True]).view(np.uint32).tolist() == [1]
    m = np.zeros(65, bool)
    m[[0, 31, 32, 63, 64]] = True
    assert S.pack(m).view(np.uint32).tolist() == [0x80000001, 0x80000001, 1]
    assert S.pack(m)[0] < 0                                      # int32 words: bit 31 is the sign
    assert not S.tail_is_clear(np.array([-1], np.int32), 31) and S.tail_is_clear(np.array([0x7FFFFFFF], np.int32), 31)


def test_filter_range_and_filter_topk_by_hand():
    lims = np.array([0, 3, 3, 7], np.int64)
    D = np.array([1.0, 5.0, 2.0, 4.0, 4.0, -1.0, 9.0], np.float32)
    I = np.array([4, 0, 2, 5, 1, 3, 0], np.int64)
    mask = np.array([False, True, True, True, True, True])       # row 0 deselected
    fl, fD, fI = S.filter_range(lims, D, I, mask)
    assert fl.tolist() == [0, 2, 2, 5] and fD.tolist() == [1.0, 2.0, 4.0, 4.0, -1.0] and fI.tolist() == [4, 2, 5, 1, 3]
    assert [x.tolist() for x in S.filter_range(lims, D, I, np.zeros(6, bool))] == [[0, 0, 0, 0], [], []]
    same = S.filter_range(lims, D, I, np.ones(6, bool))
    assert same[0].tolist() == lims.tolist() and np.array_equal(same[1], D) and np.array_equal(same[2], I)
    tD, tI = S.filter_topk(*S.split(lims, D, I), mask, 3)
    flt = float(np.finfo(np.float32).max)
    assert tI.tolist() == [[2, 4, -1], [-1, -1, -1], [1, 5, 3]]   # ties (4.0) to the lower row; padding beyond the selected rows
    assert tD.tolist() == [[2.0, 1.0, -flt], [-flt, -flt, -flt], [4.0, 4.0, -1.0]]
    # a 2-D unfiltered top-k with padding is a full result too
    D2 = np.array([[5.0, 2.0, 1.0, -flt]], np.float32)
    I2 = np.array([[0, 2, 4, -1]], np.int64)
    assert S.filter_topk(D2, I2, mask, 2)[1].tolist() == [[2, 4]] and S.filter_topk(D2, I2, np.ones(6, bool), 4)[1].tolist() == I2.tolist()
    # score order is the order of the bits: -0.0 below +0.0, negatives by magnitude
    D3 = [np.array([-0.0, 0.0, -2.0, -1.0], np.float32)]
    assert S.filter_topk(D3, [np.array([0, 1, 2, 3])], np.ones(4, bool), 4)[1].tolist() == [[1, 0, 3, 2]]
