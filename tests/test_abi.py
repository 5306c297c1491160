"""CPU: liblrx.so builds, loads and exports every symbol include/lrx.h declares; the ctypes table covers them all."""
import ctypes
import os
import re

from lightretriever_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "lrx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lrx_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_header_symbols():
    path = build.build(verbose=False)
    assert os.path.exists(path)
    l = ctypes.CDLL(path)
    syms = declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(l, s), f"{s} declared in include/lrx.h but not exported"
    assert sorted(_lib.SIGNATURES) == syms, "ctypes signature table out of sync with include/lrx.h"
    assert _lib.lib().lrx_abi_version() == _lib.ABI_VERSION == 9


def test_shipping_library_reads_no_environment_variable():
    """the A/B switches of the tools (sample stride, tile groups, fused-launch phases, ...) live behind -DLRX_DEV_KNOBS; the
    shipping liblrx.so neither imports getenv nor carries the knob names -- its behaviour depends on its arguments alone."""
    import re
    import subprocess
    from lightretriever_amd import _lib
    assert os.path.basename(_lib.LIB_PATH) == "liblrx.so" or os.environ.get("LRX_LIB_DEV_VARIANT")
    lib = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "liblrx.so")
    syms = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\bU (secure_)?getenv\b", syms), [l for l in syms.splitlines() if "getenv" in l]
    blob = open(lib, "rb").read()
    for knob in (b"LRX_SS_FORCE", b"LRX_SS_MAX", b"LRX_SEARCH_FUSED", b"LRX_FUSED_PHASES", b"LRX_EMIT_PERSIST_MIN_BPC", b"LRX_GEMM_GM", b"LRX_MAXAGG_GM",
                 b"LRX_ATTN_TILED", b"LRX_SEARCH_WIDE_MAX", b"LRX_EMIT_GM"):
        assert knob not in blob, knob
    # ... and no source under csrc/ calls getenv outside the dev-knob helper
    csrc = os.path.join(os.path.dirname(lib), "csrc")
    hits = [(f, i + 1) for f in sorted(os.listdir(csrc)) for i, l in enumerate(open(os.path.join(csrc, f), errors="replace")) if "getenv(" in l]
    assert hits == [("lrx_common.h", hits[0][1])] and len(hits) == 1, hits


def test_argument_errors_are_reported_without_a_gpu():
    l = _lib.lib()
    # invalid shapes are rejected on the host before any launch
    assert l.lrx_gemm_bf16_nt(None, None, None, None, None, 4, 8, 7, 0, None) == -1
    assert b"K=7" in l.lrx_last_error()
    assert l.lrx_attn_varlen_causal(None, None, 1, 4, 4, 4, 2, 16, None, 0, None) == -1
    # a sequence is addressed through one buffer descriptor: at 32 / 8 heads of 128, 2 GiB / 12 KiB per row = 174762 rows fit
    assert l.lrx_attn_varlen_causal(None, None, 1, 174763, 174763, 32, 8, 128, None, 0, None) == -1 and b"2 GiB" in l.lrx_last_error()
    # the work-list variant (ABI 7): same layout checks, the list must be there and large enough
    assert l.lrx_attn_varlen_causal_items(None, None, None, 0, 1, 4, 4, 4, 2, 16, None, 0, None) == -1
    assert l.lrx_attn_varlen_causal_items(None, None, None, 0, 1, 4, 4, 32, 8, 128, None, 0, None) == -1 and b"work list" in l.lrx_last_error()
    assert l.lrx_attn_build_items(None, 1, 4, 4, 32, 8, 128, 0, None, 0, None) == -1
    assert l.lrx_attn_items_bytes(1, 4, 4, 32, 8, 128, 0) >= 16 and l.lrx_attn_items_bytes(1, 4, 4, 32, 8, 100, 0) == 0
    assert l.lrx_flat_ip_scores(None, 10, 48, 48, None, 1, None, None) == -1
    assert l.lrx_flat_ip_score_ld(1000) == 1024
    assert l.lrx_encode_workspace_bytes(None, 1, 1) == 0


def test_graft_entry_build_runs_on_cpu():
    """The driver's "does it build" check: compiles (or reuses) liblrx.so for gfx950, imports the package, checks the ABI version."""
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    entry = importlib.import_module("__graft_entry__")
    entry.build()
    assert callable(entry.smoke)


def test_torch_library_registers_every_op_without_a_gpu():
    """SURVEY 8b last row: the extension exports torch.ops.lrx.* (TORCH_LIBRARY in csrc/lrx_torch.cpp, built in-tree)."""
    import torch
    assert os.path.exists(build.build_torch_ops(verbose=False))
    from lightretriever_amd import torch_ops
    for op in torch_ops.OPS:
        schema = str(getattr(torch.ops.lrx, op).default._schema)
        assert schema.startswith("lrx::" + op + "(")
    # host-side argument checks raise RuntimeError (TORCH_CHECK), never crash: CPU tensors have no CUDA kernel registered
    import pytest
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.lrx.flat_ip_topk(torch.zeros(2, 32), torch.zeros(10, 32), 3)


def test_forced_build_from_sources_compiles_every_kernel_file(tmp_path):
    """build() reuses a fresh liblrx.so, so the driver's build step may compile nothing -- this test always compiles all
    HIP sources for gfx950 (into a scratch library, the loaded one is left alone) and checks the result exports the ABI."""
    out = str(tmp_path / "liblrx_forced.so")
    path = build.build(force=True, verbose=False, out=out)
    assert path == out and os.path.getsize(out) > 1 << 20
    l = ctypes.CDLL(out)
    for s in declared_symbols():
        assert hasattr(l, s), s
    for f in os.listdir(os.path.join(ROOT, "lightretriever_amd", "build")):
        if "liblrx_forced" in f:
            os.remove(os.path.join(ROOT, "lightretriever_amd", "build", f))


def test_header_is_plain_c():
    """include/lrx.h is the boundary a non-C++ host binds (cgo / JNI / ctypes generators): it must parse as C99 and as C++11 on its own."""
    import shutil
    import subprocess
    hdr = os.path.join(ROOT, "include", "lrx.h")
    gcc, gxx = shutil.which("gcc"), shutil.which("g++")
    assert gcc and gxx
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr])
    subprocess.check_call([gxx, "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", hdr])
