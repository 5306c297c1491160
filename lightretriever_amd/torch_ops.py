"""torch.ops.lrx.*: the PyTorch custom-op binding of liblrx (csrc/lrx_torch.cpp, TORCH_LIBRARY), SURVEY.md 8b last row.

    from lightretriever_amd import torch_ops          # loads liblrx_torch.so once; raises if it has not been built
    torch.ops.lrx.encode_packed(ids, cu_seqlens, max_seqlen, enc.handle, out, mrl_dim, normalize)
    D, I = torch.ops.lrx.flat_ip_topk(q, X, k)

Same kernels, same results as the ctypes binding (`_lib`): both call the C ABI of include/lrx.h; this one takes tensors, uses the
current HIP stream, allocates workspaces from PyTorch's caching allocator and raises RuntimeError (TORCH_CHECK) on liblrx errors.
There is no fallback: without liblrx_torch.so importing this module fails.

The argument contract (checked by the binding before its first allocation, every refusal a RuntimeError naming the op and the argument;
tests/torch_op_cases.py annotates every argument of every op with it):
  * all tensors of a call live on one device, that of the op's first tensor; the call runs on that device's current stream whichever device
    is current.  CPU tensors and tensors of another device are refused;
  * dtype and rank are exact.  A tensor is contiguous unless documented as "rows may be strided": 2-D, unit column stride, row stride >= the
    width (x, out, cand, probes, probe_scores, reps); a single row has no stride of its own, its leading dimension is its width;
  * data operands -- fp32 / 16-bit / uint8 rows, codes, tables, postings -- start at a 16-byte aligned address (any tensor PyTorch allocates,
    any row slice of one whose row is a multiple of 16 bytes); `ld % 4 == 0` is the library's check.  sparse_compact_csr's reps and
    linear_transform's x / A / b are exempt (their kernels fall back to 4-byte loads), index arrays (int32 / int64) need their natural
    alignment only;
  * an optional tensor that is given is checked like a required one;
  * an `int` the C ABI takes as int32 (k, binary_k, flags, window_rows, max_seqlen, mrl_dim, out_dim, the head counts, max_scan_rows,
    quantization_factor, and every tensor size that becomes one) is range-checked, k and binary_k against 1 .. 2048 (flat_ip_topk leaves k's
    upper bound to the library); id_base, n_rows, row0, shadow_row0, row_chunk and padding_idx are int64 all the way.
OPS lists the registered names; it is read from the registration when the library is loaded."""
import os

import torch

from . import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
TORCH_LIB_PATH = os.path.join(HERE, "liblrx_torch.so")
# The names TORCH_LIBRARY(lrx, ...) registered, sorted: filled by load() from the dispatcher's own list (a private torch call, the only one that
# lists a namespace), never kept by hand.  `hasattr(torch.ops.lrx, op) for op in OPS` therefore says only that the library loaded;
# tests/test_torch_op_cases_host.py compares OPS with the m.def lines of lrx_torch.cpp and with the case table.
OPS = ()
# the operands documented as "rows may be strided" (the contract above; the case table's annotations must name exactly these)
ROWS_MAY_STRIDE = ("x", "out", "cand", "probes", "probe_scores", "reps")

_loaded = False


def load():
    global _loaded
    if not _loaded:
        if not os.path.exists(TORCH_LIB_PATH):
            raise _lib.LrxError(f"{TORCH_LIB_PATH} not found: build it with `python -m lightretriever_amd.build`; there is no fallback")
        _lib.lib()                                  # liblrx.so first (same file the registration layer links against)
        torch.ops.load_library(TORCH_LIB_PATH)
        global OPS
        OPS = tuple(sorted(name.split("::", 1)[1].split(".")[0] for name in torch._C._dispatch_get_all_op_names() if name.startswith("lrx::")))
        if not OPS:
            raise _lib.LrxError(f"{TORCH_LIB_PATH} registered no torch.ops.lrx.* op")
        _loaded = True
    return torch.ops.lrx


load()
