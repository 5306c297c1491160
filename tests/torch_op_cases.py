"""The case table of tests/test_gpu_torch_op_contract.py: one entry per op that TORCH_LIBRARY(lrx, ...) registers -- the annotation of every
schema argument under the binding's argument contract (lightretriever_amd/torch_ops.py, csrc/lrx_torch.cpp) and, for the ops that have one, a
builder of valid arguments at the smallest shapes that still cross the layouts' seams together with the expected result.  A helper module: it
holds no tests (tests/test_torch_op_cases_host.py checks it without a GPU).

Annotations (ANN[op][argument]):
  T(dtype, rank, rows=, vec=, opt=, mut=, length=)   a tensor: rows = "rows may be strided" (include/lrx.h and the binding's comments say so
                                                      for exactly these), vec = 16-byte aligned base required, mut = the region the op may
                                                      write (None: read only), length = the rule that ties its size to other arguments
  I32(lo, hi)                                          an int the C ABI takes as int32: refused outside [lo, hi]
  I64() / F() / B()                                    int64 all the way / float / bool: no range of the binding's own
Values lie on an exact grid (small integers / 64): every product and every sum of D = 64 of them is exact in fp32 and in fp64, so the expected
scores do not depend on the order of the additions and the comparison is on bits."""
from collections import OrderedDict
from dataclasses import asdict

import numpy as np
import torch

FLT_MAX = np.float32(3.4028234663852886e38)
I32_MAX = 2 ** 31 - 1
MAX_K = 2048
Q, D, N, K = 3, 64, 300, 5                 # N = two whole 128-row blocks and a partial one
NLIST, NPROBE, M_PQ = 4, 2, 8
BIN_K = 20
GEMM_M, GEMM_K = 300, 128
ENC_LENS = (70, 1, 33)
TORCH_DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "i32": torch.int32, "i64": torch.int64, "u8": torch.uint8}


def T(dtype, rank, rows=False, vec=False, opt=False, mut=None, length=None):
    return {"kind": "tensor", "dtype": dtype, "rank": rank, "rows_may_stride": rows, "vec16": vec, "optional": opt, "mutated": mut, "length": length}


def I32(lo, hi=I32_MAX):
    return {"kind": "int", "int32": True, "range": (lo, hi)}


def I64():
    return {"kind": "int", "int32": False, "range": None}


def F():
    return {"kind": "float"}


def B():
    return {"kind": "bool"}


# ---- annotations ------------------------------------------------------------------------------------------------------------------
_Q = T("f32", 2, vec=True, length="[Q, D], D the store's width")
_X = T("f32", 2, rows=True, vec=True)
_BOUNDS = T("f32", 1, length="[2]")
_ROW_MAP = T("i64", 1, opt=True, length=">= n_rows")
_SHADOW = T("f16", 1, vec=True, opt=True, length=">= ceil(N / 128) * 128 * D (whole 128-row blocks)")
_K = I32(1, MAX_K)

ANN = {
    "encode_packed": OrderedDict(ids=T("i32", 1), cu_seqlens=T("i32", 1, length="[n_seqs + 1], >= 1: its length IS the batch, a shorter one is a smaller batch and cannot be refused"), max_seqlen=I32(1), weights=I64(),
                                 out=T("f32", 2, rows=True, vec=True, mut="rows [0, n_seqs), columns [0, mrl_dim or hidden)", length="[>= n_seqs, >= width]"),
                                 mrl_dim=I32(0, "hidden_size"), normalize=B(),
                                 shadow=T("any16", 1, vec=True, opt=True, mut="the tiled rows [shadow_row0, shadow_row0 + n_seqs)",
                                          length=">= ceil((shadow_row0 + n_seqs) / 128) * 128 * D"),
                                 shadow_row0=I64(), row_bounds=T("f32", 1, opt=True, mut="both floats", length="[2]")),
    "rmsnorm": OrderedDict(x=T("bf16", 2, vec=True), w=T("bf16", 1, vec=True, length="[H], H the width of x"), eps=F()),
    "rope_qkv_gemm": OrderedDict(a=T("bf16", 2, vec=True), wqkv=T("bf16", 2, vec=True, length="[(nq + 2 nkv) d, K]"),
                                 bias=T("bf16", 1, vec=True, opt=True, length="[(nq + 2 nkv) d]"), positions=T("i32", 1, length="[M], M the rows of a"),
                                 cos=T("f32", 2, vec=True, length="[max_positions, head_dim / 2]"), sin=T("f32", 2, vec=True, length="the shape of cos"),
                                 num_q_heads=I32(1, 65536), num_kv_heads=I32(1, 65536), head_dim=I32(2, 1024)),
    "attn_varlen": OrderedDict(qkv=T("f16", 2, vec=True, length="[T, (nq + 2 nkv) d]"), cu_seqlens=T("i32", 1, length="[n_seqs + 1], >= 1: its length IS the batch, a shorter one is a smaller batch and cannot be refused"), max_seqlen=I32(1),
                               num_q_heads=I32(1, 65536), num_kv_heads=I32(1, 65536), head_dim=I32(2, 1024)),
    "swiglu_gemm": OrderedDict(a=T("bf16", 2, vec=True), wgu=T("bf16", 2, vec=True, length="[2 I, K], K the width of a")),
    "embedding_bag_mean": OrderedDict(table=T("f32", 2, vec=True), ids=T("i64", 1), offsets=T("i64", 1), padding_idx=I64(), out_dim=I32(0, "table width"),
                                      normalize=B()),
    "flat_ip_topk": OrderedDict(q=_Q, x=_X, k=I32(1, I32_MAX), id_base=I64(), row_bounds=dict(_BOUNDS, optional=True)),
    "flat_ip_topk_bounded": OrderedDict(q=_Q, x=_X, x_shadow=_SHADOW, row_bounds=_BOUNDS, k=_K, id_base=I64(), flags=I32(0)),
    "flat_ip_topk_bounded_wire": OrderedDict(q=_Q, x=_X, x_shadow=_SHADOW, row_bounds=_BOUNDS, k=_K, id_base=I64(), row_map=_ROW_MAP, flags=I32(0)),
    "merge_topk_packed": OrderedDict(words=T("i64", 3)),
    "shard_commit_rows": OrderedDict(x=_X, x_shadow=dict(_SHADOW, mutated="the tiled rows [row0, row0 + n)", length=">= ceil((row0 + n) / 128) * 128 * D"),
                                     row_bounds=dict(_BOUNDS, mutated="both floats"), row0=I64()),
    "merge_topk": OrderedDict(d_parts=T("f32", 3), i_parts=T("i64", 3, length="the shape of d_parts")),
    "flat_ip_range_search": OrderedDict(q=_Q, x=_X, x_shadow=_SHADOW, row_bounds=_BOUNDS, radius=F(), id_base=I64()),
    "sq_fp16_ip_topk": OrderedDict(q=_Q, codes=T("f16", 1, vec=True, length=">= ceil(n_rows / 128) * 128 * D"), n_rows=I64(), row_bounds=_BOUNDS, k=_K,
                                   id_base=I64(), row_map=_ROW_MAP, flags=I32(0)),
    "flat_ip_rerank": OrderedDict(q=_Q, x=_X, cand=T("i64", 2, rows=True, length="[Q, n_cand <= 2048]"), k=_K, id_base=I64(), row_map=_ROW_MAP),
    "sq_fp16_ip_rerank": OrderedDict(q=_Q, codes=T("f16", 1, vec=True, length=">= ceil(n_rows / 128) * 128 * D"), n_rows=I64(),
                                     cand=T("i64", 2, rows=True, length="[Q, n_cand <= 2048]"), k=_K, id_base=I64(), row_map=_ROW_MAP),
    "pq_ip_topk": OrderedDict(q=_Q, codes=T("u8", 1, vec=True, length=">= ceil(n_rows / 128) * 128 * ceil(M / 16) * 16"),
                              centroids=T("f32", 3, vec=True, length="[M, 256, D / M]"), n_rows=I64(), k=_K, id_base=I64(), row_map=_ROW_MAP),
    "sq8_ip_topk": OrderedDict(q=_Q, codes=T("u8", 1, vec=True, length=">= ceil(n_rows / 128) * 128 * D"), n_rows=I64(),
                               trained=T("f32", 1, vec=True, length="[2 D] or [2]"), k=_K, id_base=I64(), row_map=_ROW_MAP),
    "impact_topk": OrderedDict(postings=T("i32", 2, vec=True, length="[nnz, 2]"), term_off=T("i64", 1, length="[n_terms + 1]"), n_rows=I64(),
                               q_off=T("i32", 1, length="[Q + 1]"), q_term=T("i32", 1, length="[q_off[Q]]"), q_cnt=T("i32", 1, length="the length of q_term"),
                               k=_K, id_base=I64(), row_map=_ROW_MAP, window_rows=I32(0)),
    "sparse_compact_csr": OrderedDict(reps=T("f32", 2, rows=True), quantization_factor=I32(1), empty_marker=B()),
    "sq_fp16_ip_range_search": OrderedDict(q=_Q, codes=T("f16", 1, vec=True, length=">= ceil(n_rows / 128) * 128 * D"), n_rows=I64(), row_bounds=_BOUNDS,
                                           radius=F(), id_base=I64()),
    "pq_ip_range_search": OrderedDict(q=_Q, codes=T("u8", 1, vec=True, length=">= ceil(n_rows / 128) * 128 * ceil(M / 16) * 16"),
                                      centroids=T("f32", 3, vec=True, length="[M, 256, D / M]"), n_rows=I64(), radius=F(), id_base=I64(), row_chunk=I64()),
    "impact_range_search": OrderedDict(postings=T("i32", 2, vec=True, length="[nnz, 2]"), term_off=T("i64", 1, length="[n_terms + 1]"), n_rows=I64(),
                                       q_off=T("i32", 1, length="[Q + 1]"), q_term=T("i32", 1, length="[q_off[Q]]"),
                                       q_cnt=T("i32", 1, length="the length of q_term"), radius=F(), id_base=I64(), window_rows=I32(0), row_chunk=I64()),
    "linear_transform": OrderedDict(x=T("f32", 2, rows=True), A=T("f32", 2, length="[d_out, d_in], d_in the width of x"), b=T("f32", 1, opt=True, length="[d_out]")),
    "binary_topk": OrderedDict(q=_Q, codes=T("u8", 1, vec=True, length=">= ceil(n_rows / 128) * 128 * ceil(D / 128) * 16"), n_rows=I64(), k=_K, binary_k=_K,
                               rerank=B(), threshold=T("any", 1, opt=True, length="1 or D values, on the host or the op's device"), id_base=I64(),
                               row_map=_ROW_MAP),
}

# the 16 inverted-file ops: four families x {top-k, range} x {plain, _sel}
_IVF_STORE = {
    "flat": [("x", _X)],
    "pq": [("codes", T("u8", 1, vec=True, length="whole 128-row blocks of ceil(M / 16) * 16 bytes per row")), ("pq_centroids", T("f32", 3, vec=True, length="[M, 256, D / M]"))],
    "sq_fp16": [("codes", T("f16", 2, vec=True, length="[n_rows, D]"))],
    "sq8": [("codes", T("u8", 2, vec=True, length="[n_rows, D]")), ("trained", T("f32", 1, vec=True, length="[2 D] (qtype 0) or [2] (qtype 2)")), ("qtype", I32(0, 2))],
}
IVF_FAMILIES = tuple(_IVF_STORE)


def _ivf_ann(fam, scalar, sel):
    a = OrderedDict(q=_Q)
    a.update(_IVF_STORE[fam])
    a["list_off"] = T("i64", 1, length="[nlist + 1], nlist >= 1")
    # (the PQ family has no row count of its own: a given row_ids IS its n_rows, which the code blocks must hold)
    a["row_ids"] = T("i64", 1, opt=True, length=">= n_rows" if fam != "pq" else "[n_rows], n_rows <= the rows the code blocks hold")
    a["probes"] = T("i64", 2, rows=True, length="[Q, nprobe]")
    if fam != "flat":
        a["probe_scores"] = T("f32", 2, rows=True, opt=True, length="the shape and row stride of probes")
    if sel:
        a["sel"] = T("i32", 1, opt=True, length="[ceil(n_rows / 32)]")
    if fam != "flat":
        a["by_residual"] = B()
    a[scalar] = _K if scalar == "k" else F()
    a["max_scan_rows"] = I32(0)
    a["id_base"] = I64()
    a["row_map"] = _ROW_MAP
    return a


def ivf_op_name(fam, kind, sel):
    return f"ivf_{fam}_ip_{'topk' if kind == 'k' else 'range_search'}{'_sel' if sel else ''}"


for _fam in IVF_FAMILIES:
    for _kind in ("k", "radius"):
        for _sel in (False, True):
            ANN[ivf_op_name(_fam, _kind, _sel)] = _ivf_ann(_fam, _kind, _sel)


def mutated(op):
    """The arguments the table marks as written."""
    return {a for a, n in ANN[op].items() if n["kind"] == "tensor" and n["mutated"]}


# ---- exact references in fp64 numpy ---------------------------------------------------------------------------------------------------
def grid(rng, shape, lim=8):
    """Multiples of 1/64 in [-lim/64, lim/64]: exact in fp16, bf16 (|n| <= 8 needs 4 bits) and fp32, and so are their products and sums."""
    return (rng.integers(-lim, lim + 1, shape) / 64.0).astype(np.float32)


def topk_fp64(q, X, k, id_base=0, row_map=None):
    """(D f32 [Q, k], I i64 [Q, k], rows i64 [Q, k]): score descending, ties to the lower row, (-FLT_MAX, -1) padding past the rows."""
    S = np.asarray(q, np.float64) @ np.asarray(X, np.float64).T
    Qn, n = S.shape
    Dd, I, R = np.full((Qn, k), -FLT_MAX, np.float32), np.full((Qn, k), -1, np.int64), np.full((Qn, k), -1, np.int64)
    for i in range(Qn):
        o = np.argsort(-S[i], kind="stable")[:k]
        Dd[i, :o.size], R[i, :o.size] = S[i, o].astype(np.float32), o
        I[i, :o.size] = id_base + o if row_map is None else np.asarray(row_map)[o]
    return Dd, I, R


def range_fp64(q, X, radius, id_base=0):
    """(lims i64 [Q + 1], D f32, I i64): the rows whose score is strictly greater than radius, ascending rows inside a query."""
    S = (np.asarray(q, np.float64) @ np.asarray(X, np.float64).T).astype(np.float32).reshape(len(q), len(X))
    lims, Dd, I = [0], [], []
    for i in range(S.shape[0]):
        hit = np.flatnonzero(S[i] > np.float32(radius))
        Dd.append(S[i, hit])
        I.append(id_base + hit)
        lims.append(lims[-1] + hit.size)
    return np.asarray(lims, np.int64), np.concatenate(Dd).astype(np.float32) if Dd else np.zeros(0, np.float32), \
        np.concatenate(I).astype(np.int64) if I else np.zeros(0, np.int64)


def pack_words(Dd, ids):
    """lrx_pack_topk's word: the score's bits in the high half, the low 32 bits of the id in the low half."""
    return (np.asarray(Dd, np.float32).view(np.int32).astype(np.int64) << 32) | (np.asarray(ids, np.int64) & 0xFFFFFFFF)


def merge_fp64(d_parts, i_parts):
    """[R, Q, k] pairs -> the best k per query: score descending, ties to the lower id, (-FLT_MAX, -1) entries last."""
    R, Qn, k = d_parts.shape
    Dd, I = np.empty((Qn, k), np.float32), np.empty((Qn, k), np.int64)
    for i in range(Qn):
        d, ids = d_parts[:, i].reshape(-1), i_parts[:, i].reshape(-1)
        o = np.lexsort((ids, -d.astype(np.float64)))[:k]
        Dd[i], I[i] = d[o], ids[o]
    return Dd, I


def tile_shadow(X16, n_blocks, row0=0):
    """Row-major fp16 [n, D], standing at rows [row0, row0 + n) -> the tiled shadow of include/lrx.h as [n_blocks * 128 * D] (zeros elsewhere) and
    the mask of the elements that belong to those rows (the inverse of _TiledIPIndex.shadow_rows: tile = [16-row group w][k-step ks][fq][fi][8],
    row 128 b + 16 w + fi, column 64 s + 32 ks + 8 fq + j)."""
    n, d = X16.shape
    rows = np.zeros((n_blocks * 128, d), np.float16)
    real = np.zeros((n_blocks * 128, d), bool)
    rows[row0:row0 + n], real[row0:row0 + n] = X16, True
    tile = lambda a: a.reshape(n_blocks, 8, 16, d // 64, 2, 4, 8).transpose(0, 3, 1, 4, 5, 2, 6).reshape(-1)
    return tile(rows), tile(real)


def bounds_fp64(X):
    """{max |row|, max |row - fp16(row)|} in fp64, rounded up to fp32 (tests/search_reference.host_bounds)."""
    from search_reference import host_bounds
    return np.asarray(host_bounds(X), np.float32)


def commit_bounds(X):
    """What lrx_shard_commit_rows leaves in zeroed row_bounds: {fl32(sqrtf(max sum x^2) * (1 + 1e-6f)), the same of x - fp16(x)} -- an upper bound by
    construction (csrc/lrx_search.hip, k_shard_rows_tiled).  On the grid the sums of squares are exact in fp32 in any order, sqrtf is correctly
    rounded (the fp64 root of an fp32 number rounds to it), and the product is one fp32 multiplication: exact to the bit."""
    X64 = np.asarray(X, np.float64)
    r2 = (X64 * X64).sum(1).max()
    e = X64 - X64.astype(np.float16).astype(np.float64)
    e2 = (e * e).sum(1).max()
    assert r2 == np.float32(r2) and e2 == 0
    up = np.float32(1.0) + np.float32(1e-6)
    return np.array([np.float32(np.sqrt(r2)) * up, np.float32(np.sqrt(e2)) * up], np.float32)


# ---- builders -----------------------------------------------------------------------------------------------------------------------------
class Built:
    """One op's valid call.  args(): the arguments by schema name, mutated ones freshly allocated; result(ret, args): the tensors the call
    produced; expect: their expected values on the CPU (exact ops) or None -- then method(args) is the class method / ops.py wrapper of the same
    C entry; canon: the order-free form of a result; written(args): per mutated argument the bool mask of the elements the op may write;
    bad_lengths(args): (argument, tensor) pairs that break a length rule, each cut from an allocation that covers the full-size tensor."""
    expect = None
    method = None
    canon = staticmethod(lambda r: r)
    int_valid = {}              # int argument -> a valid value v for the 2^32 + v case (default: the argument's own value)
    int_hi = {}                 # int argument -> its maximum, where the table names it in words

    def __init__(self, args, result=None, **kw):
        self._args = args
        self.result = result or (lambda ret, a: tuple(ret) if isinstance(ret, (tuple, list)) else (ret,))
        self.written = lambda a: {}
        self.bad_lengths = lambda a: []
        self.__dict__.update(kw)

    def args(self):
        a = self._args()
        return OrderedDict(a)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def canary(shape, dtype, device):
    """A tensor of NaNs with a payload no kernel produces (0x7FC5A5A5 / 0x7E5A); integers: 0x5A bytes."""
    t = torch.empty(shape, dtype=dtype, device=device)
    if dtype == torch.float32:
        t.view(torch.int32).fill_(0x7FC5A5A5)
    elif dtype in (torch.float16, torch.bfloat16):
        t.view(torch.int16).fill_(0x7E5A if dtype == torch.float16 else 0x7FDA)
    else:
        t.view(torch.uint8).fill_(0x5A)
    return t


def _flat_data(n=N, nq=Q, seed=0):
    rng = np.random.default_rng(seed)
    return grid(rng, (n, D)), grid(rng, (nq, D))


def _flat_store(device, X):
    """(x, its tiled fp16 shadow, its bounds) built by the project's own index class."""
    from lightretriever_amd import FlatIPIndex
    idx = FlatIPIndex(D, capacity=max(len(X), 1), device=torch.device(device))
    if len(X):
        idx.add(dev(X, device))
    nb = -(-len(X) // 128)
    xb = idx._xb[:nb * 128 * D] if idx._xb is not None else None
    return idx, idx.vectors if len(X) else torch.empty(0, D, device=device), xb, idx._bounds


def make_flat_ip_topk(device, n=N, nq=Q):
    X, q = _flat_data(n, nq)
    x, qd = dev(X, device).reshape(n, D), dev(q, device).reshape(nq, D)
    bounds = dev(bounds_fp64(X), device) if n else None
    Dd, I, _ = topk_fp64(q.reshape(nq, D), X.reshape(n, D), K, 11)
    return Built(lambda: [("q", qd), ("x", x), ("k", K), ("id_base", 11), ("row_bounds", bounds)], expect=(Dd, I),
                 bad_lengths=lambda a: [("row_bounds", torch.zeros(2, device=device)[:1]), ("q", torch.zeros(Q, D + 64, device=device)[:, :D + 4].contiguous())])


def _bounded(device, wire, n=N, nq=Q):
    X, q = _flat_data(n, nq)
    idx, x, xb, bounds = _flat_store(device, X)
    qd = dev(q, device).reshape(nq, D)
    row_map = np.arange(n, dtype=np.int64) * 2 + 1
    Dd, I, R = topk_fp64(q.reshape(nq, D), X.reshape(n, D), K, 7)
    args = [("q", qd), ("x", x), ("x_shadow", xb), ("row_bounds", bounds), ("k", K), ("id_base", 7)]
    if wire:
        args += [("row_map", dev(row_map, device))]
        W = pack_words(Dd, np.where(R >= 0, row_map[np.maximum(R, 0)] if n else -1, -1))
    args += [("flags", 0)]
    short = lambda a: [("row_bounds", torch.zeros(2, device=device)[:1]), ("x_shadow", a["x_shadow"][:a["x_shadow"].numel() - 128 * D]),
                       ("q", torch.zeros(Q, D + 64, device=device)[:, :D + 4].contiguous())] + \
        ([("row_map", a["row_map"][:n - 1])] if wire else [])
    return Built(lambda: args, expect=(Dd, I, W) if wire else (Dd, I), bad_lengths=short, keep=idx)


def make_flat_ip_topk_bounded(device, **kw):
    return _bounded(device, False, **kw)


def make_flat_ip_topk_bounded_wire(device, **kw):
    return _bounded(device, True, **kw)


def make_flat_ip_range_search(device, n=N, nq=Q):
    X, q = _flat_data(n, nq)
    idx, x, xb, bounds = _flat_store(device, X)
    qd = dev(q, device).reshape(nq, D)
    radius = 0.03125
    return Built(lambda: [("q", qd), ("x", x), ("x_shadow", xb), ("row_bounds", bounds), ("radius", radius), ("id_base", 5)],
                 expect=range_fp64(q.reshape(nq, D), X.reshape(n, D), radius, 5), keep=idx,
                 bad_lengths=lambda a: [("row_bounds", torch.zeros(2, device=device)[:1]), ("x_shadow", a["x_shadow"][:a["x_shadow"].numel() - 128 * D])])


def make_flat_ip_rerank(device, nq=Q):
    import refine_yardstick as RY
    X, q = _flat_data(N, nq)
    rng = np.random.default_rng(3)
    cand = np.stack([rng.permutation(N)[:20] for _ in range(max(nq, 1))]).astype(np.int64)[:nq]
    cand[:, 3] = -1                                                  # a skipped entry
    row_map = np.arange(N, dtype=np.int64) * 3 + 2
    rm = dev(row_map, device)
    x, qd, cd = dev(X, device), dev(q, device).reshape(nq, D), dev(cand, device)
    return Built(lambda: [("q", qd), ("x", x), ("cand", cd), ("k", K), ("id_base", 50), ("row_map", rm)], expect=RY.rerank(q.reshape(nq, D), X, cand, K, 50, row_map),
                 bad_lengths=lambda a: [("row_map", rm[:N - 1]), ("cand", cd[:Q - 1]), ("q", torch.zeros(Q, D + 64, device=device)[:, :D + 4].contiguous())])


def _parts(seed=5, R=3, k=K):
    rng = np.random.default_rng(seed)
    d = np.sort(grid(rng, (R, Q, k), 40), axis=2)[:, :, ::-1].copy()
    i = np.stack([np.stack([rng.permutation(1000)[:k] + 1000 * r for _ in range(Q)]) for r in range(R)]).astype(np.int64)
    d[R - 1, :, k - 2:], i[R - 1, :, k - 2:] = -FLT_MAX, -1                # a part that ran out of rows
    return d, i


def make_merge_topk(device):
    d, i = _parts()
    dd, ii = dev(d, device), dev(i, device)
    return Built(lambda: [("d_parts", dd), ("i_parts", ii)], expect=merge_fp64(d, i), bad_lengths=lambda a: [("i_parts", ii[:, :, :K - 1].contiguous()), ("d_parts", dd[:2])])


def make_merge_topk_packed(device):
    d, i = _parts()
    w = dev(pack_words(d, i), device)
    return Built(lambda: [("words", w)], expect=merge_fp64(d, i))


def make_shard_commit_rows(device, n=N - 40, row0=40):
    """Rows [row0, row0 + n) of a 300-row shard: the shadow's other rows, and the padding rows of its partial last block, keep their canary."""
    X, _ = _flat_data(n)
    x = dev(X, device).reshape(n, D)
    nb = -(-(row0 + n) // 128)
    tiled, mask = tile_shadow(X.astype(np.float16).reshape(n, D), nb, row0)
    want_b = commit_bounds(X) if n else np.zeros(2, np.float32)

    def args():
        return [("x", x), ("x_shadow", canary(nb * 128 * D, torch.float16, device)), ("row_bounds", torch.zeros(2, device=device)), ("row0", row0)]

    def result(ret, a):
        assert ret is None
        return (torch.where(dev(mask, device), a["x_shadow"], torch.zeros((), dtype=torch.float16, device=device)), a["row_bounds"])
    return Built(args, result, expect=(np.where(mask, tiled, np.float16(0)), want_b),
                 written=lambda a: {"x_shadow": torch.from_numpy(mask), "row_bounds": torch.ones(2, dtype=torch.bool)},
                 bad_lengths=lambda a: [("row_bounds", torch.zeros(2, device=device)[:1]), ("x_shadow", a["x_shadow"][:nb * 128 * D - 1])])


def make_linear_transform(device, n=N):
    rng = np.random.default_rng(7)
    X, A, b = grid(rng, (n, D)), grid(rng, (24, D)), grid(rng, (24,))
    want = (X.astype(np.float64) @ A.astype(np.float64).T + b.astype(np.float64)).astype(np.float32)
    x, Ad, bd = dev(X, device), dev(A, device), dev(b, device)
    return Built(lambda: [("x", x), ("A", Ad), ("b", bd)], expect=(want,), bad_lengths=lambda a: [("b", bd[:23]), ("A", Ad[:, :D - 4].contiguous())])


def make_embedding_bag_mean(device):
    """Bags of 1, 2, 4 and 8 ids (a power of two: the mean of grid values is exact), one empty bag, one id equal to padding_idx."""
    rng = np.random.default_rng(8)
    table = grid(rng, (N, D))
    ids = rng.integers(1, N, 16).astype(np.int64)
    offs = np.array([0, 1, 3, 7, 7], np.int64)                             # bags [0,1) [1,3) [3,7) [7,7) [7,16): 1, 2, 4, 0 and 9 ids
    ids[[5, 6, 7]] = 0                                                     # padding_idx, left out of its bag: 4 -> 2 and 9 -> 8 ids that count
    want = np.zeros((5, D), np.float64)
    for b in range(5):
        e = ids[offs[b]:(offs[b + 1] if b + 1 < 5 else 16)]
        e = e[e != 0]
        if e.size:
            want[b] = table[e].astype(np.float64).sum(0) / e.size
    t, i, o = dev(table, device), dev(ids, device), dev(offs, device)
    return Built(lambda: [("table", t), ("ids", i), ("offsets", o), ("padding_idx", 0), ("out_dim", 0), ("normalize", False)], expect=(want.astype(np.float32),),
                 int_valid={"out_dim": 32}, int_hi={"out_dim": D})


def make_sparse_compact_csr(device):
    """reps [5, 300]: zeros, negatives (clamped), values whose quantised weight is 0, an all-zero row (the empty marker's) and a full row."""
    import sparse_reference as SR
    rng = np.random.default_rng(9)
    V = 300
    reps = (rng.integers(-64, 257, (5, V)) / 64.0).astype(np.float32) * (rng.random((5, V)) < 0.2)
    reps = reps.astype(np.float32)
    reps[2] = 0
    reps[4] = np.abs(reps[4]) + 1
    ids, weights, counts = SR.compact(reps, 100)
    off, terms, wts = [0], [], []
    for r in range(5):
        if counts[r] == 0:                                                 # empty_marker: the pair (V, 1) keeps the row
            terms.append(np.full(1, V, np.int32))
            wts.append(np.ones(1, np.int32))
        else:
            terms.append(ids[r])
            wts.append(weights[r])
        off.append(off[-1] + terms[-1].size)
    rd = dev(reps, device)
    return Built(lambda: [("reps", rd), ("quantization_factor", 100), ("empty_marker", True)],
                 expect=(np.asarray(off, np.int64), np.concatenate(terms).astype(np.int32), np.concatenate(wts).astype(np.int32)))


def make_rope_qkv_gemm(device, bias=True):
    from lightretriever_amd import ops
    rng = np.random.default_rng(10)
    nq, nkv, d = 4, 2, 64
    a = dev(grid(rng, (GEMM_M, GEMM_K)), device).bfloat16()
    w = dev(grid(rng, ((nq + 2 * nkv) * d, GEMM_K)), device).bfloat16()
    bs = dev(grid(rng, ((nq + 2 * nkv) * d,)), device).bfloat16() if bias else None
    cu = torch.tensor([0, 100, 101, GEMM_M], dtype=torch.int32, device=device)
    pos = ops.build_positions(cu, GEMM_M)
    ang = torch.arange(256, device=device)[:, None] * 0.01 * torch.arange(d // 2, device=device)[None, :]
    cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    return Built(lambda: [("a", a), ("wqkv", w), ("bias", bs), ("positions", pos), ("cos", cos), ("sin", sin), ("num_q_heads", nq), ("num_kv_heads", nkv),
                          ("head_dim", d)],
                 method=lambda g: (ops.gemm_qkv_rope(g["a"], g["wqkv"], g["positions"], g["cos"], g["sin"], nq, nkv, d, bias=g["bias"]),),
                 bad_lengths=lambda g: [("bias", bs[:bs.numel() - 8]), ("cos", torch.cat([cos, cos], 1)[:, :d // 2 + 4].contiguous()),
                                        ("sin", torch.cat([sin, sin], 1)[:, :d // 2 + 4].contiguous()), ("positions", pos[:GEMM_M - 1])] if bias else [])


def make_rmsnorm(device):
    from lightretriever_amd import ops
    rng = np.random.default_rng(11)
    x, w = dev(grid(rng, (100, 256)), device).bfloat16(), dev(grid(rng, (256,)), device).bfloat16()
    return Built(lambda: [("x", x), ("w", w), ("eps", 1e-5)], method=lambda g: (ops.rmsnorm(g["x"], g["w"], 1e-5),), bad_lengths=lambda g: [("w", w[:248])])


def make_swiglu_gemm(device):
    from lightretriever_amd import ops
    rng = np.random.default_rng(12)
    a, wgu = dev(grid(rng, (GEMM_M, GEMM_K)), device).bfloat16(), dev(grid(rng, (512, GEMM_K)), device).bfloat16()
    return Built(lambda: [("a", a), ("wgu", wgu)], method=lambda g: (ops.gemm_bf16_nt(g["a"], g["wgu"], epilogue=2),),
                 bad_lengths=lambda g: [("wgu", wgu[:, :GEMM_K - 64].contiguous())])


def make_attn_varlen(device):
    from lightretriever_amd import ops
    rng = np.random.default_rng(13)
    nq, nkv, d, Tn = 4, 2, 64, sum(ENC_LENS)
    qkv = dev(grid(rng, (Tn, (nq + 2 * nkv) * d), 64), device).half()
    cu = torch.tensor(np.concatenate([[0], np.cumsum(ENC_LENS)]), dtype=torch.int32, device=device)
    return Built(lambda: [("qkv", qkv), ("cu_seqlens", cu), ("max_seqlen", max(ENC_LENS)), ("num_q_heads", nq), ("num_kv_heads", nkv), ("head_dim", d)],
                 method=lambda g: (ops.attn_varlen_causal(g["qkv"], g["cu_seqlens"], max(ENC_LENS), nq, nkv, d),),
                 bad_lengths=lambda g: [("qkv", qkv[:, :qkv.shape[1] - 64].contiguous())])


def make_encode_packed(device, shard=False, n_seqs=len(ENC_LENS)):
    """shard: `out` = rows [3, 3 + B) of a FlatIPIndex with its tiled shadow and bounds (the shadow's other rows keep their canary).  The two-layer 256-wide model of test_gpu_torch_ops.py over sequences of 70, 1 and 33 tokens; `out` is taller and wider than [B, D] and
    its rows are strided: everything outside rows [0, 3) x columns [0, 256) keeps its canary."""
    from oracle import lrx_oracle as O
    from lightretriever_amd import EncoderConfig, LrxEncoder
    cfg_o = O.EncoderConfig(vocab_size=500, hidden_size=256, num_layers=2, num_q_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=512,
                            rope_type="llama3", rope_original_max_position=64, max_positions=256)
    w = O.random_weights(cfg_o, seed=1, std=0.04)
    enc = LrxEncoder(EncoderConfig(**asdict(cfg_o)), {k: torch.from_numpy(v) for k, v in w.items()}, device=torch.device(device))
    rng = np.random.default_rng(0)
    lens = ENC_LENS[:n_seqs]
    ids = dev(rng.integers(0, 500, size=sum(lens)).astype(np.int32), device)
    cu = dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device)
    Bn, H = len(lens), 256
    if shard:
        _, smask = tile_shadow(np.zeros((Bn, H), np.float16), 1, 3)

        def shard_args():
            return [("ids", ids), ("cu_seqlens", cu), ("max_seqlen", max(lens)), ("weights", enc.handle), ("out", canary((Bn, H), torch.float32, device)),
                    ("mrl_dim", 0), ("normalize", True), ("shadow", canary(128 * H, torch.float16, device)), ("shadow_row0", 3),
                    ("row_bounds", torch.zeros(2, device=device))]

        def shard_result(ret, a):
            assert ret is None
            rows = a["shadow"].view(1, H // 64, 8, 2, 4, 16, 8).permute(0, 2, 5, 1, 3, 4, 6).reshape(128, H)[3:3 + Bn]     # (_TiledIPIndex.shadow_rows)
            return (a["out"].contiguous(), rows.contiguous())

        def shard_method(g):
            ref = enc.encode_packed(g["ids"], g["cu_seqlens"], max(lens))
            return ref, ref.to(torch.float16)
        return Built(shard_args, shard_result, method=shard_method, keep=enc,
                     written=lambda a: {"out": torch.ones(Bn, H, dtype=torch.bool), "shadow": torch.from_numpy(smask), "row_bounds": torch.ones(2, dtype=torch.bool)},
                     bad_lengths=lambda a: [("shadow", a["shadow"][:128 * H - 8]), ("row_bounds", torch.zeros(2, device=device)[:1])],
                     int_valid={"mrl_dim": 0}, int_hi={"mrl_dim": H})
    rows = Bn + 2 if Bn > 1 else 1                                         # (one sequence: a single-row `out`, wider than its D)
    mask = torch.zeros(rows, H + 64, dtype=torch.bool)
    mask[:Bn, :H] = True

    def args():
        return [("ids", ids), ("cu_seqlens", cu), ("max_seqlen", max(lens)), ("weights", enc.handle), ("out", canary((rows, H + 64), torch.float32, device)),
                ("mrl_dim", 0), ("normalize", True), ("shadow", None), ("shadow_row0", 0), ("row_bounds", None)]

    def result(ret, a):
        assert ret is None
        return (a["out"][:Bn, :H].contiguous(),)
    return Built(args, result, method=lambda g: (enc.encode_packed(g["ids"], g["cu_seqlens"], max(lens)),), written=lambda a: {"out": mask}, keep=enc,
                 bad_lengths=lambda a: [("out", a["out"][:Bn - 1]), ("out", a["out"][:, :H - 64])], int_valid={"mrl_dim": 64}, int_hi={"mrl_dim": H})


def _impact(device):
    """40 terms, 300 documents of 1 to 6 terms with weights 1 .. 9; three queries of four terms each."""
    from lightretriever_amd import ImpactIndex
    rng = np.random.default_rng(14)
    Tn = 40
    W = np.zeros((N, Tn), np.int64)
    for r in range(N):
        t = rng.permutation(Tn)[:rng.integers(1, 7)]
        W[r, t] = rng.integers(1, 10, t.size)
    C = np.zeros((Q, Tn), np.int64)
    for i in range(Q):
        t = rng.permutation(Tn)[:4]
        C[i, t] = rng.integers(1, 4, 4)
    idx = ImpactIndex(device=torch.device(device), id_base=0)
    rows, terms = np.nonzero(W)
    idx.add(terms, W[rows, terms], np.concatenate([[0], np.cumsum((W > 0).sum(1))]))
    idx.finalize()
    qr, qt = np.nonzero(C)
    q_off = np.concatenate([[0], np.cumsum((C > 0).sum(1))]).astype(np.int32)
    return idx, (C @ W.T), dev(q_off, device), dev(qt.astype(np.int32), device), dev(C[qr, qt].astype(np.int32), device)


def make_impact_topk(device):
    idx, S, off, term, cnt = _impact(device)
    Dd, I = np.full((Q, K), -FLT_MAX, np.float32), np.full((Q, K), -1, np.int64)
    row_map = np.arange(N, dtype=np.int64) * 2 + 9
    for i in range(Q):
        hit = np.flatnonzero(S[i] >= 1)
        o = hit[np.argsort(-S[i, hit], kind="stable")][:K]
        Dd[i, :o.size], I[i, :o.size] = S[i, o].astype(np.float32), row_map[o]
    rm = dev(row_map, device)
    return Built(lambda: [("postings", idx._postings), ("term_off", idx._term_off), ("n_rows", N), ("q_off", off), ("q_term", term), ("q_cnt", cnt), ("k", K),
                          ("id_base", 0), ("row_map", rm), ("window_rows", 0)], expect=(Dd, I), keep=idx, int_valid={"window_rows": 128},
                 bad_lengths=lambda a: [("row_map", rm[:N - 1]), ("q_cnt", cnt[:cnt.numel() - 1])])


def make_impact_range_search(device):
    idx, S, off, term, cnt = _impact(device)
    radius = 20.0
    lims, Dd, I = [0], [], []
    for i in range(Q):
        hit = np.flatnonzero((S[i] >= 1) & (S[i].astype(np.float32) > np.float32(radius)))
        Dd.append(S[i, hit].astype(np.float32))
        I.append(3 + hit)
        lims.append(lims[-1] + hit.size)
    return Built(lambda: [("postings", idx._postings), ("term_off", idx._term_off), ("n_rows", N), ("q_off", off), ("q_term", term), ("q_cnt", cnt),
                          ("radius", radius), ("id_base", 3), ("window_rows", 0), ("row_chunk", 0)],
                 expect=(np.asarray(lims, np.int64), np.concatenate(Dd), np.concatenate(I).astype(np.int64)), keep=idx, int_valid={"window_rows": 128},
                 bad_lengths=lambda a: [("q_cnt", cnt[:cnt.numel() - 1])])


def make_binary_topk(device, optionals=False):
    """optionals: a [D] threshold on the device and a row_map; the expectation is then the class method's (the same C entry)."""
    import binary_yardstick as BY
    from lightretriever_amd import BinaryFlatIndex
    rng = np.random.default_rng(15)
    X = grid(rng, (N, D))
    X[X == 0] = 1 / 64.0
    q = BY.grid_queries(rng, Q, D)
    idx = BinaryFlatIndex(D, device=torch.device(device))
    idx.add(dev(X, device))
    Dd, I = BY.search(q, BY.pack(X), K, BIN_K)
    qd = dev(q, device)
    nb = -(-N // 128)
    codes = idx._codes[:nb * 128 * 16]
    if optionals:
        thr = dev(grid(rng, (D,), 2), device)
        rm = torch.arange(N, device=device, dtype=torch.int64) * 2 + 1
        return Built(lambda: [("q", qd), ("codes", codes), ("n_rows", N), ("k", K), ("binary_k", BIN_K), ("rerank", True), ("threshold", thr), ("id_base", 0),
                              ("row_map", rm)], method=lambda g: idx.search(g["q"], K, binary_k=BIN_K, threshold=g["threshold"], row_map=g["row_map"]), keep=idx,
                     bad_lengths=lambda a: [("row_map", rm[:N - 1]), ("threshold", thr[:D - 1])])
    return Built(lambda: [("q", qd), ("codes", codes), ("n_rows", N), ("k", K), ("binary_k", BIN_K), ("rerank", True), ("threshold", None), ("id_base", 7),
                          ("row_map", None)], expect=(Dd, np.where(I >= 0, I + 7, -1)), keep=idx, bad_lengths=lambda a: [("codes", codes[:codes.numel() - 16])])


def _code_index(device, which):
    """The fp16, PQ or 8-bit index over 300 grid rows, trained / filled by the project's own class."""
    import lightretriever_amd as A
    X, q = _flat_data()
    xd = dev(X, device)
    if which == "sq":
        idx = A.SQFp16Index(D, device=torch.device(device), id_base=4)
    elif which == "pq":
        idx = A.PQIndex(D, M_PQ, device=torch.device(device), id_base=4)
        idx.train(xd, seed=0)
    else:
        idx = A.SQ8Index(D, "QT_8bit", device=torch.device(device), id_base=4)
        idx.train(xd)
    idx.add(xd)
    return idx, dev(q, device)


def make_sq_fp16_ip_topk(device):
    idx, qd = _code_index(device, "sq")
    rm = torch.arange(N, device=device, dtype=torch.int64) * 2 + 1

    def method(g):
        W = torch.empty(Q, K, dtype=torch.int64, device=device)
        Dd, I = idx.search(g["q"], K, wire_out=W, row_map=g["row_map"])
        return Dd, I, W
    nb = -(-N // 128)
    codes = idx._xb[:nb * 128 * D]
    return Built(lambda: [("q", qd), ("codes", codes), ("n_rows", N), ("row_bounds", idx._bounds), ("k", K), ("id_base", 4), ("row_map", rm), ("flags", 0)],
                 method=method, keep=idx, bad_lengths=lambda a: [("codes", codes[:codes.numel() - 128 * D]), ("row_bounds", torch.zeros(2, device=device)[:1]),
                                                               ("row_map", rm[:N - 1])])


def make_sq_fp16_ip_range_search(device):
    idx, qd = _code_index(device, "sq")
    nb = -(-N // 128)
    codes = idx._xb[:nb * 128 * D]
    return Built(lambda: [("q", qd), ("codes", codes), ("n_rows", N), ("row_bounds", idx._bounds), ("radius", 0.03125), ("id_base", 4)],
                 method=lambda g: idx.range_search(g["q"], 0.03125), keep=idx, canon=_range_canon,
                 bad_lengths=lambda a: [("codes", codes[:codes.numel() - 128 * D]), ("row_bounds", torch.zeros(2, device=device)[:1])])


def make_sq_fp16_ip_rerank(device):
    from lightretriever_amd import ops  # noqa: F401
    import refine_yardstick as RY
    idx, qd = _code_index(device, "sq")
    X, q = _flat_data()
    rng = np.random.default_rng(3)
    cand = np.stack([rng.permutation(N)[:20] for _ in range(Q)]).astype(np.int64)
    cd = dev(cand, device)
    row_map = np.arange(N, dtype=np.int64) * 3 + 2
    rm = dev(row_map, device)
    nb = -(-N // 128)
    codes = idx._xb[:nb * 128 * D]
    # the grid rows are exact in fp16: the decoded codes ARE the rows, so the numpy yardstick is exact here
    return Built(lambda: [("q", qd), ("codes", codes), ("n_rows", N), ("cand", cd), ("k", K), ("id_base", 50), ("row_map", rm)],
                 expect=RY.rerank(q, X, cand, K, 50, row_map), keep=idx,
                 bad_lengths=lambda a: [("codes", codes[:codes.numel() - 128 * D]), ("cand", cd[:Q - 1]), ("row_map", rm[:N - 1])])


def make_pq_ip_topk(device):
    idx, qd = _code_index(device, "pq")
    rm = torch.arange(N, device=device, dtype=torch.int64) * 2 + 1
    nb = -(-N // 128)
    codes = idx._codes[:nb * 128 * 16]
    return Built(lambda: [("q", qd), ("codes", codes), ("centroids", idx.centroids), ("n_rows", N), ("k", K), ("id_base", 4), ("row_map", rm)],
                 method=lambda g: idx.search(g["q"], K, row_map=g["row_map"]), keep=idx,
                 bad_lengths=lambda a: [("codes", codes[:codes.numel() - 16]), ("row_map", rm[:N - 1])])


def make_pq_ip_range_search(device):
    idx, qd = _code_index(device, "pq")
    nb = -(-N // 128)
    codes = idx._codes[:nb * 128 * 16]
    return Built(lambda: [("q", qd), ("codes", codes), ("centroids", idx.centroids), ("n_rows", N), ("radius", 0.03125), ("id_base", 4), ("row_chunk", 0)],
                 method=lambda g: idx.range_search(g["q"], 0.03125), keep=idx, canon=_range_canon,
                 bad_lengths=lambda a: [("codes", codes[:codes.numel() - 16])])


def make_sq8_ip_topk(device):
    idx, qd = _code_index(device, "sq8")
    rm = torch.arange(N, device=device, dtype=torch.int64) * 2 + 1
    nb = -(-N // 128)
    codes = idx._codes[:nb * 128 * D]
    return Built(lambda: [("q", qd), ("codes", codes), ("n_rows", N), ("trained", idx.trained), ("k", K), ("id_base", 4), ("row_map", rm)],
                 method=lambda g: idx.search(g["q"], K, row_map=g["row_map"]), keep=idx,
                 bad_lengths=lambda a: [("codes", codes[:codes.numel() - 128 * D]), ("row_map", rm[:N - 1]), ("trained", idx.trained[:2 * D - 4])])


def _range_canon(r):
    """(lims, D, I) with each query's segment sorted by id: the order inside a segment is the library's to choose."""
    lims, Dd, I = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in r)
    Dd, I = Dd.copy(), I.copy()
    for a, b in zip(lims[:-1], lims[1:]):
        o = np.argsort(I[a:b], kind="stable")
        Dd[a:b], I[a:b] = Dd[a:b][o], I[a:b][o]
    return lims, Dd, I


def _make_ivf(fam, kind, sel):
    def make(device):
        from ivf_store import Store
        from lightretriever_amd import RowSelector, ops
        with torch.cuda.device(torch.device(device)):
            st = Store(fam, [100, 0, 129, 71], d=D, Q=Q)              # N = 300 in four cells: one empty, one of 128 + 1 rows
            rng = np.random.default_rng(16)
            probes = np.stack([rng.permutation(NLIST)[:NPROBE] for _ in range(Q)]).astype(np.int64)
            base = st.base(probes.shape)
            scalar = K if kind == "k" else (st.median(probes, base) if fam != "pq" else 0.0)
            a = list(st._op_args(probes, base, scalar, None, None, 9, None))
        if kind == "k":                                                 # _op_args orders (radius, max_scan, ...): the same slots hold (k, max_scan, ...)
            a[-4] = K
        names = [n for n in ANN[ivf_op_name(fam, kind, False)]]
        args = list(zip(names, a))
        if sel:
            mask = np.random.default_rng(17).random(N) < 0.5
            words = RowSelector.from_mask(torch.from_numpy(mask), device=torch.device(device)).words
            at = names.index("by_residual") if fam != "flat" else names.index(kind)
            args.insert(at, ("sel", words))
        name = ivf_op_name(fam, kind, sel)
        bad = lambda g: [("row_ids", g["row_ids"][:N - 1]) if fam != "pq" else ("codes", g["codes"][:g["codes"].numel() - 16]), ("list_off", g["list_off"][:1])] + ([("sel", g["sel"][:g["sel"].numel() - 1]),
                                                                                                 ("sel", torch.cat([g["sel"], g["sel"]])[:g["sel"].numel() + 1])] if sel else []) + \
            ([("trained", g["trained"][:2 * D - 4])] if fam == "sq8" else [])
        return Built(lambda: args, method=lambda g: getattr(ops, name)(*g.values()), canon=_range_canon if kind == "radius" else (lambda r: r), keep=st, bad_lengths=bad)
    return make


MAKE = {name[len("make_"):]: fn for name, fn in list(globals().items()) if name.startswith("make_")}
for _fam in IVF_FAMILIES:
    for _kind in ("k", "radius"):
        for _sel in (False, True):
            MAKE[ivf_op_name(_fam, _kind, _sel)] = _make_ivf(_fam, _kind, _sel)

# the ops whose expectation is computed on the CPU in fp64, bit for bit
EXACT = ("flat_ip_topk", "flat_ip_topk_bounded", "flat_ip_topk_bounded_wire", "flat_ip_range_search", "flat_ip_rerank", "merge_topk", "merge_topk_packed",
         "shard_commit_rows", "linear_transform", "binary_topk", "sparse_compact_csr", "impact_topk", "impact_range_search", "embedding_bag_mean")
# builders with the optional tensors that the first form leaves out (None there): op -> keywords
ALT = {"rope_qkv_gemm": {"bias": False}, "binary_topk": {"optionals": True}, "encode_packed": {"shard": True}}
# every search op: its no-query and no-row forms are derived from the valid call (no_query / no_row below)
SEARCH_OPS = tuple(sorted(op for op in ANN if ("topk" in op or "range_search" in op or "rerank" in op) and not op.startswith("merge")))


def _cut(a, names, n=0):
    for name in names:
        if isinstance(a.get(name), torch.Tensor):
            a[name] = a[name][:n].contiguous()


def no_query(op, a, n=0):
    """The valid call's arguments with its first n queries (0: none): q / cand / probes / probe_scores cut, the impact CSR cut."""
    a = OrderedDict(a)
    _cut(a, ("q", "cand", "probes", "probe_scores"), n)
    if "q_off" in a:
        end = int(a["q_off"][n])
        a["q_off"] = a["q_off"][:n + 1].contiguous()
        _cut(a, ("q_term", "q_cnt"), end)
    return a


def no_row(op, a):
    """The valid call's arguments over an empty store: no rows, no codes, no postings, every cell empty, candidates all -1."""
    a = OrderedDict(a)
    _cut(a, ("x", "x_shadow", "row_map", "row_ids", "sel", "postings"))
    if "codes" in a:
        a["codes"] = a["codes"][:0].contiguous()
    if "n_rows" in a:
        a["n_rows"] = 0
    for name in ("list_off", "term_off"):
        if name in a:
            a[name] = torch.zeros_like(a[name])
    if "cand" in a:
        a["cand"] = torch.full_like(a["cand"], -1)
    return a


def empty_result(op, a):
    """What every index class returns for no query or no row: [Q, k] of (-FLT_MAX, -1) (and their wire words), or lims of zeros and no hit."""
    Qn = a["q"].shape[0] if "q" in a else a["q_off"].numel() - 1
    if "radius" in a:
        return np.zeros(Qn + 1, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64)
    Dd, I = np.full((Qn, a["k"]), -FLT_MAX, np.float32), np.full((Qn, a["k"]), -1, np.int64)
    return (Dd, I, pack_words(Dd, I)) if op in ("flat_ip_topk_bounded_wire", "sq_fp16_ip_topk") else (Dd, I)


def single_row(op, a, name):
    """The valid call's arguments with the rows-may-stride operand `name` left one row (contiguous): one query, one row of reps, one sequence's
    `out` comes from its builder, or a one-row store (ivf_flat: the row is original row 0 and sits in the first non-empty cell)."""
    if name in ("cand", "probes", "probe_scores"):
        return no_query(op, a, 1)
    a = OrderedDict(a)
    if name == "reps":
        _cut(a, ("reps",), 1)
    elif name == "x" and op.startswith("ivf_flat"):
        _cut(a, ("x", "row_ids", "sel", "row_map"), 1)
        a["row_ids"] = torch.zeros_like(a["row_ids"])
        off = torch.ones_like(a["list_off"])
        off[0] = 0
        a["list_off"] = off                                                 # cell 0 holds the row, every other cell is empty
    elif name == "x" and op == "flat_ip_rerank":
        _cut(a, ("x", "row_map"), 1)
        a["cand"] = torch.where(a["cand"] >= 0, torch.zeros_like(a["cand"]), a["cand"])     # every candidate names the one row (or is skipped)
    else:
        raise KeyError((op, name))
    return a


# the single-row forms derived from the valid call (item 3): op -> the operands
SINGLE_ROW_DERIVED = {op: tuple(n for n, ann in ANN[op].items() if ann["kind"] == "tensor" and ann["rows_may_stride"] and
                                (n in ("cand", "probes", "probe_scores", "reps") or (n == "x" and (op.startswith("ivf_flat") or op == "flat_ip_rerank")))) for op in ANN}
SINGLE_ROW_DERIVED = {op: v for op, v in SINGLE_ROW_DERIVED.items() if v}

# the search ops and the empty forms their builders take (item 7): no query, no row -- these have an fp64 expectation of their own
EMPTY = {"flat_ip_topk": ({"nq": 0}, {"n": 0}), "flat_ip_topk_bounded": ({"nq": 0}, {"n": 0}), "flat_ip_topk_bounded_wire": ({"nq": 0}, {"n": 0}),
         "flat_ip_range_search": ({"nq": 0}, {"n": 0}), "flat_ip_rerank": ({"nq": 0},), "linear_transform": ({"n": 0},)}
# single-row forms (item 3): the builder's keyword that leaves the rows-may-stride operand one row
SINGLE_ROW = {"flat_ip_topk": ("x", {"n": 1}), "flat_ip_topk_bounded": ("x", {"n": 1}), "flat_ip_range_search": ("x", {"n": 1}), "linear_transform": ("x", {"n": 1}),
              "flat_ip_rerank": ("cand", {"nq": 1}), "shard_commit_rows": ("x", {"n": 1, "row0": 40}), "flat_ip_topk_bounded_wire": ("x", {"n": 1}),
              "encode_packed": ("out", {"n_seqs": 1})}
# operands that share one leading dimension in the C ABI (ld_probe): a strided form is given to both
SAME_STRIDE = {"probes": "probe_scores", "probe_scores": "probes"}
