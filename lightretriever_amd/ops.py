"""Thin torch-tensor wrappers over the individual liblrx kernels (unit tests, query side, EmbeddingBag construction)."""
from __future__ import annotations

import collections
from typing import Optional

import torch

from . import _lib
from .index import _range_call, _range_empty, _workspace


def _s():
    return _lib.current_stream()


def embedding_gather(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    out = torch.empty(ids.numel(), table.shape[1], dtype=torch.bfloat16, device=table.device)
    _lib.check(_lib.lib().lrx_embedding_gather(_lib.ptr(table), _lib.ptr(ids), ids.numel(), table.shape[1], table.shape[0], _lib.ptr(out), _s()))
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    y = torch.empty_like(x)
    _lib.check(_lib.lib().lrx_rmsnorm(_lib.ptr(x), _lib.ptr(w), _lib.ptr(y), x.shape[0], x.shape[1], eps, _s()))
    return y


def gemm_bf16_nt(A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                 epilogue: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K and A.is_contiguous() and B.is_contiguous()
    if out is None:
        out = torch.empty(M, N // 2 if epilogue == 2 else N, dtype=torch.bfloat16, device=A.device)
    _lib.check(_lib.lib().lrx_gemm_bf16_nt(_lib.ptr(A), _lib.ptr(B), _lib.ptr(out), _lib.ptr(bias), _lib.ptr(resid), M, N, K, epilogue, _s()))
    return out


def _operand_flag(operands: str, what: str, *tensors) -> int:
    """"bf16" -> 0, "fp16" -> 1 (the f16 flag of the lrx_*_ex entry points); the 16-bit operands must hold that format"""
    if operands not in ("bf16", "fp16"):
        raise ValueError(f"{what}: operands must be 'bf16' or 'fp16', not {operands!r}")
    want = torch.float16 if operands == "fp16" else torch.bfloat16
    for t in tensors:
        if t.dtype != want:
            raise TypeError(f"{what}: operands={operands!r} takes {want} matrices, got {t.dtype}")
    return int(operands == "fp16")


def _a16_flag(a16_dtype, what: str) -> int:
    if a16_dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{what}: the 16-bit output is torch.bfloat16 or torch.float16, not {a16_dtype}")
    return int(a16_dtype == torch.float16)


def gemm_bf16_nt_fused(A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, epilogue: int = 0,
                       rscale: Optional[torch.Tensor] = None, want_ss: bool = False, operands: str = "bf16", out: Optional[torch.Tensor] = None):
    """lrx_gemm_bf16_nt_fused: -> (out bf16, ss_part fp32 [ceil(N/256), M] or None).  operands="fp16" (lrx_gemm_nt_fused_ex, SwiGLU epilogue
    only): A and B hold fp16 and `out` is fp16, saturating.  out: a contiguous tensor of the result's shape and dtype to write into."""
    f16 = _operand_flag(operands, "gemm_bf16_nt_fused", A, B)
    M, K = A.shape
    N = B.shape[0]
    shape, dtype = (M, N // 2 if epilogue == 2 else N), (torch.float16 if f16 else torch.bfloat16)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=A.device)
    elif out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"gemm_bf16_nt_fused: out must be contiguous {dtype} {list(shape)}")
    ss = torch.full(((N + 255) // 256, M), float("nan"), dtype=torch.float32, device=A.device) if want_ss else None
    _lib.check(_lib.lib().lrx_gemm_nt_fused_ex(_lib.ptr(A), _lib.ptr(B), _lib.ptr(out), _lib.ptr(bias), _lib.ptr(resid), M, N, K, epilogue,
                                               _lib.ptr(rscale), _lib.ptr(ss), f16, _s()))
    return out, ss


def row_rscale(x: torch.Tensor, eps: float) -> torch.Tensor:
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().lrx_row_rscale(_lib.ptr(x), x.shape[0], x.shape[1], float(eps), _lib.ptr(out), _s()))
    return out


def finalize_rscale(ss_part: torch.Tensor, hidden_size: int, eps: float) -> torch.Tensor:
    out = torch.empty(ss_part.shape[1], dtype=torch.float32, device=ss_part.device)
    _lib.check(_lib.lib().lrx_finalize_rscale(_lib.ptr(ss_part), ss_part.shape[0], ss_part.shape[1], hidden_size, float(eps), _lib.ptr(out), _s()))
    return out


def rotary_pair_order(nq: int, nkv: int, d: int) -> torch.Tensor:
    """Row permutation of the fused qkv projection (include/lrx.h, lrx_layer_weights.wqkv): physical row 32 g + 16 i + t of every q and k head
    = logical row i * d/2 + 16 g + t; v rows stay in place.  `W_physical = W_logical[perm]`; the same index applies to the bias and, read
    the other way (`x_logical[..., perm] = x_physical`), to the q | k columns the fused kernel writes."""
    t = torch.arange(d)
    g, i, r = t // 32, (t % 32) // 16, t % 16
    head = i * (d // 2) + 16 * g + r
    rot = torch.cat([h * d + head for h in range(nq + nkv)])
    return torch.cat([rot, torch.arange((nq + nkv) * d, (nq + 2 * nkv) * d)])


def gemm_qkv_rope(A: torch.Tensor, Wqkv: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, nq: int, nkv: int,
                  d: int, bias: Optional[torch.Tensor] = None, rscale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Wqkv / bias rows in rotary-pair order (rotary_pair_order); -> fp16 [M, (nq+2nkv)d], q | k columns in the same order."""
    M, K = A.shape
    out = torch.empty(M, (nq + 2 * nkv) * d, dtype=torch.float16, device=A.device)
    _lib.check(_lib.lib().lrx_gemm_qkv_rope_fused(_lib.ptr(A), _lib.ptr(Wqkv), _lib.ptr(out), _lib.ptr(bias), _lib.ptr(positions), _lib.ptr(cos),
                                                  _lib.ptr(sin), M, K, nq, nkv, d, _lib.ptr(rscale), _s()))
    return out


def gemm_qkv_rope_slice(A: torch.Tensor, Wqkv: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, nq: int, nkv: int,
                        d: int, head0: int, n_heads: int, out: torch.Tensor, bias: Optional[torch.Tensor] = None,
                        rscale: Optional[torch.Tensor] = None, operands: str = "bf16") -> torch.Tensor:
    """lrx_gemm_qkv_rope_slice: heads [head0, head0 + n_heads) of the projection (Wqkv / bias are the FULL matrices) into their columns of
    `out`, fp16 [M, (nq+2nkv)d]; every other column of `out` is left alone.  operands="fp16" (lrx_gemm_qkv_rope_slice_ex): A and Wqkv hold
    fp16; the bias stays bf16."""
    f16 = _operand_flag(operands, "gemm_qkv_rope_slice", A, Wqkv)
    M, K = A.shape
    if out.dtype != torch.float16 or out.shape != (M, (nq + 2 * nkv) * d) or not out.is_contiguous():
        raise ValueError("gemm_qkv_rope_slice: out must be contiguous fp16 [M, (nq+2nkv)d]")
    _lib.check(_lib.lib().lrx_gemm_qkv_rope_slice_ex(_lib.ptr(A), _lib.ptr(Wqkv), _lib.ptr(out), _lib.ptr(bias), _lib.ptr(positions), _lib.ptr(cos),
                                                     _lib.ptr(sin), M, K, nq, nkv, d, _lib.ptr(rscale), head0, n_heads, f16, _s()))
    return out


def gemm_resid32(A: torch.Tensor, B: torch.Tensor, x32: torch.Tensor, gamma: Optional[torch.Tensor] = None, want_a16: bool = True, want_ss: bool = False,
                 operands: str = "bf16", a16_dtype=torch.bfloat16):
    """lrx_gemm_bf16_nt_resid32: x32 (fp32 [M,N], in place) += A . B^T -> (a16 bf16 [M,N] = bf16(x32 * gamma) or None, ss_part or None).
    operands="fp16" / a16_dtype=torch.float16 (lrx_gemm_nt_resid32_ex): A and B hold fp16 / a16 = fp16(x32 * gamma), saturating; fp16
    operands with a bf16 a16 are refused."""
    f16, out_f16 = _operand_flag(operands, "gemm_resid32", A, B), _a16_flag(a16_dtype, "gemm_resid32")
    M, K = A.shape
    N = B.shape[0]
    a16 = torch.empty(M, N, dtype=a16_dtype, device=A.device) if want_a16 else None
    ss = torch.full(((N + 255) // 256, M), float("nan"), dtype=torch.float32, device=A.device) if want_ss else None
    _lib.check(_lib.lib().lrx_gemm_nt_resid32_ex(_lib.ptr(A), _lib.ptr(B), _lib.ptr(x32), _lib.ptr(a16), _lib.ptr(gamma), M, N, K, _lib.ptr(ss), f16, out_f16,
                                                 _s()))
    return a16, ss


def embed_stream32(table: torch.Tensor, ids: torch.Tensor, gamma: torch.Tensor, eps: float, a16_dtype=torch.bfloat16):
    """lrx_embed_stream32 -> (x32 fp32 [T,H], a16 bf16 [T,H], rscale fp32 [T]).  a16_dtype=torch.float16 (lrx_embed_stream32_ex): a16 =
    fp16(x32 * gamma), saturating."""
    f16 = _a16_flag(a16_dtype, "embed_stream32")
    T, H = ids.numel(), table.shape[1]
    x32 = torch.empty(T, H, dtype=torch.float32, device=table.device)
    a16 = torch.empty(T, H, dtype=a16_dtype, device=table.device)
    rs = torch.empty(T, dtype=torch.float32, device=table.device)
    _lib.check(_lib.lib().lrx_embed_stream32_ex(_lib.ptr(table), _lib.ptr(ids), T, H, table.shape[0], _lib.ptr(gamma), _lib.ptr(x32), _lib.ptr(a16), _lib.ptr(rs),
                                                float(eps), f16, _s()))
    return x32, a16, rs


def rmsnorm_f32(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().lrx_rmsnorm_f32(_lib.ptr(x), _lib.ptr(w), _lib.ptr(y), x.shape[0], x.shape[1], float(eps), _s()))
    return y


def build_positions(cu_seqlens: torch.Tensor, total_tokens: int) -> torch.Tensor:
    pos = torch.empty(total_tokens, dtype=torch.int32, device=cu_seqlens.device)
    _lib.check(_lib.lib().lrx_build_positions(_lib.ptr(cu_seqlens), cu_seqlens.numel() - 1, total_tokens, _lib.ptr(pos), _s()))
    return pos


def attn_work_list(cu_seqlens: torch.Tensor, total_tokens: int, max_seqlen: int, nq: int, nkv: int, d: int, last_tile_only: bool = False) -> torch.Tensor:
    """The work list of `attn_varlen_causal` for this batch layout (include/lrx.h, ABI 7): build once, pass to every layer's call."""
    L = _lib.lib()
    n_seqs = cu_seqlens.numel() - 1
    nbytes = L.lrx_attn_items_bytes(n_seqs, total_tokens, max_seqlen, nq, nkv, d, int(last_tile_only))
    items = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=cu_seqlens.device)
    _lib.check(L.lrx_attn_build_items(_lib.ptr(cu_seqlens), n_seqs, total_tokens, max_seqlen, nq, nkv, d, int(last_tile_only), _lib.ptr(items),
                                      items.numel(), _s()))
    return items


def attn_varlen_causal(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int, nq: int, nkv: int, d: int,
                       last_tile_only: bool = False, work_list=None, out_dtype=torch.bfloat16) -> torch.Tensor:
    """work_list: None -> built here (one extra small launch); a tensor from `attn_work_list` with the SAME layout arguments; False -> the
    launch without a list (`lrx_attn_varlen_causal`: the same kernel walks its items itself; same bits, ~5 % longer on the tiled path).
    out_dtype=torch.float16 (lrx_attn_varlen_causal_ex): the output rows are written as fp16."""
    if qkv.dtype != torch.float16:
        raise TypeError("attn_varlen_causal: qkv must be fp16 (the fused QKV + RoPE projection writes fp16)")
    out_f16 = _a16_flag(out_dtype, "attn_varlen_causal")
    T = qkv.shape[0]
    out = (torch.zeros if last_tile_only else torch.empty)(T, nq * d, dtype=out_dtype, device=qkv.device)
    n_seqs = cu_seqlens.numel() - 1
    if work_list is False:
        _lib.check(_lib.lib().lrx_attn_varlen_causal_ex(_lib.ptr(qkv), _lib.ptr(cu_seqlens), None, 0, n_seqs, T, max_seqlen, nq, nkv, d,
                                                        _lib.ptr(out), int(last_tile_only), out_f16, _s()))
        return out
    if T == 0 or n_seqs == 0:
        return out
    if work_list is None:
        work_list = attn_work_list(cu_seqlens, T, max_seqlen, nq, nkv, d, last_tile_only)
    _lib.check(_lib.lib().lrx_attn_varlen_causal_ex(_lib.ptr(qkv), _lib.ptr(cu_seqlens), _lib.ptr(work_list), work_list.numel(), n_seqs, T, max_seqlen,
                                                    nq, nkv, d, _lib.ptr(out), int(last_tile_only), out_f16, _s()))
    return out


def attn_prefix_suffix(qkv: torch.Tensor, prefix_kv: torch.Tensor, n_seqs: int, suffix_len: int, nq: int, nkv: int, d: int,
                       out_dtype=torch.bfloat16) -> torch.Tensor:
    """qkv [n_seqs*suffix_len, (nq+2nkv)d] fp16, prefix_kv [P1, 2*nkv*d] fp16 (k | v) -> [n_seqs*suffix_len, nq*d] bf16, or fp16 with
    out_dtype=torch.float16 (lrx_attn_prefix_suffix_ex)."""
    out_f16 = _a16_flag(out_dtype, "attn_prefix_suffix")
    if qkv.dtype != torch.float16 or prefix_kv.dtype != torch.float16:
        raise TypeError("attn_prefix_suffix: qkv and prefix_kv must be fp16")
    if qkv.shape != (n_seqs * suffix_len, (nq + 2 * nkv) * d) or prefix_kv.shape[1:] != (2 * nkv * d,):
        raise ValueError("attn_prefix_suffix: operand shapes do not match the head layout")
    out = torch.empty(n_seqs * suffix_len, nq * d, dtype=out_dtype, device=qkv.device)
    _lib.check(_lib.lib().lrx_attn_prefix_suffix_ex(_lib.ptr(qkv), _lib.ptr(prefix_kv) if prefix_kv.shape[0] else None, n_seqs, suffix_len,
                                                    prefix_kv.shape[0], nq, nkv, d, _lib.ptr(out), out_f16, _s()))
    return out


def uniform_layout(n_seqs: int, length: int, position_offset: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    cu = torch.empty(n_seqs + 1, dtype=torch.int32, device=device)
    pos = torch.empty(n_seqs * length, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().lrx_uniform_layout(_lib.ptr(cu), _lib.ptr(pos), n_seqs, length, position_offset, _s()))
    return cu, pos


def gather_last_rows(src: torch.Tensor, cu_seqlens: torch.Tensor) -> torch.Tensor:
    B = cu_seqlens.numel() - 1
    dst = torch.empty(B, src.shape[1], dtype=torch.bfloat16, device=src.device)
    _lib.check(_lib.lib().lrx_gather_last_rows(_lib.ptr(src), _lib.ptr(cu_seqlens), B, src.shape[1], _lib.ptr(dst), _s()))
    return dst


def pool_norm(hidden: torch.Tensor, w: torch.Tensor, cu_seqlens: torch.Tensor, eps: float, out_dim: Optional[int] = None,
              normalize: bool = True, pooling: str = "lasttoken") -> torch.Tensor:
    """hidden bf16 [T,H] (HF's bf16 norm arithmetic) or fp32 [T,H] (the precise stream: fp32 norm); pooling: finetune/dense_pooling.py:12-82
    ('lasttoken', 'cls', 'mean', 'second_to_last', 'third_to_last')."""
    B, H = cu_seqlens.numel() - 1, hidden.shape[1]
    D = out_dim or H
    out = torch.empty(B, D, dtype=torch.float32, device=hidden.device)
    _lib.check(_lib.lib().lrx_pool_norm_mode(_lib.ptr(hidden), _lib.ptr(w), _lib.ptr(cu_seqlens), B, H, eps, _lib.POOLING[pooling], _lib.ptr(out), D, D,
                                             int(normalize), None, 0, None, int(hidden.dtype == torch.float32), _s()))
    return out


def embedding_bag_mean(table: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, padding_idx: Optional[int] = None,
                       out_dim: Optional[int] = None, normalize: bool = False) -> torch.Tensor:
    """table fp32 [V,H] (device), ids/offsets int64 (device) -> fp32 [n_bags, out_dim]."""
    V, H = table.shape
    D = out_dim or H
    nb = offsets.numel()
    out = torch.empty(nb, D, dtype=torch.float32, device=table.device)
    _lib.check(_lib.lib().lrx_embedding_bag_mean(_lib.ptr(table), V, H, _lib.ptr(ids), ids.numel(), _lib.ptr(offsets), nb,
                                                 -1 if padding_idx is None else int(padding_idx), _lib.ptr(out), D, D, int(normalize), _s()))
    return out


def flat_ip_scores(X: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    lib = _lib.lib()
    N, D = X.shape
    ld = int(lib.lrx_flat_ip_score_ld(N))
    s = torch.empty(q.shape[0], ld, dtype=torch.float32, device=X.device)
    _lib.check(lib.lrx_flat_ip_scores(_lib.ptr(X), N, X.stride(0), D, _lib.ptr(q), q.shape[0], _lib.ptr(s), _s()))
    return s


# -- sparse document vectors (N2) ------------------------------------------------------------------------------------------
def sparse_max_aggregate(hidden: torch.Tensor, lm_head: torch.Tensor, cu_seqlens: torch.Tensor, tok_mask: Optional[torch.Tensor] = None,
                         bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hidden bf16 [T,H], lm_head bf16 [V,H], tok_mask uint8 [T] (None = drop first/last token) -> fp32 [B,V] running maxima
    (out: fp32 [B, >= V] with unit inner stride to write them into; its columns from V on are left alone)."""
    T, H = hidden.shape
    V, B = lm_head.shape[0], cu_seqlens.numel() - 1
    if lm_head.shape[1] != H or hidden.dtype != torch.bfloat16 or lm_head.dtype != torch.bfloat16:
        raise ValueError("sparse_max_aggregate: hidden [T,H] / lm_head [V,H] must be bf16 with matching H")
    if tok_mask is not None and (tok_mask.dtype != torch.uint8 or tok_mask.numel() != T):
        raise ValueError("sparse_max_aggregate: tok_mask must be uint8 [T]")
    if out is None:
        out = torch.empty(B, V, dtype=torch.float32, device=hidden.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < V or out.stride(1) != 1:
        raise ValueError("sparse_max_aggregate: out must be fp32 [B, >= V] with unit inner stride")
    seg = torch.empty(T, dtype=torch.int32, device=hidden.device)
    _lib.check(_lib.lib().lrx_sparse_max_aggregate(_lib.ptr(hidden), _lib.ptr(lm_head), _lib.ptr(bias) if bias is not None else None,
                                                   _lib.ptr(cu_seqlens), _lib.ptr(tok_mask) if tok_mask is not None else None, B, T, H, V,
                                                   _lib.ptr(out), out.stride(0), _lib.ptr(seg), _s()))
    return out


def sparsify_(reps: torch.Tensor, relu: bool = True, log1p: bool = True, round_bf16: bool = True, top_k: int = 0, min_tokens_to_keep: int = 8) -> torch.Tensor:
    if reps.dtype != torch.float32 or reps.dim() != 2 or reps.stride(1) != 1:
        raise ValueError("sparsify_: fp32 [B,V] with unit inner stride")
    _lib.check(_lib.lib().lrx_sparsify(_lib.ptr(reps), reps.shape[0], reps.shape[1], reps.stride(0), int(relu), int(log1p), int(round_bf16),
                                       int(top_k), int(min_tokens_to_keep), _s()))
    return reps


def sparse_compact(reps: torch.Tensor, quantization_factor: int = 100, capacity: Optional[int] = None):
    """-> (ids int32 [B,cap], weights int32 [B,cap], counts int32 [B]); ascending token ids, weights = rint(max(x,0)*q) != 0."""
    B, V = reps.shape
    cap = int(capacity or V)
    ids = torch.empty(B, cap, dtype=torch.int32, device=reps.device)
    w = torch.empty(B, cap, dtype=torch.int32, device=reps.device)
    cnt = torch.empty(B, dtype=torch.int32, device=reps.device)
    _lib.check(_lib.lib().lrx_sparse_compact(_lib.ptr(reps), B, V, reps.stride(0), int(quantization_factor), cap, _lib.ptr(ids), _lib.ptr(w),
                                             _lib.ptr(cnt), _s()))
    return ids, w, cnt


def sparse_compact_csr(reps: torch.Tensor, quantization_factor: int = 100, empty_marker: bool = True):
    """Quantise + compact fp32 [B, V] (unit inner stride) to ragged CSR -> SparseRows: per row the (token id, rint(max(x, 0) * q)) pairs
    with a non-zero weight in ascending id order; a row without any holds the marker pair (V, 1) when empty_marker.  Two launches
    (lrx_sparse_csr_count / lrx_sparse_csr_fill) around a device cumsum; the total length is read back to the host once, so the call
    is refused under graph capture."""
    from .sparse_rows import SparseRows
    if reps.dtype != torch.float32 or reps.dim() != 2 or reps.stride(1) != 1 or not reps.is_cuda:
        raise ValueError("sparse_compact_csr: fp32 device [B, V] with unit inner stride")
    if torch.cuda.is_current_stream_capturing():
        raise _lib.LrxError("sparse_compact_csr under graph capture: the result length is read back to the host")
    B, V = reps.shape
    lib, q, mark = _lib.lib(), int(quantization_factor), int(bool(empty_marker))
    ld = reps.stride(0) if B else V
    counts = torch.empty(B, dtype=torch.int32, device=reps.device)
    _lib.check(lib.lrx_sparse_csr_count(_lib.ptr(reps), B, V, ld, q, mark, _lib.ptr(counts), _s()))
    row_off = torch.zeros(B + 1, dtype=torch.int64, device=reps.device)
    torch.cumsum(counts, 0, dtype=torch.int64, out=row_off[1:])
    nnz = int(row_off[-1])
    terms = torch.empty(nnz, dtype=torch.int32, device=reps.device)
    weights = torch.empty(nnz, dtype=torch.int32, device=reps.device)
    _lib.check(lib.lrx_sparse_csr_fill(_lib.ptr(reps), B, V, ld, q, mark, _lib.ptr(row_off), _lib.ptr(terms), _lib.ptr(weights), _s()))
    return SparseRows(row_off, terms, weights, V)


# -- graph index (fixed-degree neighbour graph + beam search) --------------------------------------------------------------------
def graph_ip_topk(q: torch.Tensor, X: torch.Tensor, graph: torch.Tensor, entry_rows: torch.Tensor, k: int, beam: int, width: int = 4,
                  max_iterations: int = 0, id_base: int = 0, row_map: Optional[torch.Tensor] = None, stats: bool = False,
                  ws_slots: Optional[dict] = None, capture_error: Optional[str] = None):
    """lrx_graph_ip_search -> (D f32[Q,k], I i64[Q,k]) or, with stats=True, (D, I, S i32[Q,2] = steps taken, rows scored): the beam search of
    include/lrx.h over the fp32 rows X [n, d] and the neighbour table graph int32 [n, degree] (contiguous, -1 = no edge), started from
    entry_rows int64 [Q, n_entry] (rows may be strided; < 0 skipped, >= n skipped and counted in lrx_device_error_count).  q fp32 [Q, d]
    contiguous.  ws_slots: a dict that keeps the workspace between calls (key "_ws")."""
    lib = _lib.lib()
    n, d = X.shape
    if graph.dtype != torch.int32 or graph.dim() != 2 or graph.shape[0] != n or not graph.is_contiguous():
        raise ValueError(f"graph_ip_topk: graph must be int32 [{n}, degree] contiguous")
    if entry_rows.dtype != torch.int64 or entry_rows.dim() != 2 or entry_rows.shape[0] != q.shape[0] or (entry_rows.shape[1] and entry_rows.stride(1) != 1):
        raise ValueError("graph_ip_topk: entry_rows must be int64 [Q, n_entry] with unit inner stride")
    Q, n_entry = entry_rows.shape
    degree = graph.shape[1]
    D = torch.empty(Q, k, dtype=torch.float32, device=q.device)
    I = torch.empty(Q, k, dtype=torch.int64, device=q.device)
    S = torch.empty(Q, 2, dtype=torch.int32, device=q.device) if stats else None
    need = int(lib.lrx_graph_ip_workspace_bytes(Q, n_entry, degree, beam, width))
    ws = _workspace({} if ws_slots is None else ws_slots, "_ws", need, q.device, capture_error) if Q else None
    _lib.check(lib.lrx_graph_ip_search(_lib.ptr(X) if n else None, n, X.stride(0) if n > 1 else d, d, _lib.ptr(graph) if n else None, degree,
                                       _lib.ptr(q) if Q else None, Q, _lib.ptr(entry_rows) if Q else None, n_entry,
                                       entry_rows.stride(0) if Q > 1 else n_entry, k, beam, width, max_iterations, int(id_base), _lib.ptr(D), _lib.ptr(I),
                                       _lib.ptr(row_map), _lib.ptr(S), _lib.ptr(ws), ws.numel() if Q else 0, _s()))
    return (D, I, S) if stats else (D, I)


def graph_detour_counts(knn: torch.Tensor) -> torch.Tensor:
    """lrx_graph_detour_counts -> counts int32 [n, K]: knn int32 [n, K] contiguous, the kNN lists of the graph build (-1 = empty slot);
    counts[u][c] = the two-hop paths u -> knn[u][a] -> knn[u][c] through list positions a, b < c (include/lrx.h)."""
    if knn.dtype != torch.int32 or knn.dim() != 2 or not knn.is_contiguous():
        raise ValueError("graph_detour_counts: knn must be int32 [n, K] contiguous")
    n, K = knn.shape
    counts = torch.empty(n, K, dtype=torch.int32, device=knn.device)
    _lib.check(_lib.lib().lrx_graph_detour_counts(_lib.ptr(knn) if n else None, n, K, _lib.ptr(counts) if n else None, _s()))
    return counts


# -- inverted file (IndexIVFFlat) ---------------------------------------------------------------------------------------------
# Every family is described ONCE, by an _IvfFamily: `fam`, the stem of its library names; `args`, its _ivf_*_args, which checks a wrapper's
# operands (its `n_operands` positionals before the k or radius) -> (Q, dims, head), the leading arguments of its two workspace functions (up to
# nprobe) and of its four library entries (up to ld_probe / by_residual); `sel_at`, where a *_sel wrapper takes its selector among them.
# _ivf_topk and _ivf_range are the bodies of all sixteen wrappers and add the rest, the same for all four families:
# lrx_<fam>_workspace_bytes(*dims, k, max_scan_rows) and lrx_<fam>_search(*head, max_scan_rows, k, id_base, D, I, row_map, ws, bytes, stream),
# or lrx_<fam>_range_workspace_bytes(*dims, max_scan_rows) and lrx_<fam>_range_search(*head, max_scan_rows, radius, id_base, lims, D, I,
# capacity, row_map, ws, bytes, stream).  The plain wrappers are written out: their signatures and docstrings document the operands.
# _ivf_sel_wrapper makes the *_sel sibling of each (a search under a row selector, selector.RowSelector): `sel` is None in a plain wrapper's
# body and (words or None,) in a *_sel one's, which calls lrx_<fam>_search_sel / _range_search_sel -- (sel words, n) in front of ws -- even
# without words.
_IvfFamily = collections.namedtuple("_IvfFamily", "fam args n_operands sel_at")


def _ivf_sel(name: str, words, n: int):
    """The (sel words, n) arguments of a *_sel entry: the words int32 [ceil(n / 32)] contiguous on the device, or None (no filter)."""
    if words is not None and (words.dtype != torch.int32 or not words.is_cuda or not words.is_contiguous() or words.dim() != 1 or
                              words.numel() != (n + 31) // 32):
        raise ValueError(f"{name}: sel must be the int32 words of a selector over the {n} rows of the index: [{(n + 31) // 32}] contiguous")
    return (_lib.ptr(words), n)


def _ivf_probes(name: str, q, probes):
    Q, nprobe = probes.shape
    if probes.dtype != torch.int64 or (nprobe and probes.stride(1) != 1) or q.shape[0] != Q:
        raise ValueError(f"{name}: probes must be int64 [Q, nprobe] with unit inner stride")
    return Q, nprobe, probes.stride(0) if Q > 1 else nprobe


def _ivf_probe_args(name: str, q, Q, probes, probe_scores, nprobe, ld, by_residual):
    """The query and probe arguments of the three entries over residual codes (the check of probe_scores included)."""
    ok = probe_scores is not None and probe_scores.dtype == torch.float32 and probe_scores.shape == probes.shape and \
        not (nprobe and probe_scores.stride(1) != 1) and not (Q > 1 and probe_scores.stride(0) != ld)
    if by_residual and not ok:
        raise ValueError(f"{name}: by_residual needs probe_scores fp32 [Q, nprobe] with the row stride of probes")
    return (_lib.ptr(q), Q, _lib.ptr(probes), _lib.ptr(probe_scores) if by_residual else None, nprobe, ld, int(bool(by_residual)))


def _ivf_topk(F: _IvfFamily, name: str, sel, operands, k: int, max_scan_rows: int, id_base: int = 0, row_map=None, ws_slots: Optional[dict] = None,
              capture_error: Optional[str] = None):
    """The wrapper `name` of family F over its `operands` (q first): the checks, the outputs, the workspace (ws_slots: a dict that keeps it
    between calls, key "_ws") and the call."""
    lib, fam, q = _lib.lib(), F.fam, operands[0]
    Q, dims, head = F.args(name, *operands)
    sel_args, sfx = ((), "") if sel is None else (_ivf_sel(name, sel[0], dims[0]), "_sel")
    D = torch.empty(Q, k, dtype=torch.float32, device=q.device)
    I = torch.empty(Q, k, dtype=torch.int64, device=q.device)
    if Q == 0:
        return D, I
    need = int(getattr(lib, f"lrx_{fam}_workspace_bytes")(*dims, k, int(max_scan_rows)))
    ws = _workspace({} if ws_slots is None else ws_slots, "_ws", need, q.device, capture_error)
    _lib.check(getattr(lib, f"lrx_{fam}_search{sfx}")(*head, int(max_scan_rows), k, int(id_base), _lib.ptr(D), _lib.ptr(I), _lib.ptr(row_map), *sel_args,
                                                      _lib.ptr(ws), ws.numel(), _s()))
    return D, I


def _ivf_range(F: _IvfFamily, name: str, sel, operands, radius: float, max_scan_rows: int, id_base: int = 0, row_map=None,
               ws_slots: Optional[dict] = None):
    """The range wrapper `name` of family F over its `operands` (q first): the checks, then the protocol of index._range_call over ONE library
    call for all Q queries (the library chunks them itself and carries lims on the device) -- outputs sized by a first guess, one host read
    of lims[Q], one retry when the guess was short.  ws_slots: as _ivf_topk's."""
    lib, fam, q = _lib.lib(), F.fam, operands[0]
    Q, dims, head = F.args(name, *operands)
    sel_args, sfx = ((), "") if sel is None else (_ivf_sel(name, sel[0], dims[0]), "_sel")
    if torch.cuda.is_current_stream_capturing():
        raise _lib.LrxError(f"{fam}_range_search under graph capture: the result length is read back to the host")
    if Q == 0:
        return _range_empty(q.device, 0)
    need = int(getattr(lib, f"lrx_{fam}_range_workspace_bytes")(*dims, int(max_scan_rows)))
    ws = _workspace({} if ws_slots is None else ws_slots, "_ws", need, q.device)
    fn = getattr(lib, f"lrx_{fam}_range_search{sfx}")
    return _range_call(q.device, Q, Q, lambda s, n, lims, D, I, cap: _lib.check(fn(
        *head, int(max_scan_rows), float(radius), int(id_base), _lib.ptr(lims), _lib.ptr(D), _lib.ptr(I), cap, _lib.ptr(row_map), *sel_args, _lib.ptr(ws),
        ws.numel(), _s())))


def _ivf_flat_args(name: str, q, X, list_off, row_ids, probes):
    Q, nprobe, ld = _ivf_probes(name, q, probes)
    n, d = X.shape
    nlist = list_off.numel() - 1
    return Q, (n, nlist, d, Q, nprobe), (_lib.ptr(X) if n else None, n, X.stride(0) if n > 1 else d, d, _lib.ptr(list_off), _lib.ptr(row_ids), nlist,
                                         _lib.ptr(q), Q, _lib.ptr(probes), nprobe, ld)


def ivf_flat_ip_range_search(q: torch.Tensor, X: torch.Tensor, list_off: torch.Tensor, row_ids: Optional[torch.Tensor], probes: torch.Tensor,
                             radius: float, max_scan_rows: int, id_base: int = 0, row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None):
    """lrx_ivf_flat_ip_range_search -> (lims i64[Q + 1], D f32[lims[Q]], I i64[lims[Q]]): every row of the cells probes[i] names whose exact
    score is > radius, in SEGMENT order (cells in the order of the probe row, rows by stored position), not sorted.  The arguments are
    ivf_flat_ip_topk's with radius for k.  Reads lims[Q] back to the host: refused under graph capture."""
    return _ivf_range(_IVF_FLAT, "ivf_flat_ip_range_search", None, (q, X, list_off, row_ids, probes), radius, max_scan_rows, id_base, row_map, ws_slots)


def ivf_flat_ip_topk(q: torch.Tensor, X: torch.Tensor, list_off: torch.Tensor, row_ids: Optional[torch.Tensor], probes: torch.Tensor, k: int,
                     max_scan_rows: int, id_base: int = 0, row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None,
                     capture_error: Optional[str] = None):
    """lrx_ivf_flat_ip_search -> (D f32[Q,k], I i64[Q,k]): the exact top k over the rows of the cells probes[i] names.  q fp32 [Q, d]
    contiguous; X fp32 [n, d] rows stored cell by cell; list_off int64 [nlist + 1]; row_ids int64 [n] (original row of a position) or None;
    probes int64 [Q, nprobe] (rows may be strided; < 0 skipped, >= nlist skipped and counted in lrx_device_error_count); max_scan_rows: the
    caller's bound on the rows one query scans.  ws_slots: a dict that keeps the workspace between calls (key "_ws")."""
    return _ivf_topk(_IVF_FLAT, "ivf_flat_ip_topk", None, (q, X, list_off, row_ids, probes), k, max_scan_rows, id_base, row_map, ws_slots, capture_error)


def _ivf_pq_args(name: str, q, codes, pq_centroids, list_off, row_ids, probes, probe_scores, by_residual):
    Q, nprobe, ld = _ivf_probes(name, q, probes)
    d = q.shape[1]
    M = pq_centroids.shape[0]
    n = codes.numel() // (-(-M // 16) * 16) if row_ids is None else row_ids.numel()
    if codes.dtype != torch.uint8 or codes.dim() != 1 or not codes.is_contiguous() or codes.numel() < -(-n // 128) * 128 * (-(-M // 16) * 16):
        raise ValueError(f"{name}: codes must be the 1-D blocked uint8 codes of the stored rows (whole 128-row blocks)")
    if pq_centroids.dtype != torch.float32 or not pq_centroids.is_contiguous() or tuple(pq_centroids.shape) != (M, 256, d // max(M, 1)) or d % M:
        raise ValueError(f"{name}: pq_centroids must be fp32 [M, 256, d / M] contiguous with d % M == 0")
    nlist = list_off.numel() - 1
    return Q, (n, nlist, d, M, Q, nprobe), (_lib.ptr(codes) if n else None, n, _lib.ptr(pq_centroids), d, M, _lib.ptr(list_off), _lib.ptr(row_ids), nlist,
                                            *_ivf_probe_args(name, q, Q, probes, probe_scores, nprobe, ld, by_residual))


def ivf_pq_ip_range_search(q: torch.Tensor, codes: torch.Tensor, pq_centroids: torch.Tensor, list_off: torch.Tensor, row_ids: Optional[torch.Tensor],
                           probes: torch.Tensor, probe_scores: Optional[torch.Tensor], by_residual: bool, radius: float, max_scan_rows: int,
                           id_base: int = 0, row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None):
    """lrx_ivf_pq_ip_range_search -> (lims, D, I): every row of the cells probes[i] names whose ADC score -- the value ivf_pq_ip_topk reports -- is
    > radius, in segment order (see ivf_flat_ip_range_search).  The arguments are ivf_pq_ip_topk's with radius for k."""
    return _ivf_range(_IVF_PQ, "ivf_pq_ip_range_search", None, (q, codes, pq_centroids, list_off, row_ids, probes, probe_scores, by_residual), radius,
                      max_scan_rows, id_base, row_map, ws_slots)


def ivf_pq_ip_topk(q: torch.Tensor, codes: torch.Tensor, pq_centroids: torch.Tensor, list_off: torch.Tensor, row_ids: Optional[torch.Tensor],
                   probes: torch.Tensor, probe_scores: Optional[torch.Tensor], by_residual: bool, k: int, max_scan_rows: int, id_base: int = 0,
                   row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None, capture_error: Optional[str] = None):
    """lrx_ivf_pq_ip_search -> (D f32[Q,k], I i64[Q,k]): the top k under the ADC score over the rows of the cells probes[i] names.  q fp32 [Q, d]
    contiguous; codes: the 1-D blocked uint8 PQ codes (whole 128-row blocks) by stored position, cell by cell; pq_centroids fp32 [M, 256, d / M];
    list_off int64 [nlist + 1] (list_off[nlist] = the rows held); row_ids int64 [n] (original row of a position) or None; probes int64
    [Q, nprobe] and probe_scores fp32 of the same shape and row stride (rows may be strided; None when not by_residual): a scanned row's score
    starts at its cell's probe score when by_residual, at 0 otherwise; max_scan_rows: the caller's bound on the rows one query scans.
    ws_slots: a dict that keeps the workspace between calls (key "_ws")."""
    return _ivf_topk(_IVF_PQ, "ivf_pq_ip_topk", None, (q, codes, pq_centroids, list_off, row_ids, probes, probe_scores, by_residual), k, max_scan_rows,
                     id_base, row_map, ws_slots, capture_error)


def _ivf_codes_args(name: str, dtype, dtype_name: str, q, codes, store, list_off, row_ids, probes, probe_scores, by_residual):
    """The searches over row-major codes (fp16, 8-bit); `store`: what the entry takes between d and list_off."""
    if codes.dtype != dtype or codes.dim() != 2 or not codes.is_contiguous() or codes.shape[1] != q.shape[1]:
        raise ValueError(f"{name}: codes must be {dtype_name} [n, d] contiguous with q's d")
    n, d = codes.shape
    Q, nprobe, ld = _ivf_probes(name, q, probes)
    if row_ids is not None and (row_ids.dtype != torch.int64 or not row_ids.is_contiguous() or row_ids.numel() < n):
        raise ValueError(f"{name}: row_ids must be int64 [>= n] contiguous")
    nlist = list_off.numel() - 1
    return Q, (n, nlist, d, Q, nprobe), (_lib.ptr(codes) if n else None, n, d, *store, _lib.ptr(list_off), _lib.ptr(row_ids), nlist,
                                         *_ivf_probe_args(name, q, Q, probes, probe_scores, nprobe, ld, by_residual))


def ivf_sq_fp16_ip_range_search(q: torch.Tensor, codes: torch.Tensor, list_off: torch.Tensor, row_ids: Optional[torch.Tensor], probes: torch.Tensor,
                                probe_scores: Optional[torch.Tensor], by_residual: bool, radius: float, max_scan_rows: int, id_base: int = 0,
                                row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None):
    """lrx_ivf_sq_fp16_ip_range_search -> (lims, D, I): every row of the cells probes[i] names whose score under the fp16 store -- the value
    ivf_sq_fp16_ip_topk reports -- is > radius, in segment order (see ivf_flat_ip_range_search).  The arguments are ivf_sq_fp16_ip_topk's with
    radius for k."""
    return _ivf_range(_IVF_SQ_FP16, "ivf_sq_fp16_ip_range_search", None, (q, codes, list_off, row_ids, probes, probe_scores, by_residual), radius,
                      max_scan_rows, id_base, row_map, ws_slots)


def ivf_sq_fp16_ip_topk(q: torch.Tensor, codes: torch.Tensor, list_off: torch.Tensor, row_ids: Optional[torch.Tensor], probes: torch.Tensor,
                        probe_scores: Optional[torch.Tensor], by_residual: bool, k: int, max_scan_rows: int, id_base: int = 0,
                        row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None, capture_error: Optional[str] = None):
    """lrx_ivf_sq_fp16_ip_search -> (D f32[Q,k], I i64[Q,k]): the exact top k under the fp16 store's score over the rows of the cells probes[i]
    names.  q fp32 [Q, d] contiguous; codes fp16 [n, d] contiguous, row-major by stored position, cell by cell; list_off int64 [nlist + 1];
    row_ids int64 [n] (original row of a position) or None; probes int64 [Q, nprobe] and probe_scores fp32 of the same shape and row stride
    (rows may be strided; None when not by_residual): a scanned row's score is its cell's probe score plus q . float(code) when by_residual,
    the product alone otherwise; max_scan_rows: the caller's bound on the rows one query scans.  ws_slots: a dict that keeps the workspace
    between calls (key "_ws")."""
    return _ivf_topk(_IVF_SQ_FP16, "ivf_sq_fp16_ip_topk", None, (q, codes, list_off, row_ids, probes, probe_scores, by_residual), k, max_scan_rows,
                     id_base, row_map, ws_slots, capture_error)


def _ivf_sq8_args(name: str, q, codes, trained, qtype, list_off, row_ids, probes, probe_scores, by_residual):
    if codes.dtype != torch.uint8 or codes.dim() != 2 or not codes.is_contiguous() or codes.shape[1] != q.shape[1]:
        raise ValueError(f"{name}: codes must be uint8 [n, d] contiguous with q's d")
    d = codes.shape[1]
    if qtype not in (0, 2) or trained.dtype != torch.float32 or not trained.is_contiguous() or trained.numel() != (2 * d if qtype == 0 else 2):
        raise ValueError(f"{name}: qtype {qtype} (0: QT_8bit, 2: QT_8bit_uniform) needs trained fp32 [2 d] or [2] contiguous")
    return _ivf_codes_args(name, torch.uint8, "uint8", q, codes, (_lib.ptr(trained), int(qtype)), list_off, row_ids, probes, probe_scores, by_residual)


def ivf_sq8_ip_range_search(q: torch.Tensor, codes: torch.Tensor, trained: torch.Tensor, qtype: int, list_off: torch.Tensor,
                            row_ids: Optional[torch.Tensor], probes: torch.Tensor, probe_scores: Optional[torch.Tensor], by_residual: bool, radius: float,
                            max_scan_rows: int, id_base: int = 0, row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None):
    """lrx_ivf_sq8_ip_range_search -> (lims, D, I): every row of the cells probes[i] names whose score under the 8-bit store -- the value
    ivf_sq8_ip_topk reports -- is > radius, in segment order (see ivf_flat_ip_range_search).  The arguments are ivf_sq8_ip_topk's with radius
    for k."""
    return _ivf_range(_IVF_SQ8, "ivf_sq8_ip_range_search", None, (q, codes, trained, qtype, list_off, row_ids, probes, probe_scores, by_residual), radius,
                      max_scan_rows, id_base, row_map, ws_slots)


def ivf_sq8_ip_topk(q: torch.Tensor, codes: torch.Tensor, trained: torch.Tensor, qtype: int, list_off: torch.Tensor, row_ids: Optional[torch.Tensor],
                    probes: torch.Tensor, probe_scores: Optional[torch.Tensor], by_residual: bool, k: int, max_scan_rows: int, id_base: int = 0,
                    row_map: Optional[torch.Tensor] = None, ws_slots: Optional[dict] = None, capture_error: Optional[str] = None):
    """lrx_ivf_sq8_ip_search -> (D f32[Q,k], I i64[Q,k]): the exact top k under the 8-bit store's score over the rows of the cells probes[i]
    names.  q fp32 [Q, d] contiguous; codes uint8 [n, d] contiguous, row-major by stored position, cell by cell; trained fp32 vmin ++ vdiff
    (2 d floats for qtype 0 = QT_8bit, 2 for qtype 2 = QT_8bit_uniform); list_off int64 [nlist + 1]; row_ids int64 [n] (original row of a
    position) or None; probes int64 [Q, nprobe] and probe_scores fp32 of the same shape and row stride (rows may be strided; None when not
    by_residual): a scanned row's score is its cell's probe score plus q . decoded row when by_residual, the product alone otherwise;
    max_scan_rows: the caller's bound on the rows one query scans.  ws_slots: a dict that keeps the workspace between calls (key "_ws")."""
    return _ivf_topk(_IVF_SQ8, "ivf_sq8_ip_topk", None, (q, codes, trained, qtype, list_off, row_ids, probes, probe_scores, by_residual), k, max_scan_rows,
                     id_base, row_map, ws_slots, capture_error)


# -- the four families: (stem of the library names, argument check, operands of a plain wrapper, where a *_sel wrapper takes `sel`) ---------
_IVF_FLAT = _IvfFamily("ivf_flat_ip", _ivf_flat_args, 5, 5)
_IVF_PQ = _IvfFamily("ivf_pq_ip", _ivf_pq_args, 8, 7)
_IVF_SQ_FP16 = _IvfFamily("ivf_sq_fp16_ip", lambda name, q, codes, *rest: _ivf_codes_args(name, torch.float16, "fp16", q, codes, (), *rest), 7, 6)
_IVF_SQ8 = _IvfFamily("ivf_sq8_ip", _ivf_sq8_args, 9, 8)


# -- the searches under a row selector (selector.RowSelector) -----------------------------------------------------------
# Each wrapper is its plain sibling with `sel` -- the selector's int32 words over the ORIGINAL rows, or None for no filter -- after the last
# positional tensor, as in torch.ops.lrx.*_sel: the top k (or every hit above the radius) over the SELECTED rows of the probed cells.
def _ivf_sel_wrapper(body, F: _IvfFamily, plain):
    name, at, end = plain.__name__ + "_sel", F.sel_at, F.n_operands + 1

    def wrapper(*a, **kw):
        return body(F, name, (a[at],), a[:at] + a[at + 1:end], *a[end:], **kw)
    wrapper.__name__ = wrapper.__qualname__ = name
    wrapper.__doc__ = f"{plain.__name__} under a row selector: its arguments with `sel` as positional {at}, its result over the selected rows."
    return wrapper


ivf_flat_ip_topk_sel = _ivf_sel_wrapper(_ivf_topk, _IVF_FLAT, ivf_flat_ip_topk)
ivf_flat_ip_range_search_sel = _ivf_sel_wrapper(_ivf_range, _IVF_FLAT, ivf_flat_ip_range_search)
ivf_pq_ip_topk_sel = _ivf_sel_wrapper(_ivf_topk, _IVF_PQ, ivf_pq_ip_topk)
ivf_pq_ip_range_search_sel = _ivf_sel_wrapper(_ivf_range, _IVF_PQ, ivf_pq_ip_range_search)
ivf_sq_fp16_ip_topk_sel = _ivf_sel_wrapper(_ivf_topk, _IVF_SQ_FP16, ivf_sq_fp16_ip_topk)
ivf_sq_fp16_ip_range_search_sel = _ivf_sel_wrapper(_ivf_range, _IVF_SQ_FP16, ivf_sq_fp16_ip_range_search)
ivf_sq8_ip_topk_sel = _ivf_sel_wrapper(_ivf_topk, _IVF_SQ8, ivf_sq8_ip_topk)
ivf_sq8_ip_range_search_sel = _ivf_sel_wrapper(_ivf_range, _IVF_SQ8, ivf_sq8_ip_range_search)
