// torch.ops.lrx.*: the PyTorch-ROCm custom-op binding of the C ABI in include/lrx.h (last row).
// A thin layer: tensors in, the current HIP stream, workspaces from PyTorch's caching allocator, errors -> TORCH_CHECK
// (Python RuntimeError).  Every op forwards to exactly one lrx_* entry point of liblrx.so; no arithmetic lives here.
// Built by lightretriever_amd/build.py into lightretriever_amd/liblrx_torch.so (next to liblrx.so, rpath $ORIGIN).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <c10/hip/HIPGraphsC10Utils.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <string>
#include <type_traits>

#include "../../include/lrx.h"

namespace {

// every op first makes the device of its first tensor current (getCurrentHIPStream() belongs to the CURRENT device, which need
// not be the tensors' device) and then takes that device's current stream
using DevGuard = c10::hip::OptionalHIPGuardMasqueradingAsCUDA;
void* cur_stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }

void lrx_check(int rc, const char* what) { TORCH_CHECK(rc == LRX_OK, what, ": liblrx error ", rc, ": ", lrx_last_error()); }

void need(const at::Tensor& t, const char* name, at::ScalarType dt, int64_t dim = -1) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(dim < 0 || t.dim() == dim, name, " must have ", dim, " dimensions");
  TORCH_CHECK(t.is_contiguous() || (t.dim() == 2 && t.stride(1) == 1), name, " must be contiguous (rows may be strided)");
}

at::Tensor bytes(int64_t n, const at::Tensor& like) { return at::empty({n}, like.options().dtype(at::kByte)); }

// ---- index ops: shared argument checks and outputs --------------------------------------------------------------------------------
// an optional 1-D tiled buffer of `dt` elements (include/lrx.h: whole 128-row blocks) that must hold rows [0, n_rows) of `width` columns
// -> its address, or null when absent; `msg` names the op
void* tiled_rows(const c10::optional<at::Tensor>& t, at::ScalarType dt, int64_t n_rows, int64_t width, const char* msg) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == dt && t->dim() == 1 && t->is_contiguous() && t->numel() >= ((n_rows + 127) / 128) * 128 * width, msg);
  return t->data_ptr();
}

// an optional int64 map of >= n_rows local rows -> its address, or null when absent; `msg` names the op
const int64_t* row_map_ptr(const c10::optional<at::Tensor>& row_map, int64_t n_rows, const char* msg) {
  if (!row_map.has_value()) return nullptr;
  need(*row_map, "row_map", at::kLong, 1);
  TORCH_CHECK(row_map->is_contiguous() && row_map->numel() >= n_rows, msg);
  return row_map->data_ptr<int64_t>();
}

// the [Q, k] outputs of a top-k search over queries q: fp32 scores d, int64 ids i and, for the wire ops, the int64 exchange words w
struct TopK {
  at::Tensor d, i, w;
};
TopK topk_out(const at::Tensor& q, int64_t k, bool wire = false) {
  const auto ids = q.options().dtype(at::kLong);
  return {at::empty({q.size(0), k}, q.options()), at::empty({q.size(0), k}, ids), wire ? at::empty({q.size(0), k}, ids) : at::Tensor()};
}

// ---- encoder ---------------------------------------------------------------------------------------------------------------------
// weights: the address of an lrx_encoder_handle {cfg*, weights*} kept alive by its owner (LrxEncoder.handle)
// shadow / row_bounds (optional): `out` = rows [shadow_row0, ...) of an index shard -- the last kernel also writes their tiled shadow rows and
// raises the shard's bounds (lrx_encode_packed_shard), like the ctypes path does for a live FlatIPIndex slot.  Without them a caller that
// encodes into committed shard rows must run shard_commit_rows afterwards.
void encode_packed(const at::Tensor& ids, const at::Tensor& cu_seqlens, int64_t max_seqlen, int64_t weights, at::Tensor out, int64_t mrl_dim,
                   bool normalize, const c10::optional<at::Tensor>& shadow, int64_t shadow_row0, const c10::optional<at::Tensor>& row_bounds) {
  DevGuard guard(ids.device());
  need(ids, "ids", at::kInt, 1);
  need(cu_seqlens, "cu_seqlens", at::kInt, 1);
  need(out, "out", at::kFloat, 2);
  TORCH_CHECK(weights != 0, "encode_packed: null weights handle");
  const lrx_encoder_handle* h = (const lrx_encoder_handle*)weights;
  const int64_t T = ids.numel(), B = cu_seqlens.numel() - 1;
  const int64_t D = mrl_dim > 0 ? mrl_dim : h->cfg->hidden_size;
  TORCH_CHECK(out.size(0) >= B && out.size(1) >= D, "encode_packed: out must be fp32 [>= n_seqs, >= mrl_dim]");
  const size_t need_b = lrx_encode_workspace_bytes(h->cfg, (int32_t)T, (int32_t)B);
  at::Tensor ws = bytes((int64_t)need_b, ids);
  void* sh = nullptr;
  if (shadow.has_value()) {
    TORCH_CHECK(shadow->is_cuda() && shadow->dim() == 1 && shadow->is_contiguous() && shadow->element_size() == 2 && D % 64 == 0 && D == out.size(1) &&
                    shadow_row0 >= 0 && shadow->numel() >= ((shadow_row0 + B + 127) / 128) * 128 * D,
                "encode_packed: shadow must be the shard's 1-D tiled 16-bit shadow (include/lrx.h), out its full-width rows from shadow_row0 on");
    sh = shadow->data_ptr();
  }
  float* rb = nullptr;
  if (row_bounds.has_value()) {
    need(*row_bounds, "row_bounds", at::kFloat, 1);
    TORCH_CHECK(row_bounds->numel() == 2, "encode_packed: row_bounds [2]");
    rb = row_bounds->data_ptr<float>();
  }
  lrx_check(lrx_encode_packed_shard(h->cfg, h->w, ids.data_ptr<int32_t>(), cu_seqlens.data_ptr<int32_t>(), (int32_t)B, (int32_t)T, (int32_t)max_seqlen,
                                    out.data_ptr<float>(), out.stride(0), (int32_t)D, normalize ? 1 : 0, sh, shadow_row0, rb, ws.data_ptr(), need_b,
                                    cur_stream()),
            "encode_packed");
}

// ---- unit kernels -------------------------------------------------------------------------------------------------------------------
at::Tensor rmsnorm(const at::Tensor& x, const at::Tensor& w, double eps) {
  DevGuard guard(x.device());
  need(x, "x", at::kBFloat16, 2);
  need(w, "w", at::kBFloat16, 1);
  TORCH_CHECK(x.is_contiguous() && w.numel() == x.size(1), "rmsnorm: x [rows, H] contiguous, w [H]");
  at::Tensor y = at::empty_like(x);
  lrx_check(lrx_rmsnorm(x.data_ptr(), w.data_ptr(), y.data_ptr(), (int32_t)x.size(0), (int32_t)x.size(1), (float)eps, cur_stream()), "rmsnorm");
  return y;
}

at::Tensor rope_qkv_gemm(const at::Tensor& a, const at::Tensor& wqkv, const c10::optional<at::Tensor>& bias, const at::Tensor& positions,
                         const at::Tensor& cos, const at::Tensor& sin, int64_t num_q_heads, int64_t num_kv_heads, int64_t head_dim) {
  DevGuard guard(a.device());
  need(a, "a", at::kBFloat16, 2);
  need(wqkv, "wqkv", at::kBFloat16, 2);
  need(positions, "positions", at::kInt, 1);
  need(cos, "cos", at::kFloat, 2);
  need(sin, "sin", at::kFloat, 2);
  TORCH_CHECK(a.is_contiguous() && wqkv.is_contiguous() && wqkv.size(1) == a.size(1), "rope_qkv_gemm: a [M,K], wqkv [N,K] contiguous");
  TORCH_CHECK(wqkv.size(0) == (num_q_heads + 2 * num_kv_heads) * head_dim, "rope_qkv_gemm: wqkv rows != (nq + 2 nkv) * d");
  at::Tensor c = at::empty({a.size(0), wqkv.size(0)}, a.options().dtype(at::kHalf));   // fp16, q | k columns in rotary-pair order (include/lrx.h)
  lrx_check(lrx_gemm_qkv_rope(a.data_ptr(), wqkv.data_ptr(), c.data_ptr(), bias.has_value() ? bias->data_ptr() : nullptr, positions.data_ptr<int32_t>(),
                              cos.data_ptr<float>(), sin.data_ptr<float>(), (int32_t)a.size(0), (int32_t)a.size(1), (int32_t)num_q_heads,
                              (int32_t)num_kv_heads, (int32_t)head_dim, cur_stream()),
            "rope_qkv_gemm");
  return c;
}

at::Tensor attn_varlen(const at::Tensor& qkv, const at::Tensor& cu_seqlens, int64_t max_seqlen, int64_t num_q_heads, int64_t num_kv_heads,
                       int64_t head_dim) {
  DevGuard guard(qkv.device());
  need(qkv, "qkv", at::kHalf, 2);
  need(cu_seqlens, "cu_seqlens", at::kInt, 1);
  TORCH_CHECK(qkv.is_contiguous() && qkv.size(1) == (num_q_heads + 2 * num_kv_heads) * head_dim, "attn_varlen: qkv [T, (nq + 2 nkv) * d] contiguous");
  at::Tensor out = at::empty({qkv.size(0), num_q_heads * head_dim}, qkv.options().dtype(at::kBFloat16));
  lrx_check(lrx_attn_varlen_causal(qkv.data_ptr(), cu_seqlens.data_ptr<int32_t>(), (int32_t)cu_seqlens.numel() - 1, (int32_t)qkv.size(0),
                                   (int32_t)max_seqlen, (int32_t)num_q_heads, (int32_t)num_kv_heads, (int32_t)head_dim, out.data_ptr(), 0, cur_stream()),
            "attn_varlen");
  return out;
}

at::Tensor swiglu_gemm(const at::Tensor& a, const at::Tensor& wgu) {
  DevGuard guard(a.device());
  need(a, "a", at::kBFloat16, 2);
  need(wgu, "wgu", at::kBFloat16, 2);
  TORCH_CHECK(a.is_contiguous() && wgu.is_contiguous() && wgu.size(1) == a.size(1) && wgu.size(0) % 2 == 0, "swiglu_gemm: a [M,K], wgu [2I,K] contiguous");
  at::Tensor c = at::empty({a.size(0), wgu.size(0) / 2}, a.options());
  lrx_check(lrx_gemm_bf16_nt(a.data_ptr(), wgu.data_ptr(), c.data_ptr(), nullptr, nullptr, (int32_t)a.size(0), (int32_t)wgu.size(0), (int32_t)a.size(1), 2,
                             cur_stream()),
            "swiglu_gemm");
  return c;
}

// ---- query side -------------------------------------------------------------------------------------------------------------------
at::Tensor embedding_bag_mean(const at::Tensor& table, const at::Tensor& ids, const at::Tensor& offsets, int64_t padding_idx, int64_t out_dim,
                              bool normalize) {
  DevGuard guard(table.device());
  need(table, "table", at::kFloat, 2);
  need(ids, "ids", at::kLong, 1);
  need(offsets, "offsets", at::kLong, 1);
  TORCH_CHECK(table.is_contiguous(), "embedding_bag_mean: table must be contiguous");
  const int64_t D = out_dim > 0 ? out_dim : table.size(1);
  at::Tensor out = at::empty({offsets.numel(), D}, table.options());
  lrx_check(lrx_embedding_bag_mean(table.data_ptr<float>(), (int32_t)table.size(0), (int32_t)table.size(1), ids.data_ptr<int64_t>(), ids.numel(),
                                   offsets.data_ptr<int64_t>(), (int32_t)offsets.numel(), padding_idx, out.data_ptr<float>(), out.stride(0), (int32_t)D,
                                   normalize ? 1 : 0, cur_stream()),
            "embedding_bag_mean");
  return out;
}

// ---- index ----------------------------------------------------------------------------------------------------------------------
std::tuple<at::Tensor, at::Tensor> flat_ip_topk(const at::Tensor& q, const at::Tensor& x, int64_t k, int64_t id_base,
                                                const c10::optional<at::Tensor>& row_bounds) {
  DevGuard guard(q.device());
  need(q, "q", at::kFloat, 2);
  need(x, "x", at::kFloat, 2);
  TORCH_CHECK(q.is_contiguous() && q.size(1) == x.size(1), "flat_ip_topk: q [Q,D] contiguous, x [N,D]");
  TopK o = topk_out(q, k);
  const size_t wsb = lrx_flat_ip_workspace_bytes(x.size(0), (int32_t)x.size(1), (int32_t)q.size(0), (int32_t)k);
  at::Tensor ws = bytes((int64_t)wsb, q);
  const float* rb = nullptr;
  if (row_bounds.has_value()) {
    need(*row_bounds, "row_bounds", at::kFloat, 1);
    TORCH_CHECK(row_bounds->numel() == 2, "flat_ip_topk: row_bounds [2]");
    rb = row_bounds->data_ptr<float>();
  }
  lrx_check(lrx_flat_ip_search(x.data_ptr<float>(), x.size(0), x.size(0) ? x.stride(0) : x.size(1), (int32_t)x.size(1), rb, q.data_ptr<float>(),
                               (int32_t)q.size(0), (int32_t)k, id_base, o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), ws.data_ptr(), wsb, cur_stream()),
            "flat_ip_topk");
  return {o.d, o.i};
}

// The store of the bounded searches (flat_ip_topk_bounded, its wire sibling and flat_ip_range_search; `op` names the one): x fp32 [N, D] rows,
// their 1-D tiled fp16 shadow x_shadow (include/lrx.h; block 0 row 0 = x row 0) or None, row_bounds [2] -> the shadow's address, or null
void* flat_bounded_args(const char* op, const at::Tensor& q, const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow, const at::Tensor& row_bounds) {
  need(q, "q", at::kFloat, 2);
  need(x, "x", at::kFloat, 2);
  need(row_bounds, "row_bounds", at::kFloat, 1);
  TORCH_CHECK(q.is_contiguous() && q.size(1) == x.size(1) && row_bounds.numel() == 2, op, ": q [Q,D] contiguous, x [N,D], row_bounds [2]");
  return tiled_rows(x_shadow, at::kHalf, x.size(0), x.size(1),
                    (std::string(op) + ": x_shadow must be the 1-D tiled fp16 shadow of x (whole 128-row blocks)").c_str());
}

// flags: LRX_SEARCH_FILTER_*
std::tuple<at::Tensor, at::Tensor> flat_ip_topk_bounded(const at::Tensor& q, const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow,
                                                        const at::Tensor& row_bounds, int64_t k, int64_t id_base, int64_t flags) {
  DevGuard guard(q.device());
  void* xb = flat_bounded_args("flat_ip_topk_bounded", q, x, x_shadow, row_bounds);
  TopK o = topk_out(q, k);
  const size_t wsb = lrx_flat_ip_bounded_workspace_bytes(x.size(0), (int32_t)x.size(1), (int32_t)q.size(0), (int32_t)k, (int32_t)flags);
  at::Tensor ws = bytes((int64_t)wsb, q);
  lrx_check(lrx_flat_ip_search_bounded(x.data_ptr<float>(), x.size(0), x.size(0) ? x.stride(0) : x.size(1), (int32_t)x.size(1), xb,
                                       row_bounds.data_ptr<float>(), q.data_ptr<float>(), (int32_t)q.size(0), (int32_t)k, id_base, o.d.data_ptr<float>(),
                                       o.i.data_ptr<int64_t>(), ws.data_ptr(), wsb, (int32_t)flags, cur_stream()),
            "flat_ip_topk_bounded");
  return {o.d, o.i};
}

// The same search for one rank of a row-sharded index: also returns the [Q, k] int64 wire words of the exchange (lrx_pack_topk's format,
// row_map applied), written by the search's own last kernel -- all_gather_into_tensor them and hand the result to merge_topk_packed.
std::tuple<at::Tensor, at::Tensor, at::Tensor> flat_ip_topk_bounded_wire(const at::Tensor& q, const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow,
                                                                         const at::Tensor& row_bounds, int64_t k, int64_t id_base,
                                                                         const c10::optional<at::Tensor>& row_map, int64_t flags) {
  DevGuard guard(q.device());
  void* xb = flat_bounded_args("flat_ip_topk_bounded_wire", q, x, x_shadow, row_bounds);
  const int64_t* rm = row_map_ptr(row_map, x.size(0), "flat_ip_topk_bounded_wire: row_map int64 [>= N] contiguous");
  TopK o = topk_out(q, k, true);
  const size_t wsb = lrx_flat_ip_bounded_workspace_bytes(x.size(0), (int32_t)x.size(1), (int32_t)q.size(0), (int32_t)k, (int32_t)flags);
  at::Tensor ws = bytes((int64_t)wsb, q);
  lrx_check(lrx_flat_ip_search_bounded_wire(x.data_ptr<float>(), x.size(0), x.size(0) ? x.stride(0) : x.size(1), (int32_t)x.size(1), xb,
                                            row_bounds.data_ptr<float>(), q.data_ptr<float>(), (int32_t)q.size(0), (int32_t)k, id_base, o.d.data_ptr<float>(),
                                            o.i.data_ptr<int64_t>(), rm, (uint64_t*)o.w.data_ptr<int64_t>(), ws.data_ptr(), wsb, (int32_t)flags, cur_stream()),
            "flat_ip_topk_bounded_wire");
  return {o.d, o.i, o.w};
}

// [R, Q, k] gathered wire words -> the global top-k (lrx_merge_topk_packed)
std::tuple<at::Tensor, at::Tensor> merge_topk_packed(const at::Tensor& words) {
  DevGuard guard(words.device());
  need(words, "words", at::kLong, 3);
  TORCH_CHECK(words.is_contiguous(), "merge_topk_packed: [R,Q,k] contiguous int64 words");
  const int64_t R = words.size(0), Q = words.size(1), k = words.size(2);
  at::Tensor d = at::empty({Q, k}, words.options().dtype(at::kFloat)), i = at::empty({Q, k}, words.options());
  lrx_check(lrx_merge_topk_packed((const uint64_t*)words.data_ptr<int64_t>(), (int32_t)R, (int32_t)Q, (int32_t)k, d.data_ptr<float>(), i.data_ptr<int64_t>(),
                                  cur_stream()),
            "merge_topk_packed");
  return {d, i};
}

// x_shadow: 1-D tiled fp16 shadow (whole 128-row blocks) with row0 = index of x's first row in it, or None (bounds only)
void shard_commit_rows(const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow, at::Tensor row_bounds, int64_t row0) {
  DevGuard guard(x.device());
  need(x, "x", at::kFloat, 2);
  need(row_bounds, "row_bounds", at::kFloat, 1);
  void* xb = tiled_rows(x_shadow, at::kHalf, row0 + x.size(0), x.size(1),
                        "shard_commit_rows: x_shadow must be the 1-D tiled fp16 shadow, large enough for rows row0 .. row0 + n");
  lrx_check(lrx_shard_commit_rows(x.data_ptr<float>(), x.stride(0), x.size(0), (int32_t)x.size(1), xb, row0, row_bounds.data_ptr<float>(), cur_stream()),
            "shard_commit_rows");
}

std::tuple<at::Tensor, at::Tensor> merge_topk(const at::Tensor& d_parts, const at::Tensor& i_parts) {
  DevGuard guard(d_parts.device());
  need(d_parts, "d_parts", at::kFloat, 3);
  need(i_parts, "i_parts", at::kLong, 3);
  TORCH_CHECK(d_parts.is_contiguous() && i_parts.is_contiguous() && d_parts.sizes() == i_parts.sizes(), "merge_topk: [R,Q,k] contiguous pairs");
  const int64_t R = d_parts.size(0), Q = d_parts.size(1), k = d_parts.size(2);
  at::Tensor d = at::empty({Q, k}, d_parts.options()), i = at::empty({Q, k}, i_parts.options());
  lrx_check(lrx_merge_topk(d_parts.data_ptr<float>(), i_parts.data_ptr<int64_t>(), (int32_t)R, (int32_t)Q, (int32_t)k, d.data_ptr<float>(),
                           i.data_ptr<int64_t>(), cur_stream()),
            "merge_topk");
  return {d, i};
}

// The store of the fp16 scalar-quantised index (sq_fp16_ip_topk and sq_fp16_ip_range_search; `op` names the one): codes = the 1-D tiled fp16
// codes (include/lrx.h, whole 128-row blocks) holding n_rows rows of q.size(1) columns; row_bounds [2] as maintained by shard_commit_rows
// -> the codes' address
void* sq_fp16_args(const char* op, const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& row_bounds) {
  need(q, "q", at::kFloat, 2);
  need(row_bounds, "row_bounds", at::kFloat, 1);
  TORCH_CHECK(q.is_contiguous() && row_bounds.numel() == 2 && q.size(1) % 64 == 0 && n_rows >= 0, op,
              ": q [Q,D] contiguous with D % 64 == 0, row_bounds [2], n_rows >= 0");
  return tiled_rows(codes, at::kHalf, n_rows, q.size(1),
                    (std::string(op) + ": codes must be the 1-D tiled fp16 codes of n_rows rows (whole 128-row blocks)").c_str());
}

// lrx_sq_fp16_ip_search.  Returns (D, I, wire words) like flat_ip_topk_bounded_wire.
std::tuple<at::Tensor, at::Tensor, at::Tensor> sq_fp16_ip_topk(const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& row_bounds,
                                                               int64_t k, int64_t id_base, const c10::optional<at::Tensor>& row_map, int64_t flags) {
  DevGuard guard(q.device());
  void* cb = sq_fp16_args("sq_fp16_ip_topk", q, codes, n_rows, row_bounds);
  const int64_t dim = q.size(1);
  const int64_t* rm = row_map_ptr(row_map, n_rows, "sq_fp16_ip_topk: row_map int64 [>= n_rows] contiguous");
  TopK o = topk_out(q, k, true);
  const size_t wsb = lrx_sq_fp16_ip_workspace_bytes(n_rows, (int32_t)dim, (int32_t)q.size(0), (int32_t)k, (int32_t)flags);
  at::Tensor ws = bytes((int64_t)wsb, q);
  lrx_check(lrx_sq_fp16_ip_search(cb, n_rows, (int32_t)dim, row_bounds.data_ptr<float>(), q.data_ptr<float>(), (int32_t)q.size(0), (int32_t)k, id_base,
                                  o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), rm, (uint64_t*)o.w.data_ptr<int64_t>(), ws.data_ptr(), wsb, (int32_t)flags,
                                  cur_stream()),
            "sq_fp16_ip_topk");
  return {o.d, o.i, o.w};
}

// Rerank (lrx_flat_ip_rerank / lrx_sq_fp16_ip_rerank): the exact scores of the caller's candidate rows cand [Q, n_cand] (int64 row numbers, rows
// may be strided; < 0 skipped, >= n_rows skipped and counted) and their top k.  Returns (D, I).
struct RerankArgs {
  int64_t n_cand, ld_cand;
  const int64_t* rm;
  at::Tensor ws;
  size_t wsb;
};
RerankArgs rerank_args(const char* op, const at::Tensor& q, int64_t dim, const at::Tensor& cand, int64_t k, int64_t n_rows,
                       const c10::optional<at::Tensor>& row_map) {
  need(q, "q", at::kFloat, 2);
  need(cand, "cand", at::kLong, 2);
  TORCH_CHECK(q.is_contiguous() && q.size(1) == dim && cand.size(0) == q.size(0), op, ": q [Q,D] contiguous, cand int64 [Q, n_cand]");
  const int64_t n_cand = cand.size(1);
  TORCH_CHECK(1 <= k && k <= n_cand && n_cand <= 2048 && n_rows >= 0, op, ": need 1 <= k <= n_cand <= 2048, got k=", k, ", n_cand=", n_cand);
  RerankArgs a;
  a.n_cand = n_cand;
  a.ld_cand = cand.size(0) > 1 ? cand.stride(0) : n_cand;
  a.rm = row_map_ptr(row_map, n_rows, "rerank: row_map int64 [>= n_rows] contiguous");
  a.wsb = lrx_ip_rerank_workspace_bytes((int32_t)q.size(0), (int32_t)n_cand, (int32_t)k);
  a.ws = bytes((int64_t)a.wsb, q);
  return a;
}

std::tuple<at::Tensor, at::Tensor> flat_ip_rerank(const at::Tensor& q, const at::Tensor& x, const at::Tensor& cand, int64_t k, int64_t id_base,
                                                  const c10::optional<at::Tensor>& row_map) {
  DevGuard guard(q.device());
  need(x, "x", at::kFloat, 2);
  const int64_t n_rows = x.size(0), dim = x.size(1);
  TORCH_CHECK(dim % 4 == 0 && dim > 0, "flat_ip_rerank: x [n_rows, D] with D % 4 == 0");
  RerankArgs a = rerank_args("flat_ip_rerank", q, dim, cand, k, n_rows, row_map);
  TopK o = topk_out(q, k);
  lrx_check(lrx_flat_ip_rerank(x.data_ptr<float>(), n_rows, n_rows > 1 ? x.stride(0) : dim, (int32_t)dim, q.data_ptr<float>(), (int32_t)q.size(0),
                               cand.data_ptr<int64_t>(), (int32_t)a.n_cand, a.ld_cand, (int32_t)k, id_base, o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(),
                               a.rm, a.ws.data_ptr(), a.wsb, cur_stream()),
            "flat_ip_rerank");
  return {o.d, o.i};
}

std::tuple<at::Tensor, at::Tensor> sq_fp16_ip_rerank(const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& cand, int64_t k,
                                                     int64_t id_base, const c10::optional<at::Tensor>& row_map) {
  DevGuard guard(q.device());
  TORCH_CHECK(q.dim() == 2 && q.size(1) % 64 == 0 && q.size(1) > 0 && n_rows >= 0, "sq_fp16_ip_rerank: q [Q,D] with D % 64 == 0, n_rows >= 0");
  const int64_t dim = q.size(1);
  RerankArgs a = rerank_args("sq_fp16_ip_rerank", q, dim, cand, k, n_rows, row_map);
  void* cb = tiled_rows(codes, at::kHalf, n_rows, dim, "sq_fp16_ip_rerank: codes must be the 1-D tiled fp16 codes of n_rows rows (whole 128-row blocks)");
  TopK o = topk_out(q, k);
  lrx_check(lrx_sq_fp16_ip_rerank(cb, n_rows, (int32_t)dim, q.data_ptr<float>(), (int32_t)q.size(0), cand.data_ptr<int64_t>(), (int32_t)a.n_cand, a.ld_cand,
                                  (int32_t)k, id_base, o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), a.rm, a.ws.data_ptr(), a.wsb, cur_stream()),
            "sq_fp16_ip_rerank");
  return {o.d, o.i};
}

// The result protocol of every range-search op (lrx_flat_ip_range_search / lrx_sq_fp16_ip_range_search / lrx_pq_ip_range_search /
// lrx_range_impact_search): `call(lims, d, i, cap)` runs the library call, lims[Q] is read back to the host once, and the call is repeated
// once with the exact capacity when the first guess of 1024 hits per query was short.  Refused under graph capture before anything is launched.
template <class Call>
std::tuple<at::Tensor, at::Tensor, at::Tensor> range_result(const at::Tensor& like, int64_t Q, const char* who, Call call) {
  TORCH_CHECK(c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None, who,
              " under graph capture: the result length is read back to the host");
  const auto f32 = like.options().dtype(at::kFloat);
  at::Tensor lims = at::zeros({Q + 1}, f32.dtype(at::kLong));
  int64_t cap = Q * 1024;
  for (int attempt = 0; attempt < 2; ++attempt) {
    at::Tensor d = at::empty({cap}, f32), i = at::empty({cap}, f32.dtype(at::kLong));
    lrx_check(call(lims.data_ptr<int64_t>(), d.data_ptr<float>(), i.data_ptr<int64_t>(), cap), who);
    const int64_t n = lims[Q].item<int64_t>();
    if (n <= cap) return {lims, d.narrow(0, 0, n), i.narrow(0, 0, n)};
    cap = n;
  }
  TORCH_CHECK(false, who, ": the result grew between two identical calls");
}

// ---- inverted file: the four families (flat, PQ, fp16, 8-bit) ------------------------------------------------------------------
// Each family has four ops -- <name>_topk, <name>_range_search and a *_sel variant of each (a search under a row selector) -- over four library
// entries that start with the same head of arguments, the family's store through ld_probe / by_residual, and end with one of two tails, the
// same for all families (include/lrx.h).  So every list is written once: a family below is a struct that checks its operands (its *_args),
// sizes its two workspaces, names its four entries and, in head(), spells the head; ivf_search() -- one for top-k, one for range -- holds the
// selector check, the workspace, the outputs, the tail and the choice between the plain and the *_sel entry; IvfOp turns a family into its four
// registered functions.  A plain op calls the plain entry, a *_sel op the *_sel entry, also when its selector is None.

// The result of a top-k op, as range_result is of a range op: `call(d, i)` runs the library call over the outputs.
template <class Call>
std::tuple<at::Tensor, at::Tensor> topk_result(const at::Tensor& q, int64_t k, const char* who, Call call) {
  TopK o = topk_out(q, k);
  lrx_check(call(o.d.data_ptr<float>(), o.i.data_ptr<int64_t>()), who);
  return {o.d, o.i};
}

// What the four families check alike, after need() on q and on their own store: list_off int64 [nlist + 1], probes int64 [Q, nprobe] (rows may
// be strided; < 0 skipped, >= nlist skipped and counted), max_scan_rows = the caller's bound on the rows one query scans, row_ids int64 (the
// original row of a position) or None, probe_scores fp32 [Q, nprobe] with the row stride of probes when by_residual, row_map.  `store_ok` is the
// family's own part of the shape check and `shapes` the sentence that names every operand of it.
using OptTensor = c10::optional<at::Tensor>;
struct IvfArgs {
  int64_t Q, nlist, nprobe, ld_probe;
  const int64_t *ri, *rm;
  const float* ps;
};
IvfArgs ivf_args(const char* who, const at::Tensor& q, bool store_ok, const char* shapes, int64_t n_rows, const at::Tensor& list_off, const OptTensor& row_ids,
                 const at::Tensor& probes, const OptTensor& probe_scores, bool by_residual, int64_t max_scan_rows, const OptTensor& row_map) {
  need(list_off, "list_off", at::kLong, 1);
  need(probes, "probes", at::kLong, 2);
  IvfArgs a{q.size(0), list_off.size(0) - 1, probes.size(1), 0, nullptr, nullptr, nullptr};
  TORCH_CHECK(q.is_contiguous() && store_ok && probes.size(0) == a.Q && list_off.is_contiguous() && a.nlist >= 1 && (a.nprobe == 0 || probes.stride(1) == 1),
              who, shapes);
  TORCH_CHECK(max_scan_rows >= 0 && max_scan_rows < (1ll << 31) && a.nlist < (1ll << 31) && a.nprobe < (1ll << 31), who, ": sizes out of range");
  if (row_ids.has_value() && row_ids->defined()) {
    need(*row_ids, "row_ids", at::kLong, 1);
    TORCH_CHECK(row_ids->is_contiguous() && row_ids->numel() >= n_rows, who, ": row_ids int64 [>= n_rows] contiguous");
    a.ri = row_ids->data_ptr<int64_t>();
  }
  a.ld_probe = a.Q > 1 ? probes.stride(0) : a.nprobe;
  if (by_residual) {
    TORCH_CHECK(probe_scores.has_value() && probe_scores->defined(), who, ": by_residual needs probe_scores");
    need(*probe_scores, "probe_scores", at::kFloat, 2);
    TORCH_CHECK(probe_scores->sizes() == probes.sizes() && (a.nprobe == 0 || probe_scores->stride(1) == 1) && (a.Q <= 1 || probe_scores->stride(0) == a.ld_probe),
                who, ": probe_scores fp32 [Q, nprobe] with the row stride of probes");
    a.ps = probe_scores->data_ptr<float>();
  }
  a.rm = row_map_ptr(row_map, n_rows, (std::string(who) + ": row_map int64 [>= n_rows] contiguous").c_str());
  return a;
}

// The selector of a *_sel op (include/lrx.h, ROW SELECTOR): the int32 words of a bitmap over the n_rows original rows, [ceil(n_rows / 32)]
// contiguous on the device, or None (no filter).  sel == nullptr: a plain op.
const uint32_t* ivf_sel_bits(const char* who, const OptTensor* sel, int64_t n_rows) {
  if (sel == nullptr || !sel->has_value() || !(*sel)->defined()) return nullptr;
  const at::Tensor& t = **sel;
  need(t, "sel", at::kInt, 1);
  TORCH_CHECK(t.is_contiguous() && t.numel() == (n_rows + 31) / 32, who, ": sel must be the int32 words of a selector over the ", n_rows,
              " rows of the index: [", (n_rows + 31) / 32, "] contiguous");
  return (const uint32_t*)t.data_ptr<int32_t>();
}

// Top k over the probed cells.  Every top-k entry ends (max_scan_rows, k, id_base, D, I, row_map, [sel words, sel rows,] ws, bytes, stream).
// Returns (D, I).
template <class Fam>
std::tuple<at::Tensor, at::Tensor> ivf_search(const char* who, const Fam& f, const OptTensor* sel, int64_t k, int64_t max_scan_rows, int64_t id_base) {
  const size_t wsb = f.topk_bytes(k, max_scan_rows);
  const uint32_t* sb = ivf_sel_bits(who, sel, f.n_rows);
  at::Tensor ws = bytes((int64_t)wsb, f.q);
  return topk_result(f.q, k, who, [&](float* d, int64_t* i) {
    return sel != nullptr ? f.head(Fam::topk_sel, max_scan_rows, (int32_t)k, id_base, d, i, f.a.rm, sb, f.n_rows, ws.data_ptr(), wsb, cur_stream())
                          : f.head(Fam::topk, max_scan_rows, (int32_t)k, id_base, d, i, f.a.rm, ws.data_ptr(), wsb, cur_stream());
  });
}

// Range search over the probed cells: the top-k op's arguments with radius for k.  Every range entry ends (max_scan_rows, radius, id_base, lims,
// D, I, capacity, row_map, [sel words, sel rows,] ws, bytes, stream).  Returns (lims, D, I), the hits of a query in segment order (cells in
// probe order, rows by stored position).
template <class Fam>
std::tuple<at::Tensor, at::Tensor, at::Tensor> ivf_search(const char* who, const Fam& f, const OptTensor* sel, double radius, int64_t max_scan_rows,
                                                          int64_t id_base) {
  const size_t wsb = f.range_bytes(max_scan_rows);
  const uint32_t* sb = ivf_sel_bits(who, sel, f.n_rows);
  at::Tensor ws = bytes((int64_t)wsb, f.q);
  return range_result(f.q, f.a.Q, who, [&](int64_t* lims, float* d, int64_t* i, int64_t cap) {
    return sel != nullptr
               ? f.head(Fam::range_sel, max_scan_rows, (float)radius, id_base, lims, d, i, cap, f.a.rm, sb, f.n_rows, ws.data_ptr(), wsb, cur_stream())
               : f.head(Fam::range, max_scan_rows, (float)radius, id_base, lims, d, i, cap, f.a.rm, ws.data_ptr(), wsb, cur_stream());
  });
}

// The four registered functions of a family: its ops take q, the family's Operands, `sel` (the *_sel ops only), its Flags, then k (int64: top k)
// or radius (double: range search), max_scan_rows, id_base and row_map.  The op's name, `who`, goes into every message.
template <class... T>
struct Types {};
template <class Fam, class Scalar, class Operands = typename Fam::Operands, class Flags = typename Fam::Flags>
struct IvfOp;
template <class Fam, class Scalar, class... Operands, class... Flags>
struct IvfOp<Fam, Scalar, Types<Operands...>, Types<Flags...>> {
  static auto run(const OptTensor* sel, const at::Tensor& q, Operands... o, Flags... f, Scalar scalar, int64_t max_scan_rows, int64_t id_base,
                  const OptTensor& row_map) {
    DevGuard guard(q.device());
    const std::string who = std::string(Fam::name) + (std::is_same<Scalar, double>::value ? "_range_search" : "_topk") + (sel != nullptr ? "_sel" : "");
    return ivf_search(who.c_str(), Fam(who.c_str(), q, o..., f..., max_scan_rows, row_map), sel, scalar, max_scan_rows, id_base);
  }
  static auto plain(const at::Tensor& q, Operands... o, Flags... f, Scalar scalar, int64_t max_scan_rows, int64_t id_base, const OptTensor& row_map) {
    return run(nullptr, q, o..., f..., scalar, max_scan_rows, id_base, row_map);
  }
  static auto with_sel(const at::Tensor& q, Operands... o, const OptTensor& sel, Flags... f, Scalar scalar, int64_t max_scan_rows, int64_t id_base,
                  const OptTensor& row_map) {
    return run(&sel, q, o..., f..., scalar, max_scan_rows, id_base, row_map);
  }
};
using TRef = const at::Tensor&;   // (the operand types of the families below)
using ORef = const OptTensor&;

// Flat: x [n_rows, D] fp32 rows stored cell by cell.
IvfArgs ivf_flat_ip_args(const char* who, TRef q, TRef x, TRef list_off, ORef row_ids, TRef probes, int64_t max_scan_rows, ORef row_map) {
  need(q, "q", at::kFloat, 2);
  need(x, "x", at::kFloat, 2);
  return ivf_args(who, q, q.size(1) == x.size(1) && (x.size(0) <= 1 || x.stride(1) == 1),
                  ": q [Q,D] contiguous, x [n_rows,D], list_off int64 [nlist + 1], probes int64 [Q, nprobe]", x.size(0), list_off, row_ids, probes, c10::nullopt,
                  false, max_scan_rows, row_map);
}
struct IvfFlat {
  static constexpr const char* name = "ivf_flat_ip";
  static constexpr auto topk = &lrx_ivf_flat_ip_search;
  static constexpr auto topk_sel = &lrx_ivf_flat_ip_search_sel;
  static constexpr auto range = &lrx_ivf_flat_ip_range_search;
  static constexpr auto range_sel = &lrx_ivf_flat_ip_range_search_sel;
  using Operands = Types<TRef /*x*/, TRef /*list_off*/, ORef /*row_ids*/, TRef /*probes*/>;
  using Flags = Types<>;
  TRef q, x, list_off, probes;
  const IvfArgs a;
  const int64_t n_rows, dim;
  IvfFlat(const char* who, TRef q, TRef x, TRef list_off, ORef row_ids, TRef probes, int64_t max_scan_rows, ORef row_map)
      : q(q), x(x), list_off(list_off), probes(probes), a(ivf_flat_ip_args(who, q, x, list_off, row_ids, probes, max_scan_rows, row_map)),
        n_rows(x.size(0)), dim(x.size(1)) {}
  size_t topk_bytes(int64_t k, int64_t max_scan_rows) const {
    return lrx_ivf_flat_ip_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)dim, (int32_t)a.Q, (int32_t)a.nprobe, (int32_t)k, max_scan_rows);
  }
  size_t range_bytes(int64_t max_scan_rows) const {
    return lrx_ivf_flat_ip_range_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)dim, (int32_t)a.Q, (int32_t)a.nprobe, max_scan_rows);
  }
  template <class Entry, class... Tail>
  int head(Entry entry, Tail... tail) const {
    return entry(n_rows ? x.data_ptr<float>() : nullptr, n_rows, n_rows > 1 ? x.stride(0) : dim, (int32_t)dim, list_off.data_ptr<int64_t>(), a.ri,
                 (int32_t)a.nlist, q.data_ptr<float>(), (int32_t)a.Q, probes.data_ptr<int64_t>(), (int32_t)a.nprobe, a.ld_probe, tail...);
  }
};

// PQ codes: codes = the 1-D blocked uint8 PQ codes (whole 128-row blocks) by stored position, cell by cell; pq_centroids [M, 256, D / M] fp32;
// n_rows is the length of row_ids, or the rows the code blocks hold.
struct IvfPqStore {
  int64_t n_rows, dim, M;
  void* cb;
};
IvfArgs ivf_pq_ip_args(const char* who, TRef q, TRef codes, TRef pq_centroids, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual,
                       int64_t max_scan_rows, ORef row_map, IvfPqStore& st) {
  need(q, "q", at::kFloat, 2);
  need(pq_centroids, "pq_centroids", at::kFloat, 3);
  const std::string blocked = std::string(who) + ": codes must be the 1-D blocked uint8 codes of the stored rows (whole 128-row blocks)";
  TORCH_CHECK(codes.is_cuda() && codes.scalar_type() == at::kByte && codes.dim() == 1 && codes.is_contiguous(), blocked);
  const int64_t dim = q.size(1), M = pq_centroids.size(0);
  const bool store_ok = pq_centroids.is_contiguous() && pq_centroids.size(1) == 256 && M > 0 && dim % M == 0 && pq_centroids.size(2) == dim / M;
  const int64_t mp = (M + 15) / 16 * 16;
  const int64_t n_rows = row_ids.has_value() && row_ids->defined() ? row_ids->numel() : (store_ok ? codes.numel() / mp : 0);
  const IvfArgs a = ivf_args(who, q, store_ok, ": q [Q,D] contiguous, pq_centroids [M,256,D/M] contiguous with D % M == 0, list_off int64 [nlist + 1], probes int64 [Q, nprobe]",
                             n_rows, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map);
  st = IvfPqStore{n_rows, dim, M, tiled_rows(codes, at::kByte, n_rows, mp, blocked.c_str())};
  return a;
}
struct IvfPq {
  static constexpr const char* name = "ivf_pq_ip";
  static constexpr auto topk = &lrx_ivf_pq_ip_search;
  static constexpr auto topk_sel = &lrx_ivf_pq_ip_search_sel;
  static constexpr auto range = &lrx_ivf_pq_ip_range_search;
  static constexpr auto range_sel = &lrx_ivf_pq_ip_range_search_sel;
  using Operands = Types<TRef /*codes*/, TRef /*pq_centroids*/, TRef /*list_off*/, ORef /*row_ids*/, TRef /*probes*/, ORef /*probe_scores*/>;
  using Flags = Types<bool /*by_residual*/>;
  TRef q, pq_centroids, list_off, probes;
  const bool by_residual;
  IvfPqStore st;
  const IvfArgs a;
  const int64_t n_rows;
  IvfPq(const char* who, TRef q, TRef codes, TRef pq_centroids, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual, int64_t max_scan_rows, ORef row_map)
      : q(q), pq_centroids(pq_centroids), list_off(list_off), probes(probes), by_residual(by_residual),
        a(ivf_pq_ip_args(who, q, codes, pq_centroids, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map, st)), n_rows(st.n_rows) {}
  size_t topk_bytes(int64_t k, int64_t max_scan_rows) const {
    return lrx_ivf_pq_ip_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)st.dim, (int32_t)st.M, (int32_t)a.Q, (int32_t)a.nprobe, (int32_t)k, max_scan_rows);
  }
  size_t range_bytes(int64_t max_scan_rows) const {
    return lrx_ivf_pq_ip_range_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)st.dim, (int32_t)st.M, (int32_t)a.Q, (int32_t)a.nprobe, max_scan_rows);
  }
  template <class Entry, class... Tail>
  int head(Entry entry, Tail... tail) const {
    return entry(n_rows ? st.cb : nullptr, n_rows, pq_centroids.data_ptr<float>(), (int32_t)st.dim, (int32_t)st.M, list_off.data_ptr<int64_t>(), a.ri,
                 (int32_t)a.nlist, q.data_ptr<float>(), (int32_t)a.Q, probes.data_ptr<int64_t>(), a.ps, (int32_t)a.nprobe, a.ld_probe, by_residual ? 1 : 0,
                 tail...);
  }
};

// Row-major codes [n_rows, D] contiguous, by stored position, cell by cell: fp16 (IvfSqFp16) and 8-bit (IvfSq8).  `shapes`: the family's sentence
// for the shape check.
IvfArgs ivf_codes_args(const char* who, TRef q, TRef codes, at::ScalarType code_type, const char* shapes, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores,
                       bool by_residual, int64_t max_scan_rows, ORef row_map) {
  need(q, "q", at::kFloat, 2);
  need(codes, "codes", code_type, 2);
  return ivf_args(who, q, q.size(1) == codes.size(1) && codes.is_contiguous(), shapes, codes.size(0), list_off, row_ids, probes, probe_scores, by_residual,
                  max_scan_rows, row_map);
}
const char* const kIvfSqShapes = ": q [Q,D] contiguous, codes fp16 [n_rows,D] contiguous, list_off int64 [nlist + 1], probes int64 [Q, nprobe]";
const char* const kIvfSq8Shapes = ": q [Q,D] contiguous, codes uint8 [n_rows,D] contiguous, list_off int64 [nlist + 1], probes int64 [Q, nprobe]";

struct IvfSqFp16 {
  static constexpr const char* name = "ivf_sq_fp16_ip";
  static constexpr auto topk = &lrx_ivf_sq_fp16_ip_search;
  static constexpr auto topk_sel = &lrx_ivf_sq_fp16_ip_search_sel;
  static constexpr auto range = &lrx_ivf_sq_fp16_ip_range_search;
  static constexpr auto range_sel = &lrx_ivf_sq_fp16_ip_range_search_sel;
  using Operands = Types<TRef /*codes*/, TRef /*list_off*/, ORef /*row_ids*/, TRef /*probes*/, ORef /*probe_scores*/>;
  using Flags = Types<bool /*by_residual*/>;
  TRef q, codes, list_off, probes;
  const bool by_residual;
  const IvfArgs a;
  const int64_t n_rows, dim;
  IvfSqFp16(const char* who, TRef q, TRef codes, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual, int64_t max_scan_rows, ORef row_map)
      : q(q), codes(codes), list_off(list_off), probes(probes), by_residual(by_residual),
        a(ivf_codes_args(who, q, codes, at::kHalf, kIvfSqShapes, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map)),
        n_rows(codes.size(0)), dim(codes.size(1)) {}
  size_t topk_bytes(int64_t k, int64_t max_scan_rows) const {
    return lrx_ivf_sq_fp16_ip_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)dim, (int32_t)a.Q, (int32_t)a.nprobe, (int32_t)k, max_scan_rows);
  }
  size_t range_bytes(int64_t max_scan_rows) const {
    return lrx_ivf_sq_fp16_ip_range_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)dim, (int32_t)a.Q, (int32_t)a.nprobe, max_scan_rows);
  }
  template <class Entry, class... Tail>
  int head(Entry entry, Tail... tail) const {
    return entry(n_rows ? codes.data_ptr() : nullptr, n_rows, (int32_t)dim, list_off.data_ptr<int64_t>(), a.ri, (int32_t)a.nlist, q.data_ptr<float>(),
                 (int32_t)a.Q, probes.data_ptr<int64_t>(), a.ps, (int32_t)a.nprobe, a.ld_probe, by_residual ? 1 : 0, tail...);
  }
};

// The 8-bit family's own operands: trained fp32 vmin ++ vdiff (2 D floats for qtype 0, 2 for qtype 2).
IvfArgs ivf_sq8_ip_args(const char* who, TRef q, TRef codes, TRef trained, int64_t qtype, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual,
                        int64_t max_scan_rows, ORef row_map) {
  need(q, "q", at::kFloat, 2);
  need(codes, "codes", at::kByte, 2);
  need(trained, "trained", at::kFloat, 1);
  TORCH_CHECK((qtype == 0 || qtype == 2) && trained.is_contiguous() && trained.numel() == (qtype == 0 ? 2 * codes.size(1) : 2),
              who, ": qtype ", qtype, " (0: QT_8bit, 2: QT_8bit_uniform) with trained fp32 [2 D] or [2] contiguous");
  return ivf_codes_args(who, q, codes, at::kByte, kIvfSq8Shapes, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map);
}
struct IvfSq8 {
  static constexpr const char* name = "ivf_sq8_ip";
  static constexpr auto topk = &lrx_ivf_sq8_ip_search;
  static constexpr auto topk_sel = &lrx_ivf_sq8_ip_search_sel;
  static constexpr auto range = &lrx_ivf_sq8_ip_range_search;
  static constexpr auto range_sel = &lrx_ivf_sq8_ip_range_search_sel;
  using Operands = Types<TRef /*codes*/, TRef /*trained*/, int64_t /*qtype*/, TRef /*list_off*/, ORef /*row_ids*/, TRef /*probes*/, ORef /*probe_scores*/>;
  using Flags = Types<bool /*by_residual*/>;
  TRef q, codes, trained, list_off, probes;
  const int64_t qtype;
  const bool by_residual;
  const IvfArgs a;
  const int64_t n_rows, dim;
  IvfSq8(const char* who, TRef q, TRef codes, TRef trained, int64_t qtype, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual, int64_t max_scan_rows,
         ORef row_map)
      : q(q), codes(codes), trained(trained), list_off(list_off), probes(probes), qtype(qtype), by_residual(by_residual),
        a(ivf_sq8_ip_args(who, q, codes, trained, qtype, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map)),
        n_rows(codes.size(0)), dim(codes.size(1)) {}
  size_t topk_bytes(int64_t k, int64_t max_scan_rows) const {
    return lrx_ivf_sq8_ip_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)dim, (int32_t)a.Q, (int32_t)a.nprobe, (int32_t)k, max_scan_rows);
  }
  size_t range_bytes(int64_t max_scan_rows) const {
    return lrx_ivf_sq8_ip_range_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)dim, (int32_t)a.Q, (int32_t)a.nprobe, max_scan_rows);
  }
  template <class Entry, class... Tail>
  int head(Entry entry, Tail... tail) const {
    return entry(n_rows ? codes.data_ptr() : nullptr, n_rows, (int32_t)dim, trained.data_ptr<float>(), (int32_t)qtype, list_off.data_ptr<int64_t>(), a.ri,
                 (int32_t)a.nlist, q.data_ptr<float>(), (int32_t)a.Q, probes.data_ptr<int64_t>(), a.ps, (int32_t)a.nprobe, a.ld_probe, by_residual ? 1 : 0,
                 tail...);
  }
};

// The store of the product-quantised index (pq_ip_topk and pq_ip_range_search; `op` names the one): codes = the 1-D blocked uint8 codes
// (include/lrx.h, whole 128-row blocks) of n_rows rows, centroids [M, 256, D / M] fp32 -> the codes' address
void* pq_args(const char* op, const at::Tensor& q, const at::Tensor& codes, const at::Tensor& centroids, int64_t n_rows) {
  need(q, "q", at::kFloat, 2);
  need(centroids, "centroids", at::kFloat, 3);
  const int64_t dim = q.size(1), M = centroids.size(0);
  TORCH_CHECK(q.is_contiguous() && centroids.is_contiguous() && centroids.size(1) == 256 && M > 0 && dim % M == 0 && centroids.size(2) == dim / M && n_rows >= 0,
              op, ": q [Q,D] contiguous, centroids [M,256,D/M] contiguous with D % M == 0, n_rows >= 0");
  return tiled_rows(codes, at::kByte, n_rows, (M + 15) / 16 * 16,
                    (std::string(op) + ": codes must be the 1-D blocked uint8 codes of n_rows rows (whole 128-row blocks)").c_str());
}

// lrx_pq_ip_search.  Returns (D, I).
std::tuple<at::Tensor, at::Tensor> pq_ip_topk(const at::Tensor& q, const at::Tensor& codes, const at::Tensor& centroids, int64_t n_rows, int64_t k,
                                              int64_t id_base, const c10::optional<at::Tensor>& row_map) {
  DevGuard guard(q.device());
  void* cb = pq_args("pq_ip_topk", q, codes, centroids, n_rows);
  const int64_t dim = q.size(1), M = centroids.size(0);
  const int64_t* rm = row_map_ptr(row_map, n_rows, "pq_ip_topk: row_map int64 [>= n_rows] contiguous");
  TopK o = topk_out(q, k);
  const size_t wsb = lrx_pq_ip_workspace_bytes(n_rows, (int32_t)dim, (int32_t)M, (int32_t)q.size(0), (int32_t)k);
  at::Tensor ws = bytes((int64_t)wsb, q);
  lrx_check(lrx_pq_ip_search(cb, n_rows, centroids.data_ptr<float>(), (int32_t)dim, (int32_t)M, q.data_ptr<float>(), (int32_t)q.size(0), (int32_t)k, id_base,
                             o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), rm, ws.data_ptr(), wsb, 0, cur_stream()),
            "pq_ip_topk");
  return {o.d, o.i};
}

// 8-bit scalar-quantised index (lrx_sq8_ip_search): codes = the 1-D tiled uint8 codes (include/lrx.h, whole 128-row blocks) of n_rows rows,
// trained = vmin ++ vdiff fp32: 2 D floats (QT_8bit) or 2 (QT_8bit_uniform).  Returns (D, I).
std::tuple<at::Tensor, at::Tensor> sq8_ip_topk(const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& trained, int64_t k,
                                               int64_t id_base, const c10::optional<at::Tensor>& row_map) {
  DevGuard guard(q.device());
  need(q, "q", at::kFloat, 2);
  need(trained, "trained", at::kFloat, 1);
  const int64_t dim = q.size(1);
  TORCH_CHECK(q.is_contiguous() && trained.is_contiguous() && dim > 0 && dim % 64 == 0 && (trained.numel() == 2 * dim || trained.numel() == 2) && n_rows >= 0,
              "sq8_ip_topk: q [Q,D] contiguous with D % 64 == 0, trained [2 D] (QT_8bit) or [2] (QT_8bit_uniform), n_rows >= 0");
  const int32_t qtype = trained.numel() == 2 ? 2 : 0;
  void* cb = tiled_rows(codes, at::kByte, n_rows, dim, "sq8_ip_topk: codes must be the 1-D tiled uint8 codes of n_rows rows (whole 128-row blocks)");
  const int64_t* rm = row_map_ptr(row_map, n_rows, "sq8_ip_topk: row_map int64 [>= n_rows] contiguous");
  TopK o = topk_out(q, k);
  const size_t wsb = lrx_sq8_ip_workspace_bytes(n_rows, (int32_t)dim, (int32_t)q.size(0), (int32_t)k);
  at::Tensor ws = bytes((int64_t)wsb, q);
  lrx_check(lrx_sq8_ip_search(cb, n_rows, trained.data_ptr<float>(), (int32_t)dim, qtype, q.data_ptr<float>(), (int32_t)q.size(0), (int32_t)k, id_base,
                              o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), rm, ws.data_ptr(), wsb, 0, cur_stream()),
            "sq8_ip_topk");
  return {o.d, o.i};
}

// The store and queries of the impact index (impact_topk and impact_range_search; `op` names the one): postings int32 [nnz, 2] = {row, weight}
// grouped by term, ascending row inside a term; term_off int64 [n_terms + 1]; the queries in CSR form, q_off int32 [Q + 1], q_term / q_cnt
// int32 [q_off[Q]] (include/lrx.h) -> Q.  Reads q_off[Q] back to the host once (the CSR is checked against its arrays); no_capture: the op
// reads its result length back too, so it is refused under graph capture here, before that first read.
int64_t impact_args(const char* op, const at::Tensor& postings, const at::Tensor& term_off, int64_t n_rows, const at::Tensor& q_off, const at::Tensor& q_term,
                    const at::Tensor& q_cnt, bool no_capture) {
  need(postings, "postings", at::kInt, 2);
  need(term_off, "term_off", at::kLong, 1);
  need(q_off, "q_off", at::kInt, 1);
  need(q_term, "q_term", at::kInt, 1);
  need(q_cnt, "q_cnt", at::kInt, 1);
  TORCH_CHECK(postings.is_contiguous() && postings.size(1) == 2 && term_off.numel() >= 1 && q_off.numel() >= 1 && q_term.numel() == q_cnt.numel() && n_rows >= 0,
              op, ": postings int32 [nnz,2] contiguous, term_off int64 [T+1], q_off int32 [Q+1], q_term / q_cnt int32 of one length, n_rows >= 0");
  TORCH_CHECK(!no_capture || c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None, op,
              " under graph capture: the result length is read back to the host");
  const int64_t Q = q_off.numel() - 1;
  TORCH_CHECK(q_off[Q].item<int32_t>() == q_term.numel(), op, ": q_off[Q] must equal the length of q_term");
  return Q;
}

// lrx_impact_search.  The overflow refusal of the contract is the caller's (ImpactIndex.search makes it).  Returns (D, I).
std::tuple<at::Tensor, at::Tensor> impact_topk(const at::Tensor& postings, const at::Tensor& term_off, int64_t n_rows, const at::Tensor& q_off,
                                               const at::Tensor& q_term, const at::Tensor& q_cnt, int64_t k, int64_t id_base,
                                               const c10::optional<at::Tensor>& row_map, int64_t window_rows) {
  DevGuard guard(postings.device());
  const int64_t Q = impact_args("impact_topk", postings, term_off, n_rows, q_off, q_term, q_cnt, false);
  const int64_t* rm = row_map_ptr(row_map, n_rows, "impact_topk: row_map int64 [>= n_rows] contiguous");
  const auto f32 = postings.options().dtype(at::kFloat);
  at::Tensor d = at::empty({Q, k}, f32), i = at::empty({Q, k}, f32.dtype(at::kLong));
  const size_t wsb = lrx_impact_workspace_bytes(n_rows, (int32_t)Q, (int32_t)k);
  at::Tensor ws = bytes((int64_t)wsb, postings);
  lrx_check(lrx_impact_search(postings.data_ptr(), term_off.data_ptr<int64_t>(), (int32_t)(term_off.numel() - 1), n_rows, q_off.data_ptr<int32_t>(),
                              q_term.data_ptr<int32_t>(), q_cnt.data_ptr<int32_t>(), (int32_t)Q, (int32_t)k, id_base, d.data_ptr<float>(),
                              i.data_ptr<int64_t>(), rm, ws.data_ptr(), wsb, (int32_t)window_rows, cur_stream()),
            "impact_topk");
  return {d, i};
}

// Binary flat index (lrx_binary_ip_search / lrx_binary_hamming_search): codes = the 1-D blocked uint8 codes (include/lrx.h, whole 128-row blocks) of
// n_rows rows of q.size(1) bits; threshold: None (0), one element, or [D].  rerank: (D fp32, I) of the float rerank of the Hamming top-binary_k;
// else (D int32, I) of the Hamming top-k.
std::tuple<at::Tensor, at::Tensor> binary_topk(const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, int64_t k, int64_t binary_k, bool rerank,
                                               const c10::optional<at::Tensor>& threshold, int64_t id_base, const c10::optional<at::Tensor>& row_map) {
  DevGuard guard(q.device());
  need(q, "q", at::kFloat, 2);
  const int64_t dim = q.size(1);
  TORCH_CHECK(q.is_contiguous() && dim > 0 && dim % 8 == 0 && n_rows >= 0, "binary_topk: q [Q,D] contiguous with D % 8 == 0, n_rows >= 0");
  void* cb = tiled_rows(codes, at::kByte, n_rows, (dim + 127) / 128 * 16, "binary_topk: codes must be the 1-D blocked uint8 codes of n_rows rows (whole 128-row blocks)");
  const int64_t* rm = row_map_ptr(row_map, n_rows, "binary_topk: row_map int64 [>= n_rows] contiguous");
  float thr = 0.f;
  const float* thr_vec = nullptr;
  at::Tensor tv;
  if (threshold.has_value()) {
    TORCH_CHECK(threshold->numel() == 1 || threshold->numel() == dim, "binary_topk: threshold must hold 1 or D values");
    if (threshold->numel() == 1) {
      thr = threshold->item<float>();
    } else {
      tv = threshold->to(q.options()).contiguous();
      thr_vec = tv.data_ptr<float>();
    }
  }
  TopK o = topk_out(q, k);
  const size_t wsb = lrx_binary_workspace_bytes(n_rows, (int32_t)dim, (int32_t)q.size(0), (int32_t)binary_k);
  at::Tensor ws = bytes((int64_t)wsb, q);
  if (rerank) {
    lrx_check(lrx_binary_ip_search(cb, n_rows, (int32_t)dim, q.data_ptr<float>(), (int32_t)q.size(0), thr, thr_vec, (int32_t)k, (int32_t)binary_k, id_base,
                                   o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), rm, ws.data_ptr(), wsb, 0, cur_stream()),
              "binary_topk");
    return {o.d, o.i};
  }
  at::Tensor dist = at::empty({q.size(0), k}, q.options().dtype(at::kInt));
  lrx_check(lrx_binary_hamming_search(cb, n_rows, (int32_t)dim, q.data_ptr<float>(), (int32_t)q.size(0), thr, thr_vec, (int32_t)k, id_base,
                                      dist.data_ptr<int32_t>(), o.i.data_ptr<int64_t>(), rm, ws.data_ptr(), wsb, 0, cur_stream()),
            "binary_topk");
  return {dist, o.i};
}

// Range search (lrx_flat_ip_range_search): (lims [Q+1], D [lims[Q]], I [lims[Q]]).
std::tuple<at::Tensor, at::Tensor, at::Tensor> flat_ip_range_search(const at::Tensor& q, const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow,
                                                                    const at::Tensor& row_bounds, double radius, int64_t id_base) {
  DevGuard guard(q.device());
  void* xb = flat_bounded_args("flat_ip_range_search", q, x, x_shadow, row_bounds);
  const int64_t Q = q.size(0);
  const size_t wsb = lrx_flat_ip_range_workspace_bytes(x.size(0), (int32_t)x.size(1), (int32_t)Q, x_shadow.has_value() ? 1 : 0);
  at::Tensor ws = bytes((int64_t)wsb, q);
  return range_result(q, Q, "flat_ip_range_search", [&](int64_t* lims, float* d, int64_t* i, int64_t cap) {
    return lrx_flat_ip_range_search(x.data_ptr<float>(), x.size(0), x.size(0) ? x.stride(0) : x.size(1), (int32_t)x.size(1), xb, row_bounds.data_ptr<float>(),
                                    q.data_ptr<float>(), (int32_t)Q, (float)radius, id_base, lims, d, i, cap, ws.data_ptr(), wsb, cur_stream());
  });
}

// Range search over the quantised and sparse indexes: the result protocol is range_result's (above flat_ip_range_search).
std::tuple<at::Tensor, at::Tensor, at::Tensor> sq_fp16_ip_range_search(const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& row_bounds,
                                                                       double radius, int64_t id_base) {
  DevGuard guard(q.device());
  void* cb = sq_fp16_args("sq_fp16_ip_range_search", q, codes, n_rows, row_bounds);
  const int64_t dim = q.size(1), Q = q.size(0);
  const size_t wsb = lrx_sq_fp16_ip_range_workspace_bytes(n_rows, (int32_t)dim, (int32_t)Q);
  at::Tensor ws = bytes((int64_t)wsb, q);
  return range_result(q, Q, "sq_fp16_ip_range_search", [&](int64_t* lims, float* d, int64_t* i, int64_t cap) {
    return lrx_sq_fp16_ip_range_search(cb, n_rows, (int32_t)dim, row_bounds.data_ptr<float>(), q.data_ptr<float>(), (int32_t)Q, (float)radius, id_base, lims, d, i,
                                       cap, ws.data_ptr(), wsb, cur_stream());
  });
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> pq_ip_range_search(const at::Tensor& q, const at::Tensor& codes, const at::Tensor& centroids, int64_t n_rows,
                                                                  double radius, int64_t id_base, int64_t row_chunk) {
  DevGuard guard(q.device());
  void* cb = pq_args("pq_ip_range_search", q, codes, centroids, n_rows);
  const int64_t dim = q.size(1), M = centroids.size(0), Q = q.size(0);
  const size_t wsb = lrx_pq_ip_range_workspace_bytes(n_rows, (int32_t)dim, (int32_t)M, (int32_t)Q, row_chunk);
  at::Tensor ws = bytes((int64_t)wsb, q);
  return range_result(q, Q, "pq_ip_range_search", [&](int64_t* lims, float* d, int64_t* i, int64_t cap) {
    return lrx_pq_ip_range_search(cb, n_rows, centroids.data_ptr<float>(), (int32_t)dim, (int32_t)M, q.data_ptr<float>(), (int32_t)Q, (float)radius, id_base, lims,
                                  d, i, cap, ws.data_ptr(), wsb, cur_stream(), row_chunk);
  });
}

// (the overflow refusal of the contract is the caller's, as for impact_topk: ImpactIndex.range_search makes it)
std::tuple<at::Tensor, at::Tensor, at::Tensor> impact_range_search(const at::Tensor& postings, const at::Tensor& term_off, int64_t n_rows, const at::Tensor& q_off,
                                                                   const at::Tensor& q_term, const at::Tensor& q_cnt, double radius, int64_t id_base,
                                                                   int64_t window_rows, int64_t row_chunk) {
  DevGuard guard(postings.device());
  const int64_t Q = impact_args("impact_range_search", postings, term_off, n_rows, q_off, q_term, q_cnt, true);
  const size_t wsb = lrx_range_impact_workspace_bytes(n_rows, (int32_t)Q, row_chunk);
  at::Tensor ws = bytes((int64_t)wsb, postings);
  return range_result(postings, Q, "impact_range_search", [&](int64_t* lims, float* d, int64_t* i, int64_t cap) {
    return lrx_range_impact_search(postings.data_ptr(), term_off.data_ptr<int64_t>(), (int32_t)(term_off.numel() - 1), n_rows, q_off.data_ptr<int32_t>(),
                                   q_term.data_ptr<int32_t>(), q_cnt.data_ptr<int32_t>(), (int32_t)Q, (float)radius, id_base, lims, d, i, cap, ws.data_ptr(), wsb,
                                   (int32_t)window_rows, cur_stream(), row_chunk);
  });
}

// Quantise + compact to ragged CSR (lrx_sparse_csr_count / lrx_sparse_csr_fill): reps fp32 [B, V] (rows may be strided) -> (row_off int64 [B + 1],
// terms int32 [row_off[B]], weights int32 [row_off[B]]).  The exclusive scan between the two launches is at::cumsum; row_off[B] is read back to
// the host once to size the outputs, so the op is refused under graph capture before anything is launched.
std::tuple<at::Tensor, at::Tensor, at::Tensor> sparse_compact_csr(const at::Tensor& reps, int64_t quantization_factor, bool empty_marker) {
  DevGuard guard(reps.device());
  need(reps, "reps", at::kFloat, 2);
  TORCH_CHECK(c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None,
              "sparse_compact_csr under graph capture: the result length is read back to the host");
  const int64_t B = reps.size(0), V = reps.size(1);
  TORCH_CHECK(V > 0 && B < (int64_t(1) << 31) && quantization_factor > 0 && quantization_factor < (int64_t(1) << 31),
              "sparse_compact_csr: reps [B, V > 0], 0 < quantization_factor < 2^31");
  const int64_t ld = B ? reps.stride(0) : V;
  at::Tensor counts = at::empty({B}, reps.options().dtype(at::kInt));
  lrx_check(lrx_sparse_csr_count(reps.data_ptr<float>(), (int32_t)B, (int32_t)V, ld, (int32_t)quantization_factor, empty_marker ? 1 : 0,
                                 counts.data_ptr<int32_t>(), cur_stream()),
            "sparse_compact_csr");
  at::Tensor row_off = at::zeros({B + 1}, reps.options().dtype(at::kLong));
  if (B) row_off.narrow(0, 1, B).copy_(at::cumsum(counts, 0, at::kLong));
  const int64_t nnz = B ? row_off[B].item<int64_t>() : 0;
  at::Tensor terms = at::empty({nnz}, counts.options()), weights = at::empty({nnz}, counts.options());
  lrx_check(lrx_sparse_csr_fill(reps.data_ptr<float>(), (int32_t)B, (int32_t)V, ld, (int32_t)quantization_factor, empty_marker ? 1 : 0,
                                row_off.data_ptr<int64_t>(), terms.data_ptr<int32_t>(), weights.data_ptr<int32_t>(), cur_stream()),
            "sparse_compact_csr");
  return {row_off, terms, weights};
}

// Exact fp32 linear map (lrx_linear_transform): x [n, d_in] (rows may be strided), A [d_out, d_in] contiguous, b [d_out] or None -> [n, d_out].
at::Tensor linear_transform(const at::Tensor& x, const at::Tensor& A, const c10::optional<at::Tensor>& b) {
  DevGuard guard(x.device());
  need(x, "x", at::kFloat, 2);
  need(A, "A", at::kFloat, 2);
  TORCH_CHECK(A.is_contiguous() && A.size(1) == x.size(1), "linear_transform: x [n, d_in], A [d_out, d_in] contiguous");
  const float* bp = nullptr;
  if (b.has_value()) {
    need(*b, "b", at::kFloat, 1);
    TORCH_CHECK(b->is_contiguous() && b->numel() == A.size(0), "linear_transform: b [d_out] contiguous");
    bp = b->data_ptr<float>();
  }
  at::Tensor out = at::empty({x.size(0), A.size(0)}, x.options());
  lrx_check(lrx_linear_transform(x.data_ptr<float>(), x.size(0), x.size(0) > 1 ? x.stride(0) : x.size(1), A.data_ptr<float>(), bp, (int32_t)x.size(1),
                                 (int32_t)A.size(0), out.data_ptr<float>(), A.size(0), cur_stream()),
            "linear_transform");
  return out;
}

}  // namespace

TORCH_LIBRARY(lrx, m) {
  m.def("encode_packed(Tensor ids, Tensor cu_seqlens, int max_seqlen, int weights, Tensor(a!) out, int mrl_dim=0, bool normalize=True, "
        "Tensor(b!)? shadow=None, int shadow_row0=0, Tensor(c!)? row_bounds=None) -> ()");
  m.def("rmsnorm(Tensor x, Tensor w, float eps) -> Tensor");
  m.def("rope_qkv_gemm(Tensor a, Tensor wqkv, Tensor? bias, Tensor positions, Tensor cos, Tensor sin, int num_q_heads, int num_kv_heads, int head_dim) -> Tensor");
  m.def("attn_varlen(Tensor qkv, Tensor cu_seqlens, int max_seqlen, int num_q_heads, int num_kv_heads, int head_dim) -> Tensor");
  m.def("swiglu_gemm(Tensor a, Tensor wgu) -> Tensor");
  m.def("embedding_bag_mean(Tensor table, Tensor ids, Tensor offsets, int padding_idx=-1, int out_dim=0, bool normalize=True) -> Tensor");
  m.def("flat_ip_topk(Tensor q, Tensor x, int k, int id_base=0, Tensor? row_bounds=None) -> (Tensor, Tensor)");
  m.def("flat_ip_topk_bounded(Tensor q, Tensor x, Tensor? x_shadow, Tensor row_bounds, int k, int id_base=0, int flags=0) -> (Tensor, Tensor)");
  m.def("flat_ip_topk_bounded_wire(Tensor q, Tensor x, Tensor? x_shadow, Tensor row_bounds, int k, int id_base=0, Tensor? row_map=None, int flags=0) -> (Tensor, Tensor, Tensor)");
  m.def("merge_topk_packed(Tensor words) -> (Tensor, Tensor)");
  m.def("shard_commit_rows(Tensor x, Tensor(a!)? x_shadow, Tensor(b!) row_bounds, int row0=0) -> ()");
  m.def("merge_topk(Tensor d_parts, Tensor i_parts) -> (Tensor, Tensor)");
  m.def("flat_ip_range_search(Tensor q, Tensor x, Tensor? x_shadow, Tensor row_bounds, float radius, int id_base=0) -> (Tensor, Tensor, Tensor)");
  m.def("sq_fp16_ip_topk(Tensor q, Tensor codes, int n_rows, Tensor row_bounds, int k, int id_base=0, Tensor? row_map=None, int flags=0) -> (Tensor, Tensor, Tensor)");
  m.def("flat_ip_rerank(Tensor q, Tensor x, Tensor cand, int k, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("sq_fp16_ip_rerank(Tensor q, Tensor codes, int n_rows, Tensor cand, int k, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("ivf_flat_ip_range_search(Tensor q, Tensor x, Tensor list_off, Tensor? row_ids, Tensor probes, float radius, int max_scan_rows, int id_base=0, "
        "Tensor? row_map=None) -> (Tensor, Tensor, Tensor)");
  m.def("ivf_flat_ip_range_search_sel(Tensor q, Tensor x, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? sel, float radius, "
        "int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor, Tensor)");
  m.def("ivf_pq_ip_range_search(Tensor q, Tensor codes, Tensor pq_centroids, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? probe_scores, "
        "bool by_residual, float radius, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor, Tensor)");
  m.def("ivf_pq_ip_range_search_sel(Tensor q, Tensor codes, Tensor pq_centroids, Tensor list_off, Tensor? row_ids, Tensor probes, "
        "Tensor? probe_scores, Tensor? sel, bool by_residual, float radius, int max_scan_rows, int id_base=0, "
        "Tensor? row_map=None) -> (Tensor, Tensor, Tensor)");
  m.def("ivf_sq_fp16_ip_range_search(Tensor q, Tensor codes, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? probe_scores, bool by_residual, "
        "float radius, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor, Tensor)");
  m.def("ivf_sq_fp16_ip_range_search_sel(Tensor q, Tensor codes, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? probe_scores, "
        "Tensor? sel, bool by_residual, float radius, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor, Tensor)");
  m.def("ivf_sq8_ip_range_search(Tensor q, Tensor codes, Tensor trained, int qtype, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? probe_scores, "
        "bool by_residual, float radius, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor, Tensor)");
  m.def("ivf_sq8_ip_range_search_sel(Tensor q, Tensor codes, Tensor trained, int qtype, Tensor list_off, Tensor? row_ids, Tensor probes, "
        "Tensor? probe_scores, Tensor? sel, bool by_residual, float radius, int max_scan_rows, int id_base=0, "
        "Tensor? row_map=None) -> (Tensor, Tensor, Tensor)");
  m.def("ivf_flat_ip_topk(Tensor q, Tensor x, Tensor list_off, Tensor? row_ids, Tensor probes, int k, int max_scan_rows, int id_base=0, "
        "Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("ivf_flat_ip_topk_sel(Tensor q, Tensor x, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? sel, int k, int max_scan_rows, "
        "int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("ivf_pq_ip_topk(Tensor q, Tensor codes, Tensor pq_centroids, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? probe_scores, "
        "bool by_residual, int k, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("ivf_pq_ip_topk_sel(Tensor q, Tensor codes, Tensor pq_centroids, Tensor list_off, Tensor? row_ids, Tensor probes, "
        "Tensor? probe_scores, Tensor? sel, bool by_residual, int k, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, "
        "Tensor)");
  m.def("ivf_sq_fp16_ip_topk(Tensor q, Tensor codes, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? probe_scores, bool by_residual, int k, "
        "int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("ivf_sq_fp16_ip_topk_sel(Tensor q, Tensor codes, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? probe_scores, "
        "Tensor? sel, bool by_residual, int k, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("ivf_sq8_ip_topk(Tensor q, Tensor codes, Tensor trained, int qtype, Tensor list_off, Tensor? row_ids, Tensor probes, Tensor? probe_scores, "
        "bool by_residual, int k, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("ivf_sq8_ip_topk_sel(Tensor q, Tensor codes, Tensor trained, int qtype, Tensor list_off, Tensor? row_ids, Tensor probes, "
        "Tensor? probe_scores, Tensor? sel, bool by_residual, int k, int max_scan_rows, int id_base=0, Tensor? row_map=None) -> (Tensor, "
        "Tensor)");
  m.def("pq_ip_topk(Tensor q, Tensor codes, Tensor centroids, int n_rows, int k, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("sq8_ip_topk(Tensor q, Tensor codes, int n_rows, Tensor trained, int k, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
  m.def("impact_topk(Tensor postings, Tensor term_off, int n_rows, Tensor q_off, Tensor q_term, Tensor q_cnt, int k, int id_base=0, Tensor? row_map=None, "
        "int window_rows=0) -> (Tensor, Tensor)");
  m.def("sparse_compact_csr(Tensor reps, int quantization_factor=100, bool empty_marker=True) -> (Tensor, Tensor, Tensor)");
  m.def("sq_fp16_ip_range_search(Tensor q, Tensor codes, int n_rows, Tensor row_bounds, float radius, int id_base=0) -> (Tensor, Tensor, Tensor)");
  m.def("pq_ip_range_search(Tensor q, Tensor codes, Tensor centroids, int n_rows, float radius, int id_base=0, int row_chunk=0) -> (Tensor, Tensor, Tensor)");
  m.def("impact_range_search(Tensor postings, Tensor term_off, int n_rows, Tensor q_off, Tensor q_term, Tensor q_cnt, float radius, int id_base=0, "
        "int window_rows=0, int row_chunk=0) -> (Tensor, Tensor, Tensor)");
  m.def("linear_transform(Tensor x, Tensor A, Tensor? b=None) -> Tensor");
  m.def("binary_topk(Tensor q, Tensor codes, int n_rows, int k, int binary_k=1000, bool rerank=True, Tensor? threshold=None, int id_base=0, Tensor? row_map=None) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(lrx, CUDA, m) {   // (the ROCm build of PyTorch dispatches HIP tensors under the CUDA key)
  m.impl("encode_packed", &encode_packed);
  m.impl("rmsnorm", &rmsnorm);
  m.impl("rope_qkv_gemm", &rope_qkv_gemm);
  m.impl("attn_varlen", &attn_varlen);
  m.impl("swiglu_gemm", &swiglu_gemm);
  m.impl("embedding_bag_mean", &embedding_bag_mean);
  m.impl("flat_ip_topk", &flat_ip_topk);
  m.impl("flat_ip_topk_bounded", &flat_ip_topk_bounded);
  m.impl("flat_ip_topk_bounded_wire", &flat_ip_topk_bounded_wire);
  m.impl("merge_topk_packed", &merge_topk_packed);
  m.impl("shard_commit_rows", &shard_commit_rows);
  m.impl("merge_topk", &merge_topk);
  m.impl("flat_ip_range_search", &flat_ip_range_search);
  m.impl("sq_fp16_ip_topk", &sq_fp16_ip_topk);
  m.impl("flat_ip_rerank", &flat_ip_rerank);
  m.impl("sq_fp16_ip_rerank", &sq_fp16_ip_rerank);
  m.impl("ivf_flat_ip_range_search", &IvfOp<IvfFlat, double>::plain);
  m.impl("ivf_flat_ip_range_search_sel", &IvfOp<IvfFlat, double>::with_sel);
  m.impl("ivf_pq_ip_range_search", &IvfOp<IvfPq, double>::plain);
  m.impl("ivf_pq_ip_range_search_sel", &IvfOp<IvfPq, double>::with_sel);
  m.impl("ivf_sq_fp16_ip_range_search", &IvfOp<IvfSqFp16, double>::plain);
  m.impl("ivf_sq_fp16_ip_range_search_sel", &IvfOp<IvfSqFp16, double>::with_sel);
  m.impl("ivf_sq8_ip_range_search", &IvfOp<IvfSq8, double>::plain);
  m.impl("ivf_sq8_ip_range_search_sel", &IvfOp<IvfSq8, double>::with_sel);
  m.impl("ivf_flat_ip_topk", &IvfOp<IvfFlat, int64_t>::plain);
  m.impl("ivf_flat_ip_topk_sel", &IvfOp<IvfFlat, int64_t>::with_sel);
  m.impl("ivf_pq_ip_topk", &IvfOp<IvfPq, int64_t>::plain);
  m.impl("ivf_pq_ip_topk_sel", &IvfOp<IvfPq, int64_t>::with_sel);
  m.impl("ivf_sq_fp16_ip_topk", &IvfOp<IvfSqFp16, int64_t>::plain);
  m.impl("ivf_sq_fp16_ip_topk_sel", &IvfOp<IvfSqFp16, int64_t>::with_sel);
  m.impl("ivf_sq8_ip_topk", &IvfOp<IvfSq8, int64_t>::plain);
  m.impl("ivf_sq8_ip_topk_sel", &IvfOp<IvfSq8, int64_t>::with_sel);
  m.impl("pq_ip_topk", &pq_ip_topk);
  m.impl("sq8_ip_topk", &sq8_ip_topk);
  m.impl("impact_topk", &impact_topk);
  m.impl("binary_topk", &binary_topk);
  m.impl("sparse_compact_csr", &sparse_compact_csr);
  m.impl("sq_fp16_ip_range_search", &sq_fp16_ip_range_search);
  m.impl("pq_ip_range_search", &pq_ip_range_search);
  m.impl("impact_range_search", &impact_range_search);
  m.impl("linear_transform", &linear_transform);
}
