// torch.ops.lrx.*: the PyTorch-ROCm custom-op binding of the C ABI in include/lrx.h (last row).
// A thin layer: tensors in, the current HIP stream, workspaces from PyTorch's caching allocator, errors -> TORCH_CHECK
// (Python RuntimeError).  Every op forwards to exactly one lrx_* entry point of liblrx.so; no arithmetic lives here.
// What the layer decides is which pointer, leading dimension and int32 each entry gets: the ARGUMENT CONTRACT below (struct Op) says what
// it admits, every op checks its arguments through it before its first allocation, and tests/test_gpu_torch_op_contract.py holds it to that.
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

// ---- the argument contract --------------------------------------------------------------------------------------------------------
// (lightretriever_amd/torch_ops.py states it for callers; tests/torch_op_cases.py annotates every argument of every op with it)
//   * every tensor of a call lives on ONE device, the device of the op's first tensor; a CPU tensor or one of another device is refused;
//   * dtype and rank are exact; a tensor is contiguous unless it is documented as "rows may be strided" (kRows): 2-D, unit column stride, a
//     row stride >= its width -- and a single row has no stride: its leading dimension is its width (ld());
//   * data operands that kernels read or write 16 bytes at a time (kVec: fp32 / 16-bit / uint8 rows, codes, tables) have a 16-byte aligned
//     base; `ld % 4 == 0` stays with the library.  Index arrays (int32 / int64) need only their natural alignment;
//   * an optional tensor that is given passes the same checks as a required one (Op::opt);
//   * an integer that the C ABI takes as int32 is range-checked (Op::i32) BEFORE anything is allocated or launched.
// Every refusal is a TORCH_CHECK (RuntimeError) that names the op and the argument.
using OptTensor = c10::optional<at::Tensor>;
enum : int { kRows = 1, kVec = 2 };

// the leading dimension of a rows-may-be-strided operand
int64_t ld(const at::Tensor& t) { return t.size(0) > 1 ? t.stride(0) : t.size(1); }

// One call of an op: its name for every message, the device of its first tensor (made current for the call's lifetime) and the checks above.
struct Op {
  const char* name;
  c10::Device dev;
  DevGuard guard;
  Op(const char* name, const at::Tensor& first, const char* arg) : name(name), dev(first.device()) {
    TORCH_CHECK(first.is_cuda(), name, ": ", arg, " must be a device tensor, got one on ", dev);
    guard.set_device(dev);
  }
  void need(const at::Tensor& t, const char* arg, at::ScalarType dt, int64_t dim, int flags = 0) const {
    TORCH_CHECK(t.is_cuda(), name, ": ", arg, " must be a device tensor, got one on ", t.device());
    TORCH_CHECK(t.device() == dev, name, ": ", arg, " is on ", t.device(), ", the op's first tensor on ", dev, ": all tensors of a call must share a device");
    TORCH_CHECK(t.scalar_type() == dt, name, ": ", arg, " must be ", dt, ", got ", t.scalar_type());
    TORCH_CHECK(t.dim() == dim, name, ": ", arg, " must have ", dim, " dimensions, got ", t.dim());
    if ((flags & kRows) && dim == 2) {
      TORCH_CHECK(t.is_contiguous() || (t.stride(1) == 1 && t.stride(0) >= t.size(1)), name, ": ", arg,
                  " must have unit column stride and a row stride >= its width (rows may be strided)");
    } else {
      TORCH_CHECK(t.is_contiguous(), name, ": ", arg, " must be contiguous");
    }
    TORCH_CHECK(!(flags & kVec) || t.numel() == 0 || (uintptr_t)t.data_ptr() % 16 == 0, name, ": ", arg, " must start at a 16-byte aligned address");
  }
  // an optional tensor: absent (None / undefined) -> false, else need() and true
  bool opt(const OptTensor& t, const char* arg, at::ScalarType dt, int64_t dim, int flags = 0) const {
    if (!t.has_value() || !t->defined()) return false;
    need(*t, arg, dt, dim, flags);
    return true;
  }
  // an integer the C ABI takes as int32: lo <= v <= hi <= INT32_MAX
  int32_t i32(int64_t v, const char* arg, int64_t lo, int64_t hi = INT32_MAX) const {
    TORCH_CHECK(lo <= v && v <= hi, name, ": ", arg, " = ", v, " is outside [", lo, ", ", hi, "]");
    return (int32_t)v;
  }
  void check(int rc) const { lrx_check(rc, name); }
};
constexpr int64_t kMaxK = 2048;   // include/lrx.h: 1 <= k <= 2048 for every top-k entry
constexpr int64_t kMaxHeads = 65536, kMaxHeadDim = 1024;   // far above any model; keeps (nq + 2 nkv) * d inside int64

at::Tensor bytes(int64_t n, const at::Tensor& like) { return at::empty({n}, like.options().dtype(at::kByte)); }

// ---- index ops: shared argument checks and outputs --------------------------------------------------------------------------------
// an optional 1-D tiled buffer of `dt` elements (include/lrx.h: whole 128-row blocks) that must hold rows [0, n_rows) of `width` columns
// -> its address, or null when absent; `arg` names it and `what` says what it is
void* tiled_rows(const Op& op, const OptTensor& t, const char* arg, at::ScalarType dt, int64_t n_rows, int64_t width, const char* what) {
  if (!op.opt(t, arg, dt, 1, kVec)) return nullptr;
  TORCH_CHECK(n_rows >= 0 && t->numel() >= ((n_rows + 127) / 128) * 128 * width, op.name, ": ", arg, " must be ", what, " (whole 128-row blocks), got ",
              t->numel(), " elements for ", n_rows, " rows");
  return t->data_ptr();
}

// an optional int64 map of >= n_rows local rows -> its address, or null when absent
const int64_t* row_map_ptr(const Op& op, const OptTensor& row_map, int64_t n_rows) {
  if (!op.opt(row_map, "row_map", at::kLong, 1)) return nullptr;
  TORCH_CHECK(row_map->numel() >= n_rows, op.name, ": row_map int64 [>= ", n_rows, "] contiguous, got ", row_map->numel());
  return row_map->data_ptr<int64_t>();
}

// the two floats {max row norm, ...} of a shard (include/lrx.h), required or optional -> their address, or null when absent
float* row_bounds_ptr(const Op& op, const OptTensor& row_bounds) {
  if (!op.opt(row_bounds, "row_bounds", at::kFloat, 1)) return nullptr;
  TORCH_CHECK(row_bounds->numel() == 2, op.name, ": row_bounds [2], got ", row_bounds->numel(), " elements");
  return row_bounds->data_ptr<float>();
}

// the [Q, k] outputs of a top-k search over queries q: fp32 scores d, int64 ids i and, for the wire ops, the int64 exchange words w
// (k has passed Op::i32 by then)
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
  Op op("encode_packed", ids, "ids");
  op.need(ids, "ids", at::kInt, 1);
  op.need(cu_seqlens, "cu_seqlens", at::kInt, 1);
  op.need(out, "out", at::kFloat, 2, kRows | kVec);
  TORCH_CHECK(weights != 0, "encode_packed: null weights handle");
  const lrx_encoder_handle* h = (const lrx_encoder_handle*)weights;
  TORCH_CHECK(cu_seqlens.numel() >= 1, "encode_packed: cu_seqlens int32 [n_seqs + 1], got an empty tensor");
  const int32_t T = op.i32(ids.numel(), "ids (its length)", 0), B = op.i32(cu_seqlens.numel() - 1, "cu_seqlens (its length - 1)", 0);
  const int32_t msl = op.i32(max_seqlen, "max_seqlen", 1);
  const int32_t D = op.i32(mrl_dim, "mrl_dim", 0, h->cfg->hidden_size) > 0 ? (int32_t)mrl_dim : h->cfg->hidden_size;
  TORCH_CHECK(out.size(0) >= B && out.size(1) >= D, "encode_packed: out must be fp32 [>= n_seqs, >= mrl_dim], got [", out.size(0), ", ", out.size(1), "] for ", B,
              " sequences of ", D, " columns");
  void* sh = nullptr;
  // (the shadow's 16-bit format is the encoder's: fp16 or bf16, whichever the tensor says)
  TORCH_CHECK(!shadow.has_value() || !shadow->defined() || (shadow->dim() == 1 && shadow->element_size() == 2),
              "encode_packed: shadow must be the shard's 1-D tiled 16-bit shadow (include/lrx.h), got ", shadow->dim(), " dimensions of ", shadow->scalar_type());
  if (op.opt(shadow, "shadow", shadow.has_value() && shadow->defined() && shadow->scalar_type() == at::kBFloat16 ? at::kBFloat16 : at::kHalf, 1, kVec)) {
    TORCH_CHECK(D % 64 == 0 && D == out.size(1) && shadow_row0 >= 0 && shadow->numel() >= ((shadow_row0 + B + 127) / 128) * 128 * D,
                "encode_packed: shadow must be the shard's 1-D tiled 16-bit shadow (include/lrx.h), out its full-width rows from shadow_row0 on");
    sh = shadow->data_ptr();
  }
  float* rb = row_bounds_ptr(op, row_bounds);
  const size_t need_b = lrx_encode_workspace_bytes(h->cfg, T, B);
  at::Tensor ws = bytes((int64_t)need_b, ids);
  op.check(lrx_encode_packed_shard(h->cfg, h->w, ids.data_ptr<int32_t>(), cu_seqlens.data_ptr<int32_t>(), B, T, msl, out.data_ptr<float>(), ld(out), D,
                                   normalize ? 1 : 0, sh, shadow_row0, rb, ws.data_ptr(), need_b, cur_stream()));
}

// ---- unit kernels -------------------------------------------------------------------------------------------------------------------
at::Tensor rmsnorm(const at::Tensor& x, const at::Tensor& w, double eps) {
  Op op("rmsnorm", x, "x");
  op.need(x, "x", at::kBFloat16, 2, kVec);
  op.need(w, "w", at::kBFloat16, 1, kVec);
  TORCH_CHECK(w.numel() == x.size(1), "rmsnorm: x [rows, H] contiguous, w [H]");
  const int32_t rows = op.i32(x.size(0), "x (its rows)", 0), H = op.i32(x.size(1), "x (its width)", 0);
  at::Tensor y = at::empty(x.sizes(), x.options());
  op.check(lrx_rmsnorm(x.data_ptr(), w.data_ptr(), y.data_ptr(), rows, H, (float)eps, cur_stream()));
  return y;
}

at::Tensor rope_qkv_gemm(const at::Tensor& a, const at::Tensor& wqkv, const c10::optional<at::Tensor>& bias, const at::Tensor& positions,
                         const at::Tensor& cos, const at::Tensor& sin, int64_t num_q_heads, int64_t num_kv_heads, int64_t head_dim) {
  Op op("rope_qkv_gemm", a, "a");
  op.need(a, "a", at::kBFloat16, 2, kVec);
  op.need(wqkv, "wqkv", at::kBFloat16, 2, kVec);
  op.need(positions, "positions", at::kInt, 1);
  op.need(cos, "cos", at::kFloat, 2, kVec);
  op.need(sin, "sin", at::kFloat, 2, kVec);
  const int32_t nq = op.i32(num_q_heads, "num_q_heads", 1, kMaxHeads), nkv = op.i32(num_kv_heads, "num_kv_heads", 1, kMaxHeads), d = op.i32(head_dim, "head_dim", 2, kMaxHeadDim);
  const int32_t M = op.i32(a.size(0), "a (its rows)", 0), K = op.i32(a.size(1), "a (its width)", 0);
  TORCH_CHECK(wqkv.size(1) == K, "rope_qkv_gemm: a [M,K], wqkv [N,K] contiguous");
  TORCH_CHECK(wqkv.size(0) == ((int64_t)nq + 2 * (int64_t)nkv) * d, "rope_qkv_gemm: wqkv rows != (num_q_heads + 2 num_kv_heads) * head_dim");
  TORCH_CHECK(positions.numel() == M, "rope_qkv_gemm: positions int32 [M], one per row of a: got ", positions.numel(), " for ", M, " rows");
  TORCH_CHECK(cos.size(1) == d / 2 && sin.sizes() == cos.sizes(), "rope_qkv_gemm: cos and sin fp32 [max_positions, head_dim / 2] contiguous, got cos [",
              cos.size(0), ", ", cos.size(1), "], sin [", sin.size(0), ", ", sin.size(1), "] for head_dim ", d);
  const bool has_bias = op.opt(bias, "bias", at::kBFloat16, 1, kVec);
  TORCH_CHECK(!has_bias || bias->numel() == wqkv.size(0), "rope_qkv_gemm: bias bf16 [(num_q_heads + 2 num_kv_heads) * head_dim] contiguous");
  at::Tensor c = at::empty({a.size(0), wqkv.size(0)}, a.options().dtype(at::kHalf));   // fp16, q | k columns in rotary-pair order (include/lrx.h)
  op.check(lrx_gemm_qkv_rope(a.data_ptr(), wqkv.data_ptr(), c.data_ptr(), has_bias ? bias->data_ptr() : nullptr, positions.data_ptr<int32_t>(),
                             cos.data_ptr<float>(), sin.data_ptr<float>(), M, K, nq, nkv, d, cur_stream()));
  return c;
}

at::Tensor attn_varlen(const at::Tensor& qkv, const at::Tensor& cu_seqlens, int64_t max_seqlen, int64_t num_q_heads, int64_t num_kv_heads,
                       int64_t head_dim) {
  Op op("attn_varlen", qkv, "qkv");
  op.need(qkv, "qkv", at::kHalf, 2, kVec);
  op.need(cu_seqlens, "cu_seqlens", at::kInt, 1);
  const int32_t nq = op.i32(num_q_heads, "num_q_heads", 1, kMaxHeads), nkv = op.i32(num_kv_heads, "num_kv_heads", 1, kMaxHeads), d = op.i32(head_dim, "head_dim", 2, kMaxHeadDim);
  const int32_t msl = op.i32(max_seqlen, "max_seqlen", 1), T = op.i32(qkv.size(0), "qkv (its rows)", 0);
  TORCH_CHECK(cu_seqlens.numel() >= 1, "attn_varlen: cu_seqlens int32 [n_seqs + 1], got an empty tensor");
  const int32_t B = op.i32(cu_seqlens.numel() - 1, "cu_seqlens (its length - 1)", 0);
  TORCH_CHECK(qkv.size(1) == ((int64_t)nq + 2 * (int64_t)nkv) * d, "attn_varlen: qkv [T, (num_q_heads + 2 num_kv_heads) * head_dim] contiguous");
  at::Tensor out = at::empty({qkv.size(0), (int64_t)nq * d}, qkv.options().dtype(at::kBFloat16));
  op.check(lrx_attn_varlen_causal(qkv.data_ptr(), cu_seqlens.data_ptr<int32_t>(), B, T, msl, nq, nkv, d, out.data_ptr(), 0, cur_stream()));
  return out;
}

at::Tensor swiglu_gemm(const at::Tensor& a, const at::Tensor& wgu) {
  Op op("swiglu_gemm", a, "a");
  op.need(a, "a", at::kBFloat16, 2, kVec);
  op.need(wgu, "wgu", at::kBFloat16, 2, kVec);
  TORCH_CHECK(wgu.size(1) == a.size(1) && wgu.size(0) % 2 == 0, "swiglu_gemm: a [M,K], wgu [2I,K] contiguous");
  const int32_t M = op.i32(a.size(0), "a (its rows)", 0), N = op.i32(wgu.size(0), "wgu (its rows)", 0), K = op.i32(a.size(1), "a (its width)", 0);
  at::Tensor c = at::empty({a.size(0), wgu.size(0) / 2}, a.options());
  op.check(lrx_gemm_bf16_nt(a.data_ptr(), wgu.data_ptr(), c.data_ptr(), nullptr, nullptr, M, N, K, 2, cur_stream()));
  return c;
}

// ---- query side -------------------------------------------------------------------------------------------------------------------
at::Tensor embedding_bag_mean(const at::Tensor& table, const at::Tensor& ids, const at::Tensor& offsets, int64_t padding_idx, int64_t out_dim,
                              bool normalize) {
  Op op("embedding_bag_mean", table, "table");
  op.need(table, "table", at::kFloat, 2, kVec);
  op.need(ids, "ids", at::kLong, 1);
  op.need(offsets, "offsets", at::kLong, 1);
  const int32_t V = op.i32(table.size(0), "table (its rows)", 0), H = op.i32(table.size(1), "table (its width)", 0);
  const int32_t B = op.i32(offsets.numel(), "offsets (its length)", 0);
  const int32_t D = op.i32(out_dim, "out_dim", 0, H) > 0 ? (int32_t)out_dim : H;
  at::Tensor out = at::empty({offsets.numel(), (int64_t)D}, table.options());
  op.check(lrx_embedding_bag_mean(table.data_ptr<float>(), V, H, ids.data_ptr<int64_t>(), ids.numel(), offsets.data_ptr<int64_t>(), B, padding_idx,
                                  out.data_ptr<float>(), D, D, normalize ? 1 : 0, cur_stream()));
  return out;
}

// ---- index ----------------------------------------------------------------------------------------------------------------------
std::tuple<at::Tensor, at::Tensor> flat_ip_topk(const at::Tensor& q, const at::Tensor& x, int64_t k, int64_t id_base,
                                                const c10::optional<at::Tensor>& row_bounds) {
  Op op("flat_ip_topk", q, "q");
  op.need(q, "q", at::kFloat, 2, kVec);
  op.need(x, "x", at::kFloat, 2, kRows | kVec);
  TORCH_CHECK(q.size(1) == x.size(1), "flat_ip_topk: q [Q,D] contiguous, x [N,D]: got D = ", q.size(1), " and ", x.size(1));
  const int32_t D = op.i32(x.size(1), "x (its width)", 0), Q = op.i32(q.size(0), "q (its rows)", 0), k32 = op.i32(k, "k", 1);
  const float* rb = row_bounds_ptr(op, row_bounds);
  TopK o = topk_out(q, k);
  const size_t wsb = lrx_flat_ip_workspace_bytes(x.size(0), D, Q, k32);
  at::Tensor ws = bytes((int64_t)wsb, q);
  op.check(lrx_flat_ip_search(x.data_ptr<float>(), x.size(0), ld(x), D, rb, q.data_ptr<float>(), Q, k32, id_base, o.d.data_ptr<float>(),
                              o.i.data_ptr<int64_t>(), ws.data_ptr(), wsb, cur_stream()));
  return {o.d, o.i};
}

// The store of the bounded searches (flat_ip_topk_bounded, its wire sibling and flat_ip_range_search): x fp32 [N, D] rows (may be strided), their
// 1-D tiled fp16 shadow x_shadow (include/lrx.h; block 0 row 0 = x row 0) or None, row_bounds [2] -> the shadow's address, or null
void* flat_bounded_args(const Op& op, const at::Tensor& q, const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow, const at::Tensor& row_bounds) {
  op.need(q, "q", at::kFloat, 2, kVec);
  op.need(x, "x", at::kFloat, 2, kRows | kVec);
  row_bounds_ptr(op, row_bounds);
  TORCH_CHECK(q.size(1) == x.size(1), op.name, ": q [Q,D] contiguous, x [N,D], row_bounds [2]: got D = ", q.size(1), " and ", x.size(1));
  op.i32(x.size(1), "x (its width)", 0);
  op.i32(q.size(0), "q (its rows)", 0);
  return tiled_rows(op, x_shadow, "x_shadow", at::kHalf, x.size(0), x.size(1), "the 1-D tiled fp16 shadow of x");
}

// flags: LRX_SEARCH_FILTER_*
std::tuple<at::Tensor, at::Tensor> flat_ip_topk_bounded(const at::Tensor& q, const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow,
                                                        const at::Tensor& row_bounds, int64_t k, int64_t id_base, int64_t flags) {
  Op op("flat_ip_topk_bounded", q, "q");
  void* xb = flat_bounded_args(op, q, x, x_shadow, row_bounds);
  const int32_t D = (int32_t)x.size(1), Q = (int32_t)q.size(0), k32 = op.i32(k, "k", 1, kMaxK), fl = op.i32(flags, "flags", 0);
  TopK o = topk_out(q, k);
  const size_t wsb = lrx_flat_ip_bounded_workspace_bytes(x.size(0), D, Q, k32, fl);
  at::Tensor ws = bytes((int64_t)wsb, q);
  op.check(lrx_flat_ip_search_bounded(x.data_ptr<float>(), x.size(0), ld(x), D, xb, row_bounds.data_ptr<float>(), q.data_ptr<float>(), Q, k32, id_base,
                                      o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), ws.data_ptr(), wsb, fl, cur_stream()));
  return {o.d, o.i};
}

// The same search for one rank of a row-sharded index: also returns the [Q, k] int64 wire words of the exchange (lrx_pack_topk's format,
// row_map applied), written by the search's own last kernel -- all_gather_into_tensor them and hand the result to merge_topk_packed.
std::tuple<at::Tensor, at::Tensor, at::Tensor> flat_ip_topk_bounded_wire(const at::Tensor& q, const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow,
                                                                         const at::Tensor& row_bounds, int64_t k, int64_t id_base,
                                                                         const c10::optional<at::Tensor>& row_map, int64_t flags) {
  Op op("flat_ip_topk_bounded_wire", q, "q");
  void* xb = flat_bounded_args(op, q, x, x_shadow, row_bounds);
  const int64_t* rm = row_map_ptr(op, row_map, x.size(0));
  const int32_t D = (int32_t)x.size(1), Q = (int32_t)q.size(0), k32 = op.i32(k, "k", 1, kMaxK), fl = op.i32(flags, "flags", 0);
  TopK o = topk_out(q, k, true);
  const size_t wsb = lrx_flat_ip_bounded_workspace_bytes(x.size(0), D, Q, k32, fl);
  at::Tensor ws = bytes((int64_t)wsb, q);
  op.check(lrx_flat_ip_search_bounded_wire(x.data_ptr<float>(), x.size(0), ld(x), D, xb, row_bounds.data_ptr<float>(), q.data_ptr<float>(), Q, k32, id_base,
                                           o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), rm, (uint64_t*)o.w.data_ptr<int64_t>(), ws.data_ptr(), wsb, fl,
                                           cur_stream()));
  return {o.d, o.i, o.w};
}

// [R, Q, k] gathered wire words -> the global top-k (lrx_merge_topk_packed)
std::tuple<at::Tensor, at::Tensor> merge_topk_packed(const at::Tensor& words) {
  Op op("merge_topk_packed", words, "words");
  op.need(words, "words", at::kLong, 3);
  const int32_t R = op.i32(words.size(0), "words (its parts R)", 0), Q = op.i32(words.size(1), "words (its queries Q)", 0),
                k = op.i32(words.size(2), "words (its width k)", 0);
  at::Tensor d = at::empty({Q, k}, words.options().dtype(at::kFloat)), i = at::empty({Q, k}, words.options());
  op.check(lrx_merge_topk_packed((const uint64_t*)words.data_ptr<int64_t>(), R, Q, k, d.data_ptr<float>(), i.data_ptr<int64_t>(), cur_stream()));
  return {d, i};
}

// x_shadow: 1-D tiled fp16 shadow (whole 128-row blocks) with row0 = index of x's first row in it, or None (bounds only)
void shard_commit_rows(const at::Tensor& x, const c10::optional<at::Tensor>& x_shadow, at::Tensor row_bounds, int64_t row0) {
  Op op("shard_commit_rows", x, "x");
  op.need(x, "x", at::kFloat, 2, kRows | kVec);
  float* rb = row_bounds_ptr(op, row_bounds);
  TORCH_CHECK(row0 >= 0, "shard_commit_rows: row0 = ", row0, " must be >= 0");
  const int32_t D = op.i32(x.size(1), "x (its width)", 0);
  void* xb = tiled_rows(op, x_shadow, "x_shadow", at::kHalf, row0 + x.size(0), x.size(1), "the 1-D tiled fp16 shadow, large enough for rows row0 .. row0 + n");
  op.check(lrx_shard_commit_rows(x.data_ptr<float>(), ld(x), x.size(0), D, xb, row0, rb, cur_stream()));
}

std::tuple<at::Tensor, at::Tensor> merge_topk(const at::Tensor& d_parts, const at::Tensor& i_parts) {
  Op op("merge_topk", d_parts, "d_parts");
  op.need(d_parts, "d_parts", at::kFloat, 3);
  op.need(i_parts, "i_parts", at::kLong, 3);
  TORCH_CHECK(d_parts.sizes() == i_parts.sizes(), "merge_topk: d_parts and i_parts [R,Q,k] contiguous pairs of one shape");
  const int32_t R = op.i32(d_parts.size(0), "d_parts (its parts R)", 0), Q = op.i32(d_parts.size(1), "d_parts (its queries Q)", 0),
                k = op.i32(d_parts.size(2), "d_parts (its width k)", 0);
  at::Tensor d = at::empty({Q, k}, d_parts.options()), i = at::empty({Q, k}, i_parts.options());
  op.check(lrx_merge_topk(d_parts.data_ptr<float>(), i_parts.data_ptr<int64_t>(), R, Q, k, d.data_ptr<float>(), i.data_ptr<int64_t>(), cur_stream()));
  return {d, i};
}

// The store of the fp16 scalar-quantised index (sq_fp16_ip_topk and sq_fp16_ip_range_search; `op` names the one): codes = the 1-D tiled fp16
// codes (include/lrx.h, whole 128-row blocks) holding n_rows rows of q.size(1) columns; row_bounds [2] as maintained by shard_commit_rows
// -> the codes' address
void* sq_fp16_args(const Op& op, const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& row_bounds) {
  op.need(q, "q", at::kFloat, 2, kVec);
  row_bounds_ptr(op, row_bounds);
  TORCH_CHECK(q.size(1) % 64 == 0 && n_rows >= 0, op.name, ": q [Q,D] contiguous with D % 64 == 0, row_bounds [2], n_rows >= 0: got D = ", q.size(1),
              ", n_rows = ", n_rows);
  op.i32(q.size(1), "q (its width)", 0);
  op.i32(q.size(0), "q (its rows)", 0);
  return tiled_rows(op, codes, "codes", at::kHalf, n_rows, q.size(1), "the 1-D tiled fp16 codes of n_rows rows");
}

// lrx_sq_fp16_ip_search.  Returns (D, I, wire words) like flat_ip_topk_bounded_wire.
std::tuple<at::Tensor, at::Tensor, at::Tensor> sq_fp16_ip_topk(const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& row_bounds,
                                                               int64_t k, int64_t id_base, const c10::optional<at::Tensor>& row_map, int64_t flags) {
  Op op("sq_fp16_ip_topk", q, "q");
  void* cb = sq_fp16_args(op, q, codes, n_rows, row_bounds);
  const int32_t dim = (int32_t)q.size(1), Q = (int32_t)q.size(0), k32 = op.i32(k, "k", 1, kMaxK), fl = op.i32(flags, "flags", 0);
  const int64_t* rm = row_map_ptr(op, row_map, n_rows);
  TopK o = topk_out(q, k, true);
  const size_t wsb = lrx_sq_fp16_ip_workspace_bytes(n_rows, dim, Q, k32, fl);
  at::Tensor ws = bytes((int64_t)wsb, q);
  op.check(lrx_sq_fp16_ip_search(cb, n_rows, dim, row_bounds.data_ptr<float>(), q.data_ptr<float>(), Q, k32, id_base, o.d.data_ptr<float>(),
                                 o.i.data_ptr<int64_t>(), rm, (uint64_t*)o.w.data_ptr<int64_t>(), ws.data_ptr(), wsb, fl, cur_stream()));
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
RerankArgs rerank_args(const Op& op, const at::Tensor& q, int64_t dim, const at::Tensor& cand, int64_t k, int64_t n_rows,
                       const c10::optional<at::Tensor>& row_map) {
  op.need(q, "q", at::kFloat, 2, kVec);
  op.need(cand, "cand", at::kLong, 2, kRows);
  TORCH_CHECK(q.size(1) == dim && cand.size(0) == q.size(0), op.name, ": q [Q,D] contiguous, cand int64 [Q, n_cand]: got q [", q.size(0), ", ", q.size(1),
              "], cand [", cand.size(0), ", ", cand.size(1), "] for D = ", dim);
  const int64_t n_cand = cand.size(1);
  TORCH_CHECK(1 <= k && k <= n_cand && n_cand <= 2048 && n_rows >= 0, op.name, ": need 1 <= k <= n_cand <= 2048, got k=", k, ", n_cand=", n_cand);
  op.i32(dim, "q (its width)", 0);
  op.i32(q.size(0), "q (its rows)", 0);
  RerankArgs a;
  a.n_cand = n_cand;
  a.ld_cand = ld(cand);
  a.rm = row_map_ptr(op, row_map, n_rows);
  a.wsb = lrx_ip_rerank_workspace_bytes((int32_t)q.size(0), (int32_t)n_cand, (int32_t)k);
  a.ws = bytes((int64_t)a.wsb, q);
  return a;
}

std::tuple<at::Tensor, at::Tensor> flat_ip_rerank(const at::Tensor& q, const at::Tensor& x, const at::Tensor& cand, int64_t k, int64_t id_base,
                                                  const c10::optional<at::Tensor>& row_map) {
  Op op("flat_ip_rerank", q, "q");
  op.need(x, "x", at::kFloat, 2, kRows | kVec);
  const int64_t n_rows = x.size(0), dim = x.size(1);
  TORCH_CHECK(dim % 4 == 0 && dim > 0, "flat_ip_rerank: x [n_rows, D] with D % 4 == 0");
  RerankArgs a = rerank_args(op, q, dim, cand, k, n_rows, row_map);
  TopK o = topk_out(q, k);
  op.check(lrx_flat_ip_rerank(x.data_ptr<float>(), n_rows, ld(x), (int32_t)dim, q.data_ptr<float>(), (int32_t)q.size(0), cand.data_ptr<int64_t>(),
                              (int32_t)a.n_cand, a.ld_cand, (int32_t)k, id_base, o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), a.rm, a.ws.data_ptr(), a.wsb,
                              cur_stream()));
  return {o.d, o.i};
}

std::tuple<at::Tensor, at::Tensor> sq_fp16_ip_rerank(const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& cand, int64_t k,
                                                     int64_t id_base, const c10::optional<at::Tensor>& row_map) {
  Op op("sq_fp16_ip_rerank", q, "q");
  TORCH_CHECK(q.dim() == 2 && q.size(1) % 64 == 0 && q.size(1) > 0 && n_rows >= 0, "sq_fp16_ip_rerank: q [Q,D] with D % 64 == 0, n_rows >= 0");
  const int64_t dim = q.size(1);
  RerankArgs a = rerank_args(op, q, dim, cand, k, n_rows, row_map);
  void* cb = tiled_rows(op, codes, "codes", at::kHalf, n_rows, dim, "the 1-D tiled fp16 codes of n_rows rows");
  TopK o = topk_out(q, k);
  op.check(lrx_sq_fp16_ip_rerank(cb, n_rows, (int32_t)dim, q.data_ptr<float>(), (int32_t)q.size(0), cand.data_ptr<int64_t>(), (int32_t)a.n_cand, a.ld_cand,
                                 (int32_t)k, id_base, o.d.data_ptr<float>(), o.i.data_ptr<int64_t>(), a.rm, a.ws.data_ptr(), a.wsb, cur_stream()));
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
struct IvfArgs {
  int64_t Q, nlist, nprobe, ld_probe;
  const int64_t *ri, *rm;
  const float* ps;
};
IvfArgs ivf_args(const Op& op, const at::Tensor& q, bool store_ok, const char* shapes, int64_t n_rows, const at::Tensor& list_off, const OptTensor& row_ids,
                 const at::Tensor& probes, const OptTensor& probe_scores, bool by_residual, int64_t max_scan_rows, const OptTensor& row_map) {
  const char* who = op.name;
  op.need(list_off, "list_off", at::kLong, 1);
  op.need(probes, "probes", at::kLong, 2, kRows);
  IvfArgs a{q.size(0), list_off.size(0) - 1, probes.size(1), 0, nullptr, nullptr, nullptr};
  TORCH_CHECK(store_ok && probes.size(0) == a.Q && a.nlist >= 1, who, shapes);
  op.i32(max_scan_rows, "max_scan_rows", 0);
  op.i32(a.nlist, "list_off (its length - 1)", 1);
  op.i32(a.nprobe, "probes (its width)", 0);
  op.i32(a.Q, "q (its rows)", 0);
  op.i32(q.size(1), "q (its width)", 0);
  if (op.opt(row_ids, "row_ids", at::kLong, 1)) {
    TORCH_CHECK(row_ids->numel() >= n_rows, who, ": row_ids int64 [>= n_rows] contiguous, got ", row_ids->numel(), " for ", n_rows, " rows");
    a.ri = row_ids->data_ptr<int64_t>();
  }
  a.ld_probe = ld(probes);
  // (probe_scores without by_residual is not read, but what is given is checked: no tensor reaches the library unexamined)
  const bool has_ps = op.opt(probe_scores, "probe_scores", at::kFloat, 2, kRows);
  if (by_residual) {
    TORCH_CHECK(has_ps, who, ": by_residual needs probe_scores");
    TORCH_CHECK(probe_scores->sizes() == probes.sizes() && ld(*probe_scores) == a.ld_probe, who,
                ": probe_scores fp32 [Q, nprobe] with the row stride of probes");
    a.ps = probe_scores->data_ptr<float>();
  }
  a.rm = row_map_ptr(op, row_map, n_rows);
  return a;
}

// The selector of a *_sel op (include/lrx.h, ROW SELECTOR): the int32 words of a bitmap over the n_rows original rows, [ceil(n_rows / 32)]
// contiguous on the device, or None (no filter).  sel == nullptr: a plain op.
const uint32_t* ivf_sel_bits(const Op& op, const OptTensor* sel, int64_t n_rows) {
  if (sel == nullptr || !op.opt(*sel, "sel", at::kInt, 1)) return nullptr;
  const at::Tensor& t = **sel;
  TORCH_CHECK(t.numel() == (n_rows + 31) / 32, op.name, ": sel must be the int32 words of a selector over the ", n_rows,
              " rows of the index: [", (n_rows + 31) / 32, "] contiguous");
  return (const uint32_t*)t.data_ptr<int32_t>();
}

// Top k over the probed cells.  Every top-k entry ends (max_scan_rows, k, id_base, D, I, row_map, [sel words, sel rows,] ws, bytes, stream).
// Returns (D, I).
template <class Fam>
std::tuple<at::Tensor, at::Tensor> ivf_search(const Op& op, const Fam& f, const OptTensor* sel, int64_t k, int64_t max_scan_rows, int64_t id_base) {
  const char* who = op.name;
  op.i32(k, "k", 1, kMaxK);
  const size_t wsb = f.topk_bytes(k, max_scan_rows);
  const uint32_t* sb = ivf_sel_bits(op, sel, f.n_rows);
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
std::tuple<at::Tensor, at::Tensor, at::Tensor> ivf_search(const Op& op, const Fam& f, const OptTensor* sel, double radius, int64_t max_scan_rows,
                                                          int64_t id_base) {
  const char* who = op.name;
  const size_t wsb = f.range_bytes(max_scan_rows);
  const uint32_t* sb = ivf_sel_bits(op, sel, f.n_rows);
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
    const std::string who = std::string(Fam::name) + (std::is_same<Scalar, double>::value ? "_range_search" : "_topk") + (sel != nullptr ? "_sel" : "");
    const Op op(who.c_str(), q, "q");
    return ivf_search(op, Fam(op, q, o..., f..., max_scan_rows, row_map), sel, scalar, max_scan_rows, id_base);
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
IvfArgs ivf_flat_ip_args(const Op& op, TRef q, TRef x, TRef list_off, ORef row_ids, TRef probes, int64_t max_scan_rows, ORef row_map) {
  op.need(q, "q", at::kFloat, 2, kVec);
  op.need(x, "x", at::kFloat, 2, kRows | kVec);
  return ivf_args(op, q, q.size(1) == x.size(1),
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
  IvfFlat(const Op& op, TRef q, TRef x, TRef list_off, ORef row_ids, TRef probes, int64_t max_scan_rows, ORef row_map)
      : q(q), x(x), list_off(list_off), probes(probes), a(ivf_flat_ip_args(op, q, x, list_off, row_ids, probes, max_scan_rows, row_map)),
        n_rows(x.size(0)), dim(x.size(1)) {}
  size_t topk_bytes(int64_t k, int64_t max_scan_rows) const {
    return lrx_ivf_flat_ip_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)dim, (int32_t)a.Q, (int32_t)a.nprobe, (int32_t)k, max_scan_rows);
  }
  size_t range_bytes(int64_t max_scan_rows) const {
    return lrx_ivf_flat_ip_range_workspace_bytes(n_rows, (int32_t)a.nlist, (int32_t)dim, (int32_t)a.Q, (int32_t)a.nprobe, max_scan_rows);
  }
  template <class Entry, class... Tail>
  int head(Entry entry, Tail... tail) const {
    return entry(n_rows ? x.data_ptr<float>() : nullptr, n_rows, ld(x), (int32_t)dim, list_off.data_ptr<int64_t>(), a.ri,
                 (int32_t)a.nlist, q.data_ptr<float>(), (int32_t)a.Q, probes.data_ptr<int64_t>(), (int32_t)a.nprobe, a.ld_probe, tail...);
  }
};

// PQ codes: codes = the 1-D blocked uint8 PQ codes (whole 128-row blocks) by stored position, cell by cell; pq_centroids [M, 256, D / M] fp32;
// n_rows is the length of row_ids, or the rows the code blocks hold.
struct IvfPqStore {
  int64_t n_rows, dim, M;
  void* cb;
};
IvfArgs ivf_pq_ip_args(const Op& op, TRef q, TRef codes, TRef pq_centroids, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual,
                       int64_t max_scan_rows, ORef row_map, IvfPqStore& st) {
  op.need(q, "q", at::kFloat, 2, kVec);
  op.need(pq_centroids, "pq_centroids", at::kFloat, 3, kVec);
  const int64_t dim = q.size(1), M = pq_centroids.size(0);
  const bool store_ok = pq_centroids.size(1) == 256 && M > 0 && dim % M == 0 && pq_centroids.size(2) == dim / M;
  const int64_t mp = (M + 15) / 16 * 16;
  const int64_t n_rows = row_ids.has_value() && row_ids->defined() ? row_ids->numel() : (store_ok ? codes.numel() / mp : 0);
  const IvfArgs a = ivf_args(op, q, store_ok, ": q [Q,D] contiguous, pq_centroids [M,256,D/M] contiguous with D % M == 0, list_off int64 [nlist + 1], probes int64 [Q, nprobe]",
                             n_rows, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map);
  st = IvfPqStore{n_rows, dim, M, tiled_rows(op, codes, "codes", at::kByte, n_rows, mp, "the 1-D blocked uint8 codes of the stored rows")};
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
  IvfPq(const Op& op, TRef q, TRef codes, TRef pq_centroids, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual, int64_t max_scan_rows, ORef row_map)
      : q(q), pq_centroids(pq_centroids), list_off(list_off), probes(probes), by_residual(by_residual),
        a(ivf_pq_ip_args(op, q, codes, pq_centroids, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map, st)), n_rows(st.n_rows) {}
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
IvfArgs ivf_codes_args(const Op& op, TRef q, TRef codes, at::ScalarType code_type, const char* shapes, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores,
                       bool by_residual, int64_t max_scan_rows, ORef row_map) {
  op.need(q, "q", at::kFloat, 2, kVec);
  op.need(codes, "codes", code_type, 2, kVec);
  return ivf_args(op, q, q.size(1) == codes.size(1), shapes, codes.size(0), list_off, row_ids, probes, probe_scores, by_residual,
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
  IvfSqFp16(const Op& op, TRef q, TRef codes, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual, int64_t max_scan_rows, ORef row_map)
      : q(q), codes(codes), list_off(list_off), probes(probes), by_residual(by_residual),
        a(ivf_codes_args(op, q, codes, at::kHalf, kIvfSqShapes, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map)),
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
IvfArgs ivf_sq8_ip_args(const Op& op, TRef q, TRef codes, TRef trained, int64_t qtype, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual,
                        int64_t max_scan_rows, ORef row_map) {
  const IvfArgs a = ivf_codes_args(op, q, codes, at::kByte, kIvfSq8Shapes, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map);
  op.need(trained, "trained", at::kFloat, 1, kVec);
  TORCH_CHECK((qtype == 0 || qtype == 2) && trained.numel() == (qtype == 0 ? 2 * codes.size(1) : 2),
              op.name, ": qtype ", qtype, " (0: QT_8bit, 2: QT_8bit_uniform) with trained fp32 [2 D] or [2] contiguous");
  return a;
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
  IvfSq8(const Op& op, TRef q, TRef codes, TRef trained, int64_t qtype, TRef list_off, ORef row_ids, TRef probes, ORef probe_scores, bool by_residual, int64_t max_scan_rows,
         ORef row_map)
      : q(q), codes(codes), trained(trained), list_off(list_off), probes(probes), qtype(qtype), by_residual(by_residual),
        a(ivf_sq8_ip_args(op, q, codes, trained, qtype, list_off, row_ids, probes, probe_scores, by_residual, max_scan_rows, row_map)),
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
void* pq_args(const Op& op, const at::Tensor& q, const at::Tensor& codes, const at::Tensor& centroids, int64_t n_rows) {
  op.need(q, "q", at::kFloat, 2, kVec);
  op.need(centroids, "centroids", at::kFloat, 3, kVec);
  const int64_t dim = q.size(1), M = centroids.size(0);
  TORCH_CHECK(centroids.size(1) == 256 && M > 0 && dim % M == 0 && centroids.size(2) == dim / M && n_rows >= 0, op.name,
              ": q [Q,D] contiguous, centroids [M,256,D/M] contiguous with D % M == 0, n_rows >= 0");
  op.i32(dim, "q (its width)", 0);
  op.i32(q.size(0), "q (its rows)", 0);
  return tiled_rows(op, codes, "codes", at::kByte, n_rows, (M + 15) / 16 * 16, "the 1-D blocked uint8 codes of n_rows rows");
}

// lrx_pq_ip_search.  Returns (D, I).
std::tuple<at::Tensor, at::Tensor> pq_ip_topk(const at::Tensor& q, const at::Tensor& codes, const at::Tensor& centroids, int64_t n_rows, int64_t k,
                                              int64_t id_base, const c10::optional<at::Tensor>& row_map) {
  Op op("pq_ip_topk", q, "q");
  void* cb = pq_args(op, q, codes, centroids, n_rows);
  const int64_t dim = q.size(1), M = centroids.size(0);
  const int64_t* rm = row_map_ptr(op, row_map, n_rows);
  op.i32(k, "k", 1, kMaxK);
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
  Op op("sq8_ip_topk", q, "q");
  op.need(q, "q", at::kFloat, 2, kVec);
  op.need(trained, "trained", at::kFloat, 1, kVec);
  const int64_t dim = q.size(1);
  op.i32(dim, "q (its width)", 0);
  op.i32(q.size(0), "q (its rows)", 0);
  op.i32(k, "k", 1, kMaxK);
  TORCH_CHECK(dim > 0 && dim % 64 == 0 && (trained.numel() == 2 * dim || trained.numel() == 2) && n_rows >= 0,
              "sq8_ip_topk: q [Q,D] contiguous with D % 64 == 0, trained [2 D] (QT_8bit) or [2] (QT_8bit_uniform), n_rows >= 0");
  const int32_t qtype = trained.numel() == 2 ? 2 : 0;
  void* cb = tiled_rows(op, codes, "codes", at::kByte, n_rows, dim, "the 1-D tiled uint8 codes of n_rows rows");
  const int64_t* rm = row_map_ptr(op, row_map, n_rows);
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
int64_t impact_args(const Op& op, const at::Tensor& postings, const at::Tensor& term_off, int64_t n_rows, const at::Tensor& q_off, const at::Tensor& q_term,
                    const at::Tensor& q_cnt, int64_t window_rows, bool no_capture) {
  op.need(postings, "postings", at::kInt, 2, kVec);
  op.need(term_off, "term_off", at::kLong, 1);
  op.need(q_off, "q_off", at::kInt, 1);
  op.need(q_term, "q_term", at::kInt, 1);
  op.need(q_cnt, "q_cnt", at::kInt, 1);
  op.i32(window_rows, "window_rows", 0);
  TORCH_CHECK(postings.size(1) == 2 && term_off.numel() >= 1 && q_off.numel() >= 1 && q_term.numel() == q_cnt.numel() && n_rows >= 0,
              op.name, ": postings int32 [nnz,2] contiguous, term_off int64 [T+1], q_off int32 [Q+1], q_term / q_cnt int32 of one length, n_rows >= 0");
  TORCH_CHECK(!no_capture || c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None, op.name,
              " under graph capture: the result length is read back to the host");
  const int64_t Q = op.i32(q_off.numel() - 1, "q_off (its length - 1)", 0);
  op.i32(term_off.numel() - 1, "term_off (its length - 1)", 0);
  TORCH_CHECK(q_off[Q].item<int32_t>() == q_term.numel(), op.name, ": q_off[Q] must equal the length of q_term");
  return Q;
}

// lrx_impact_search.  The overflow refusal of the contract is the caller's (ImpactIndex.search makes it).  Returns (D, I).
std::tuple<at::Tensor, at::Tensor> impact_topk(const at::Tensor& postings, const at::Tensor& term_off, int64_t n_rows, const at::Tensor& q_off,
                                               const at::Tensor& q_term, const at::Tensor& q_cnt, int64_t k, int64_t id_base,
                                               const c10::optional<at::Tensor>& row_map, int64_t window_rows) {
  Op op("impact_topk", postings, "postings");
  op.i32(k, "k", 1, kMaxK);
  const int64_t Q = impact_args(op, postings, term_off, n_rows, q_off, q_term, q_cnt, window_rows, false);
  const int64_t* rm = row_map_ptr(op, row_map, n_rows);
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
  Op op("binary_topk", q, "q");
  op.need(q, "q", at::kFloat, 2, kVec);
  const int64_t dim = q.size(1);
  TORCH_CHECK(dim > 0 && dim % 8 == 0 && n_rows >= 0, "binary_topk: q [Q,D] contiguous with D % 8 == 0, n_rows >= 0");
  op.i32(dim, "q (its width)", 0);
  op.i32(q.size(0), "q (its rows)", 0);
  op.i32(k, "k", 1, kMaxK);
  op.i32(binary_k, "binary_k", 1, kMaxK);   // (sizes the workspace of both forms)
  void* cb = tiled_rows(op, codes, "codes", at::kByte, n_rows, (dim + 127) / 128 * 16, "the 1-D blocked uint8 codes of n_rows rows");
  const int64_t* rm = row_map_ptr(op, row_map, n_rows);
  float thr = 0.f;
  const float* thr_vec = nullptr;
  at::Tensor tv;
  if (threshold.has_value() && threshold->defined()) {
    TORCH_CHECK(threshold->numel() == 1 || threshold->numel() == dim, "binary_topk: threshold must hold 1 or D values");
    TORCH_CHECK(threshold->is_cpu() || threshold->device() == op.dev, "binary_topk: threshold is on ", threshold->device(), ", the op's first tensor on ", op.dev,
                ": it must be on the host or on that device");
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
  Op op("flat_ip_range_search", q, "q");
  void* xb = flat_bounded_args(op, q, x, x_shadow, row_bounds);
  const int64_t Q = q.size(0);
  const size_t wsb = lrx_flat_ip_range_workspace_bytes(x.size(0), (int32_t)x.size(1), (int32_t)Q, x_shadow.has_value() ? 1 : 0);
  at::Tensor ws = bytes((int64_t)wsb, q);
  return range_result(q, Q, "flat_ip_range_search", [&](int64_t* lims, float* d, int64_t* i, int64_t cap) {
    return lrx_flat_ip_range_search(x.data_ptr<float>(), x.size(0), ld(x), (int32_t)x.size(1), xb, row_bounds.data_ptr<float>(),
                                    q.data_ptr<float>(), (int32_t)Q, (float)radius, id_base, lims, d, i, cap, ws.data_ptr(), wsb, cur_stream());
  });
}

// Range search over the quantised and sparse indexes: the result protocol is range_result's (above flat_ip_range_search).
std::tuple<at::Tensor, at::Tensor, at::Tensor> sq_fp16_ip_range_search(const at::Tensor& q, const at::Tensor& codes, int64_t n_rows, const at::Tensor& row_bounds,
                                                                       double radius, int64_t id_base) {
  Op op("sq_fp16_ip_range_search", q, "q");
  void* cb = sq_fp16_args(op, q, codes, n_rows, row_bounds);
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
  Op op("pq_ip_range_search", q, "q");
  void* cb = pq_args(op, q, codes, centroids, n_rows);
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
  Op op("impact_range_search", postings, "postings");
  const int64_t Q = impact_args(op, postings, term_off, n_rows, q_off, q_term, q_cnt, window_rows, true);
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
  Op op("sparse_compact_csr", reps, "reps");
  op.need(reps, "reps", at::kFloat, 2, kRows);
  TORCH_CHECK(c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None,
              "sparse_compact_csr under graph capture: the result length is read back to the host");
  const int64_t B = reps.size(0), V = reps.size(1);
  op.i32(quantization_factor, "quantization_factor", 1);
  op.i32(B, "reps (its rows)", 0);
  op.i32(V, "reps (its width)", 1);
  const int64_t ldr = ld(reps);
  at::Tensor counts = at::empty({B}, reps.options().dtype(at::kInt));
  lrx_check(lrx_sparse_csr_count(reps.data_ptr<float>(), (int32_t)B, (int32_t)V, ldr, (int32_t)quantization_factor, empty_marker ? 1 : 0,
                                 counts.data_ptr<int32_t>(), cur_stream()),
            "sparse_compact_csr");
  at::Tensor row_off = at::zeros({B + 1}, reps.options().dtype(at::kLong));
  if (B) row_off.narrow(0, 1, B).copy_(at::cumsum(counts, 0, at::kLong));
  const int64_t nnz = B ? row_off[B].item<int64_t>() : 0;
  at::Tensor terms = at::empty({nnz}, counts.options()), weights = at::empty({nnz}, counts.options());
  lrx_check(lrx_sparse_csr_fill(reps.data_ptr<float>(), (int32_t)B, (int32_t)V, ldr, (int32_t)quantization_factor, empty_marker ? 1 : 0,
                                row_off.data_ptr<int64_t>(), terms.data_ptr<int32_t>(), weights.data_ptr<int32_t>(), cur_stream()),
            "sparse_compact_csr");
  return {row_off, terms, weights};
}

// Exact fp32 linear map (lrx_linear_transform): x [n, d_in] (rows may be strided), A [d_out, d_in] contiguous, b [d_out] or None -> [n, d_out].
at::Tensor linear_transform(const at::Tensor& x, const at::Tensor& A, const c10::optional<at::Tensor>& b) {
  Op op("linear_transform", x, "x");
  op.need(x, "x", at::kFloat, 2, kRows);
  op.need(A, "A", at::kFloat, 2);
  TORCH_CHECK(A.size(1) == x.size(1), "linear_transform: x [n, d_in], A [d_out, d_in] contiguous");
  op.i32(x.size(1), "x (its width)", 0);
  op.i32(A.size(0), "A (its rows)", 0);
  const float* bp = nullptr;
  if (op.opt(b, "b", at::kFloat, 1)) {
    TORCH_CHECK(b->numel() == A.size(0), "linear_transform: b [d_out] contiguous");
    bp = b->data_ptr<float>();
  }
  at::Tensor out = at::empty({x.size(0), A.size(0)}, x.options());
  lrx_check(lrx_linear_transform(x.data_ptr<float>(), x.size(0), ld(x), A.data_ptr<float>(), bp, (int32_t)x.size(1),
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
