// liblrx search, part P -- ROW SELECTOR (faiss IDSelectorBatch / IDSelectorBitmap / IDSelectorRange / IDSelectorNot) for the four inverted-file
// searches: a bitmap over the ORIGINAL rows 0 .. n_bits - 1 of an index -- the number a search reports before id_base / row_map, not a stored
// position and not a mapped id.  Bit r is (bits[r >> 5] >> (r & 31)) & 1; bits is ceil(n_bits / 32) words; the bits at or beyond n_bits in the
// last word are written as 0 by every kernel here and never read by a scan (sel_test is only asked about rows inside [0, n_bits)).
// k_selector_fill, k_selector_from_mask, k_selector_set_rows, k_selector_invert and their lrx_selector_* entries (contract: include/lrx.h;
// DESIGN 5.4.15).  Part of the ONE translation unit lrx_search.hip, included ahead of lrx_search_ivf.h, whose scans read the bitmap through
// sel_test.  Not a stand-alone header.
#pragma once

extern __device__ unsigned int g_ivf_bad;   // (lrx_search_ivf.h) rows outside [0, n_bits) that k_selector_set_rows skipped are counted here

__device__ __forceinline__ bool sel_test(const uint32_t* __restrict__ bits, int64_t r) { return (bits[r >> 5] >> (unsigned)(r & 31)) & 1u; }

// the bits of word w that name rows below n_bits
__device__ __forceinline__ uint32_t sel_word_mask(int64_t w, int64_t n_bits) {
  const int64_t left = n_bits - w * 32;
  return left >= 32 ? 0xFFFFFFFFu : (left <= 0 ? 0u : (1u << (unsigned)left) - 1u);
}

__global__ void __launch_bounds__(256)
k_selector_fill(uint32_t* __restrict__ bits, int64_t n_bits, int value) {
  const int64_t nw = (n_bits + 31) >> 5;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x)
    bits[w] = value ? sel_word_mask(w, n_bits) : 0u;
}

// One thread packs the 32 mask bytes of a word (any non-zero byte is a set bit) and stores it with a plain store: two 16-byte loads where the
// word is whole and the mask is 16-byte aligned, byte loads otherwise (the last word, an unaligned view).
__global__ void __launch_bounds__(256)
k_selector_from_mask(const uint8_t* __restrict__ mask, int64_t n_bits, uint32_t* __restrict__ bits, int aligned) {
  const int64_t nw = (n_bits + 31) >> 5;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r0 = w * 32;
    uint32_t out = 0;
    if (aligned && r0 + 32 <= n_bits) {
      const uint4 a = *(const uint4*)(mask + r0), b = *(const uint4*)(mask + r0 + 16);
      const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) out |= ((v[i] >> (8 * e)) & 255u) ? 1u << (4 * i + e) : 0u;
    } else {
      const int nb = (int)(n_bits - r0 < 32 ? n_bits - r0 : 32);
      for (int e = 0; e < nb; ++e) out |= mask[r0 + e] ? 1u << e : 0u;
    }
    bits[w] = out;
  }
}

// One thread per entry: atomicOr of its bit (duplicates are fine).  A row outside [0, n_bits) is never turned into an address: it is skipped
// and counted, as a probe entry >= nlist is.
__global__ void __launch_bounds__(256)
k_selector_set_rows(const int64_t* __restrict__ rows, int64_t n, int64_t n_bits, uint32_t* __restrict__ bits) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = rows[i];
    if (r >= 0 && r < n_bits) atomicOr(&bits[r >> 5], 1u << (unsigned)(r & 31));
    else atomicAdd(&g_ivf_bad, 1u);
  }
}

__global__ void __launch_bounds__(256)
k_selector_invert(const uint32_t* in, uint32_t* out, int64_t n_bits) {   // (in may be out)
  const int64_t nw = (n_bits + 31) >> 5;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x) out[w] = ~in[w] & sel_word_mask(w, n_bits);
}

// ---- host side ---------------------------------------------------------------------------------------------------
static unsigned selector_grid(int64_t n) {
  const int64_t b = lrx_cdiv(n, 256), cap = 16 * (int64_t)lrx_cu_count();
  return (unsigned)(b < 1 ? 1 : (b < cap ? b : cap));
}
#define SELECTOR_CHECK_BITS(name, n_bits) \
  LRX_CHECK_ARG(n_bits >= 0 && n_bits < (1ll << 32), name ": n_bits=%lld out of range (0..2^32 - 1)", (long long)n_bits)

extern "C" int lrx_selector_fill(uint32_t* bits, int64_t n_bits, int32_t value, void* stream) {
  SELECTOR_CHECK_BITS("selector_fill", n_bits);
  if (n_bits == 0) return LRX_OK;
  LRX_CHECK_ARG(bits != nullptr, "selector_fill: null pointer");
  hipLaunchKernelGGL(k_selector_fill, dim3(selector_grid((n_bits + 31) >> 5)), dim3(256), 0, (hipStream_t)stream, bits, n_bits, (int)(value != 0));
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_selector_from_mask(const uint8_t* mask, int64_t n_bits, uint32_t* bits, void* stream) {
  SELECTOR_CHECK_BITS("selector_from_mask", n_bits);
  if (n_bits == 0) return LRX_OK;
  LRX_CHECK_ARG(mask != nullptr && bits != nullptr, "selector_from_mask: null pointer");
  hipLaunchKernelGGL(k_selector_from_mask, dim3(selector_grid((n_bits + 31) >> 5)), dim3(256), 0, (hipStream_t)stream, mask, n_bits, bits,
                     (int)((uintptr_t)mask % 16 == 0));
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_selector_set_rows(const int64_t* rows, int64_t n, int64_t n_bits, uint32_t* bits, void* stream) {
  SELECTOR_CHECK_BITS("selector_set_rows", n_bits);
  LRX_CHECK_ARG(n >= 0, "selector_set_rows: n=%lld must be >= 0", (long long)n);
  if (n == 0) return LRX_OK;
  LRX_CHECK_ARG(rows != nullptr && (bits != nullptr || n_bits == 0), "selector_set_rows: null pointer");
  hipLaunchKernelGGL(k_selector_set_rows, dim3(selector_grid(n)), dim3(256), 0, (hipStream_t)stream, rows, n, n_bits, bits);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_selector_invert(const uint32_t* in, uint32_t* out, int64_t n_bits, void* stream) {
  SELECTOR_CHECK_BITS("selector_invert", n_bits);
  if (n_bits == 0) return LRX_OK;
  LRX_CHECK_ARG(in != nullptr && out != nullptr, "selector_invert: null pointer");
  hipLaunchKernelGGL(k_selector_invert, dim3(selector_grid((n_bits + 31) >> 5)), dim3(256), 0, (hipStream_t)stream, in, out, n_bits);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}
