// lrx_linear_transform: out[r][o] = b[o] + sum_k A[o][k] * x[r][k], fp32 throughout on the f32-input MFMA (v_mfma_f32_32x32x2_f32) -- the
// linear map of a PCA pre-transform (transform.py: PCAMatrix.apply / reverse_transform and the Gram matrix of its training).  DESIGN §5.4.8.
//
// Numerics (the contract of include/lrx.h): every output element has ONE accumulator, initialised with b[o] (or +0), that takes the products
// in ascending k -- the MFMA is a k-ordered chain of f32 fma (one rounding per product) and a workgroup walks the whole of K itself: no
// split-K, no atomics.  So a row's result depends on that row, A and b alone: not on n_rows, the row's position or the tile it lands in.
//
// Shape: 256 threads = 4 waves as 2 (rows) x 2 (columns); a workgroup computes BM = 64 MT rows x BN = 64 NT columns, a wave 32 MT x 32 NT as
// MT x NT accumulators of 32 x 32.  <2, 2> (128 x 128, four independent chains per wave) and <2, 1> (d_out <= 64) are the throughput tiles;
// <1, 1> (64 x 64, one chain per wave: the 32x32x2 MFMA's dependent latency equals its issue interval, so one chain still issues back to
// back) is taken when the larger tiles would be fewer than LT_SMALL_GRID workgroups -- a batch of queries -- because a workgroup walks the
// whole of K alone and the time of such a call is the time of ONE tile.  The tile never shows in the result (see above).  x and A go
// through LDS in 32-deep k-slices, two buffers, register-staged: the loads of slice s + 1 are issued before the MFMAs of slice s and written
// to the other buffer after them, one barrier per slice.  A is re-read by every row tile and left to L2.
//
// LDS image of a slice: row-major with a stride of 36 floats (144 B: the 16-byte reads of 16 consecutive rows fall on distinct banks), and
// inside every group of 8 consecutive k the even ones first: position 4 h + j holds k = 2 j + h.  Lane l = 32 h + i of the MFMA of k-step j
// needs element (row i, k = 2 j + h): one 16-byte LDS read per group gives a lane its operand of four consecutive k-steps, and the steps
// still run in ascending k.  This is why d_in must be a multiple of 8.
#include "lrx_common.h"

#define LT_BK 32    // depth of a k-slice
#define LT_SMALL_GRID 128   // fewer 128-row tiles than this: 64 x 64 tiles instead (a quarter of the work per workgroup, four times as many)
#define LT_LD 36    // LDS row stride (floats)

// 8 consecutive floats of a row (p 16-byte aligned when vec != 0), or zeros when !ok
__device__ __forceinline__ void lt_load8(const float* __restrict__ p, bool ok, int vec, f32x4& lo, f32x4& hi) {
  lo = f32x4{0.f, 0.f, 0.f, 0.f};
  hi = lo;
  if (ok) {
    if (vec) {
      lo = *(const f32x4*)p;
      hi = *(const f32x4*)(p + 4);
    } else {
      lo = f32x4{p[0], p[1], p[2], p[3]};
      hi = f32x4{p[4], p[5], p[6], p[7]};
    }
  }
}

// ... into the LDS image: the even k first
__device__ __forceinline__ void lt_store8(float* s, const f32x4& lo, const f32x4& hi) {
  *(f32x4*)s = f32x4{lo.x, lo.z, hi.x, hi.z};
  *(f32x4*)(s + 4) = f32x4{lo.y, lo.w, hi.y, hi.w};
}

template <int MT, int NT>
__global__ __launch_bounds__(256) void k_lt_linear(const float* __restrict__ x, int64_t n_rows, int64_t ldx, const float* __restrict__ A,
                                                   const float* __restrict__ bias, int K, int d_out, int n_col_tiles, float* __restrict__ out,
                                                   int64_t ldo, int vec_x, int vec_a) {
  constexpr int BM = 64 * MT, BN = 64 * NT;
  __shared__ __attribute__((aligned(16))) float sx[2][BM * LT_LD];
  __shared__ __attribute__((aligned(16))) float sa[2][BN * LT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
  const int64_t m0 = (int64_t)(blockIdx.x / (unsigned)n_col_tiles) * BM;
  const int n0 = (int)(blockIdx.x % (unsigned)n_col_tiles) * BN;

  // staging: an item is (row, group of 8 k) of the slice; x has BM x 4 items (MT per thread), A has BN x 4 (NT per thread)
  const int srow = tid >> 2, sg = tid & 3;
  f32x4 xlo[MT], xhi[MT], alo[NT], ahi[NT];
  auto load_slice = [&](int k0) {
    const int k = k0 + sg * 8;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int64_t r = m0 + srow + 64 * j;
      lt_load8(x + r * ldx + k, r < n_rows && k < K, vec_x, xlo[j], xhi[j]);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int o = n0 + srow + 64 * j;
      lt_load8(A + (int64_t)o * K + k, o < d_out && k < K, vec_a, alo[j], ahi[j]);
    }
  };
  auto store_slice = [&](int buf) {
#pragma unroll
    for (int j = 0; j < MT; ++j) lt_store8(&sx[buf][(srow + 64 * j) * LT_LD + sg * 8], xlo[j], xhi[j]);
#pragma unroll
    for (int j = 0; j < NT; ++j) lt_store8(&sa[buf][(srow + 64 * j) * LT_LD + sg * 8], alo[j], ahi[j]);
  };

  // the accumulators start at the bias: C/D of the 32x32 MFMA has its column on the lane (lane & 31)
  f32x16 acc[MT][NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = n0 + wn * 32 * NT + n * 32 + li;
    const float b0 = (bias != nullptr && col < d_out) ? bias[col] : 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = b0;
  }

  const int n_slices = (K + LT_BK - 1) / LT_BK;
  load_slice(0);
  store_slice(0);
  __syncthreads();
  for (int s = 0; s < n_slices; ++s) {
    const int buf = s & 1;
    if (s + 1 < n_slices) load_slice((s + 1) * LT_BK);
    const int rest = K - s * LT_BK;
    const int groups = rest >= LT_BK ? LT_BK / 8 : rest / 8;   // (the last slice of a K that is no multiple of 32 is shorter: nothing is padded in)
    const float* px = &sx[buf][(wm * 32 * MT + li) * LT_LD + lh * 4];
    const float* pa = &sa[buf][(wn * 32 * NT + li) * LT_LD + lh * 4];
    for (int t = 0; t < groups; ++t) {
      f32x4 fx[MT], fa[NT];
#pragma unroll
      for (int m = 0; m < MT; ++m) fx[m] = *(const f32x4*)(px + m * 32 * LT_LD + t * 8);
#pragma unroll
      for (int n = 0; n < NT; ++n) fa[n] = *(const f32x4*)(pa + n * 32 * LT_LD + t * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fx[m][j], fa[n][j], acc[m][n], 0, 0, 0);
    }
    if (s + 1 < n_slices) store_slice(buf ^ 1);
    __syncthreads();
  }

  // C/D: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5); a store instruction writes 32 consecutive columns of two rows
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int col = n0 + wn * 32 * NT + n * 32 + li;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t r = m0 + wm * 32 * MT + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (r < n_rows && col < d_out) out[r * ldo + col] = acc[m][n][e];
      }
    }
}

template <int MT, int NT>
static int lt_launch(const float* x, int64_t n_rows, int64_t ldx, const float* A, const float* b, int32_t d_in, int32_t d_out, float* out, int64_t ldo,
                     hipStream_t stream) {
  constexpr int BM = 64 * MT;
  const int64_t n_ct = lrx_cdiv(d_out, 64 * NT);
  const int64_t max_row_tiles = 0x7FFFFFFFll / n_ct;                  // (a launch's grid is one dimension of < 2^31 workgroups)
  const int vec_x = (((uintptr_t)x | (uintptr_t)(ldx * 4)) & 15) == 0, vec_a = ((uintptr_t)A & 15) == 0;   // (d_in % 8 == 0: A's rows stay aligned)
  for (int64_t t0 = 0, n_rt = lrx_cdiv(n_rows, BM); t0 < n_rt; t0 += max_row_tiles) {
    const int64_t nt = n_rt - t0 < max_row_tiles ? n_rt - t0 : max_row_tiles, r0 = t0 * BM;
    hipLaunchKernelGGL((k_lt_linear<MT, NT>), dim3((unsigned)(nt * n_ct)), dim3(256), 0, stream, x + r0 * ldx, n_rows - r0 < nt * BM ? n_rows - r0 : nt * BM,
                       ldx, A, b, (int)d_in, (int)d_out, (int)n_ct, out + r0 * ldo, ldo, vec_x, vec_a);
    LRX_LAUNCH_CHECK();
  }
  return LRX_OK;
}

extern "C" int lrx_linear_transform(const float* x, int64_t n_rows, int64_t ldx, const float* A, const float* b, int32_t d_in, int32_t d_out, float* out,
                                    int64_t ldo, void* stream) {
  LRX_CHECK_ARG(d_in >= 8 && d_in <= 8192 && d_in % 8 == 0, "linear_transform: d_in=%d must be a multiple of 8 (8 .. 8192)", d_in);
  LRX_CHECK_ARG(d_out >= 1, "linear_transform: d_out=%d must be at least 1", d_out);
  LRX_CHECK_ARG(n_rows >= 0 && ldx >= d_in && ldo >= d_out, "linear_transform: bad rows (n_rows=%lld, ldx=%lld < d_in=%d or ldo=%lld < d_out=%d)",
                (long long)n_rows, (long long)ldx, d_in, (long long)ldo, d_out);
  if (n_rows == 0) return LRX_OK;
  LRX_CHECK_ARG(x != nullptr && A != nullptr && out != nullptr, "linear_transform: null x, A or out");
  const int nt = d_out <= 64 ? 1 : 2;
  if (lrx_cdiv(n_rows, 128) * lrx_cdiv(d_out, 64 * nt) < LT_SMALL_GRID) return lt_launch<1, 1>(x, n_rows, ldx, A, b, d_in, d_out, out, ldo, (hipStream_t)stream);
  if (nt == 1) return lt_launch<2, 1>(x, n_rows, ldx, A, b, d_in, d_out, out, ldo, (hipStream_t)stream);
  return lt_launch<2, 2>(x, n_rows, ldx, A, b, d_in, d_out, out, ldo, (hipStream_t)stream);
}
