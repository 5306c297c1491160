// liblrx search, part 8 -- 8-BIT SCALAR-QUANTISED inner-product index (faiss IndexScalarQuantizer(d, QT_8bit | QT_8bit_uniform,
// METRIC_INNER_PRODUCT), range statistic RS_minmax), map: section I.
// Part of the ONE translation unit lrx_search.hip (included at its end, after lrx_search_codes.h: it reuses SelShared, select_topk_sorted and
// rescore_band of the selection, lrx_cu_count, and the shared plan, checks and scan driver).  Needs no other index header.  Contract and
// code layout: include/lrx.h (lrx_sq8_ip_search), DESIGN.md §5.4.5.
//
//     k_sq8_minmax          column min / max of a row range folded into a device [2, d] (integer atomics on the float's bits, NaN skipped)
//     k_sq8_encode          fp32 rows -> tiled codes: t = (x - vmin) / vdiff clamped to [0, 1], code = (int)(255 t)
//     k_sq8_decode          y = vmin + ((code + 0.5) / 255) vdiff (reconstruct_n; sq8_dec is also the row the exact score is defined over)
//     k_sq8_prep            per query: w = q vdiff / 255 as two int8 digit planes (w ~ scale (128 hi + lo)) in MFMA operand tiles, the bias
//                           q . vmin + 128.5 sum w, and the rigorous bound eps(q) of |filter score - exact score|
//     k_sq8_scan            THE HOT PATH: one pass over the codes on the i8 MFMA (codes xor 0x80 = code - 128 as int8, exact i32 sums),
//                           writes the [Q, ld] filter scores of a row chunk and their 128-row block maxima
//     k_sq8_select_rescore  per query: top-k of the filter scores, every row within 2 eps of the k-th rescored from the codes in fp64,
//                           the best k returned (rescore_band; a band larger than the list takes its streaming form, counted as a fallback)
#pragma once

#define SQ8_BLK 128                     // rows per code block
#define SQ8_QT_MAX 8                    // 16-query tiles per scan launch
#define SQ8_QCHUNK (16 * SQ8_QT_MAX)    // queries per library chunk
#define SQ8_ROW_CHUNK (1ll << 22)       // rows per score matrix
#define SQ8_MATRIX_BYTES (1ll << 30)    // score matrix budget of one query chunk
#define SQ8_NMAX 16319                  // |128 hi + lo| <= 127 * 128 + 63: hi in [-127, 127], lo in [-64, 63]
#define SQ8_QT_8BIT 0                   // faiss ScalarQuantizer::QuantizerType
#define SQ8_QT_8BIT_UNIFORM 2

typedef int sq8_i32x4 __attribute__((ext_vector_type(4)));

// byte offset of code (row r, dimension i) in the tiled layout (include/lrx.h): block r / 128, 64-column slice i / 64, 16-row group, then
// the 1-KiB MFMA operand tile [16-column piece i % 64 / 16][row r % 16][16 bytes]: lane l = 16 piece + row of a wave loads bytes 16 l .. 16 l + 15
static __host__ __device__ __forceinline__ int64_t sq8_code_off(int64_t r, int i, int D) {
  return (r >> 7) * SQ8_BLK * (int64_t)D + (int64_t)(i >> 6) * (SQ8_BLK * 64) + ((r >> 4) & 7) * 1024 + ((i >> 4) & 3) * 256 + (r & 15) * 16 + (i & 15);
}

// the contract's decode, fp32, no contraction, IEEE division
__device__ __forceinline__ float sq8_dec(uint32_t c, float vmin, float vdiff) {
#pragma clang fp contract(off)
  const float t = __fdiv_rn((float)c + 0.5f, 255.f);
  const float m = t * vdiff;
  return vmin + m;
}

__device__ __forceinline__ void sq8_atomic_min(float* addr, float v) {   // (+0 canonical: the caller adds 0.f)
  if (v >= 0.f) atomicMin((int*)addr, __float_as_int(v));
  else atomicMax((unsigned int*)addr, __float_as_uint(v));
}
__device__ __forceinline__ void sq8_atomic_max(float* addr, float v) {
  if (v >= 0.f) atomicMax((int*)addr, __float_as_int(v));
  else atomicMin((unsigned int*)addr, __float_as_uint(v));
}

// Grid (d / 64, row strips of 1024): lane = column, the four waves take every fourth row of the strip; the strip's minimum and maximum
// are folded into mm[0][col] / mm[1][col] (initialised to +inf / -inf by the caller) with integer atomics on the bits of the float:
// order-independent, so the result is determined by the rows.  NaN is skipped (fminf / fmaxf semantics); -0 counts as +0.
__global__ void __launch_bounds__(256)
k_sq8_minmax(const float* __restrict__ X, int64_t n_rows, int64_t ldx, int D, float* __restrict__ mm) {
  __shared__ float s_mn[4][64], s_mx[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * 1024;
  const int64_t r1 = r0 + 1024 < n_rows ? r0 + 1024 : n_rows;
  float mn = INFINITY, mx = -INFINITY;
  if (col < D)
    for (int64_t r = r0 + wave; r < r1; r += 4) {
      const float v = X[r * ldx + col] + 0.f;
      if (v == v) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    }
  s_mn[wave][lane] = mn;
  s_mx[wave][lane] = mx;
  __syncthreads();
  if (wave == 0 && col < D) {
#pragma unroll
    for (int w = 1; w < 4; ++w) { mn = s_mn[w][lane] < mn ? s_mn[w][lane] : mn; mx = s_mx[w][lane] > mx ? s_mx[w][lane] : mx; }
    if (mn <= mx) { sq8_atomic_min(mm + col, mn); sq8_atomic_max(mm + D + col, mx); }
  }
}

// One thread per 16-column piece of a row: 64 B of fp32 in, one 16-byte store into the tiled codes.
__global__ void __launch_bounds__(256)
k_sq8_encode(const float* __restrict__ X, int64_t n_rows, int64_t ldx, const float* __restrict__ trained, int D, int uniform,
             uint8_t* __restrict__ codes, int64_t row0) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int pieces = D >> 4;
  if (t >= n_rows * pieces) return;
  const int64_t r = t / pieces;
  const int i0 = (int)(t - r * pieces) * 16;
  const float* x = X + r * ldx + i0;
  uint32_t w[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = i0 + 4 * g + e;
      const float vmin = trained[uniform ? 0 : i], vdiff = trained[uniform ? 1 : D + i];
      float u = vdiff != 0.f ? __fdiv_rn(x[4 * g + e] - vmin, vdiff) : 0.f;
      if (!(u >= 0.f)) u = 0.f;                       // below the range, and NaN
      if (u > 1.f) u = 1.f;
      word |= (uint32_t)(int)(255.f * u) << (8 * e);
    }
    w[g] = word;
  }
  *(uint4*)(codes + sq8_code_off(row0 + r, i0, D)) = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void __launch_bounds__(256)
k_sq8_decode(const uint8_t* __restrict__ codes, int64_t row0, int64_t n_rows, const float* __restrict__ trained, int D, int uniform,
             float* __restrict__ out, int64_t ldo) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * D) return;
  const int64_t r = t / D;
  const int i = (int)(t - r * D);
  out[r * ldo + i] = sq8_dec(codes[sq8_code_off(row0 + r, i, D)], trained[uniform ? 0 : i], trained[uniform ? 1 : D + i]);
}

__device__ __forceinline__ double sq8_block_sum(double v, double* red /* 4 */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per query of the padded chunk (16 qtiles queries; the padding queries get zero digits).  With w_i = q_i vdiff_i / 255
// (fp64) the contract's score is, up to the roundings listed below, sum_i w_i (code_i - 128) + bias, bias = q . vmin + 128.5 sum_i w_i.
// The scan multiplies n_i = round(w_i / scale) = 128 hi_i + lo_i, scale = max |w| / SQ8_NMAX, exactly (i8 x i8 -> i32), so
//     |filter - exact| <= 128 sum_i |w_i - scale n_i|                  (|code - 128| <= 128)
//                       + 2^-21 sum_i |q_i| (|vmin_i| + |vdiff_i|)     (three fp32 roundings of the decode, < 3.03 2^-24 (|vmin| + |vdiff|) per
//                                                                      element; the fp32 roundings of the filter score and of the exact score,
//                                                                      each < 1.01 2^-24 of the same sum: 5.05 2^-24 < 2^-21)
//                       + 3 2^-149 sum_i |q_i|                         (where t vdiff or vmin + m is subnormal its rounding error is absolute,
//                                                                      at most 2^-150 each; scores themselves are assumed normal or zero)
// eps(q) is that sum, evaluated in fp64, times 1.01 (the fp64 roundings of w, bias and the sums are below 2^-40 of it), rounded up to fp32.
// Digit tile of (query tile qt, 64-column slice kc, plane p): 1 KiB at ((qt KC + kc) 2 + p) 1024, [16-column piece][query % 16][16 bytes].
__global__ void __launch_bounds__(256)
k_sq8_prep(const float* __restrict__ q, int nq, const float* __restrict__ trained, int D, int uniform, int8_t* __restrict__ digits,
           double* __restrict__ qscale, double* __restrict__ qbias, float* __restrict__ qeps) {
  __shared__ double red[4];
  __shared__ float s_max[4];
  const int qi = blockIdx.x, tid = threadIdx.x;
  const int KC = D >> 6;
  int8_t* dq = digits + (int64_t)(qi >> 4) * KC * 2048 + (qi & 15) * 16;
  if (qi >= nq) {
    for (int i = tid; i < D; i += 256) {
      const int64_t o = (int64_t)(i >> 6) * 2048 + ((i >> 4) & 3) * 256 + (i & 15);
      dq[o] = 0;
      dq[o + 1024] = 0;
    }
    return;
  }
  const float* qrow = q + (int64_t)qi * D;
  double sw = 0.0, sv = 0.0, st = 0.0, sa = 0.0;
  float mw = 0.f;
  for (int i = tid; i < D; i += 256) {
    const double qv = (double)qrow[i], vmin = (double)trained[uniform ? 0 : i], vdiff = (double)trained[uniform ? 1 : D + i];
    const double w = qv * vdiff / 255.0;
    sw += w;
    sv += qv * vmin;
    st += fabs(qv) * (fabs(vmin) + fabs(vdiff));
    sa += fabs(qv);
    mw = fmaxf(mw, (float)fabs(w) * 1.0000002f);
  }
  mw = wave_max(mw);
  if ((tid & 63) == 0) s_max[tid >> 6] = mw;
  sw = sq8_block_sum(sw, red);
  sv = sq8_block_sum(sv, red);
  st = sq8_block_sum(st, red);
  sa = sq8_block_sum(sa, red);
  const double wmax = (double)fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));   // >= max |w| (rounded up)
  const double scale = wmax / (double)SQ8_NMAX;
  double err = 0.0;
  for (int i = tid; i < D; i += 256) {
    const double w = (double)qrow[i] * (double)trained[uniform ? 1 : D + i] / 255.0;
    int n = scale > 0.0 ? (int)rint(w / scale) : 0;
    n = n > SQ8_NMAX ? SQ8_NMAX : (n < -SQ8_NMAX ? -SQ8_NMAX : n);
    const int hi = (n + 64) >> 7, lo = n - 128 * hi;     // hi in [-127, 127], lo in [-64, 63]
    err += fabs(w - scale * (double)n);
    const int64_t o = (int64_t)(i >> 6) * 2048 + ((i >> 4) & 3) * 256 + (i & 15);
    dq[o] = (int8_t)hi;
    dq[o + 1024] = (int8_t)lo;
  }
  err = sq8_block_sum(err, red);
  if (tid == 0) {
    qscale[qi] = scale;
    qbias[qi] = sv + 128.5 * sw;
    qeps[qi] = (float)((128.0 * err + st * 4.76837158203125e-07 + sa * (3.0 * 0x1p-149)) * 1.01) * 1.0000002f;   // (2^-21, 3 2^-149)
  }
}

// The filter scan.  256 threads, workgroup x walks the 128-row blocks x, x + gridDim.x, ...; wave w owns the 16-row groups 2 w and 2 w + 1
// of the block and QT 16-query tiles.  Per 64-column slice a wave loads its two code tiles (1 KiB each, 16 bytes per lane, streamed once:
// non-temporal) and the 2 QT digit tiles of the queries (L2-resident, the same for every block), flips the codes' top bits (code - 128 as
// int8) and issues 4 QT mfma_i32_16x16x64_i8.  Lane l of both operands holds columns 16 (l / 16) .. + 15 of the slice for row / query
// l % 16: the MFMA pairs byte j of lane group g of A with byte j of lane group g of B whatever its internal k order, and a dot product does
// not depend on the order of its terms -- exact in i32 (|sum| <= 128 * 128 * d < 2^31 for d <= 65536).
// Epilogue: C element (lane, j) is (query l % 16, row 4 (l / 16) + j of the group); score = (float)(scale (128 hi + lo) + bias) in fp64,
// four consecutive rows of a query per lane: one 16-byte store.  Block maxima over the valid rows (-> select_topk_sorted).
template <int QT>
__global__ void __launch_bounds__(256)
k_sq8_scan(const uint8_t* __restrict__ codes, int64_t n_rows, int D, const int8_t* __restrict__ digits, const double* __restrict__ qscale,
           const double* __restrict__ qbias, int nq, float* __restrict__ scores, int64_t ld, float* __restrict__ blkmax, int nblk_ld) {
  __shared__ float s_max[4][QT * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KC = D >> 6;
  const int64_t nblk = (n_rows + SQ8_BLK - 1) / SQ8_BLK;
  const int qcol = lane & 15;
  double sc[QT], bs[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qi = t * 16 + qcol;
    sc[t] = qi < nq ? qscale[qi] : 0.0;
    bs[t] = qi < nq ? qbias[qi] : 0.0;
  }
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    sq8_i32x4 ah[2][QT], al[2][QT];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int t = 0; t < QT; ++t) { ah[g][t] = sq8_i32x4{0, 0, 0, 0}; al[g][t] = sq8_i32x4{0, 0, 0, 0}; }
    const uint8_t* ap = codes + blk * SQ8_BLK * (int64_t)D + (2 * wave) * 1024 + lane * 16;
    const int8_t* bp = digits + lane * 16;
    // (An explicit prefetch of slice kc + 1 into a second register set was measured and not kept: k_sq8_scan<8> 1.35 ms against 1.06 - 1.08 ms
    // at 1M x 2048, Q = 100 -- 404 VGPRs instead of 360 and no shorter wait.  The compiler does not unroll this loop on request either.)
    for (int kc = 0; kc < KC; ++kc) {
      sq8_i32x4 a0 = __builtin_nontemporal_load((const sq8_i32x4*)(ap + (int64_t)kc * (SQ8_BLK * 64)));
      sq8_i32x4 a1 = __builtin_nontemporal_load((const sq8_i32x4*)(ap + (int64_t)kc * (SQ8_BLK * 64) + 1024));
      a0 ^= (int)0x80808080;
      a1 ^= (int)0x80808080;
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const sq8_i32x4 bh = *(const sq8_i32x4*)(bp + ((int64_t)t * KC + kc) * 2048);
        const sq8_i32x4 bl = *(const sq8_i32x4*)(bp + ((int64_t)t * KC + kc) * 2048 + 1024);
        ah[0][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, bh, ah[0][t], 0, 0, 0);
        al[0][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, bl, al[0][t], 0, 0, 0);
        ah[1][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, bh, ah[1][t], 0, 0, 0);
        al[1][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, bl, al[1][t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int qi = t * 16 + qcol;
      float mx = -INFINITY;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int64_t r = blk * SQ8_BLK + (2 * wave + g) * 16 + (lane >> 4) * 4;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = (float)(sc[t] * (128.0 * (double)ah[g][t][j] + (double)al[g][t][j]) + bs[t]);
          if (r + j < n_rows) mx = fmaxf(mx, v[j]);
        }
        if (qi < nq) *(float4*)(scores + (int64_t)qi * ld + r) = make_float4(v[0], v[1], v[2], v[3]);   // (ld covers whole blocks)
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      if (lane < 16) s_max[wave][t * 16 + lane] = mx;
    }
    __syncthreads();
    if (tid < QT * 16 && tid < nq)
      blkmax[(int64_t)tid * nblk_ld + blk] = fmaxf(fmaxf(s_max[0][tid], s_max[1][tid]), fmaxf(s_max[2][tid], s_max[3][tid]));
    __syncthreads();
  }
}

// The contract's score of row r by one half-wave: lane sub decodes the 16-column pieces sub, sub + 32, ... (one 16-byte load each) with
// sq8_dec and accumulates (double) q_i * (double) y_i; xor tree over the 32 lanes, one rounding to fp32.
__device__ __forceinline__ float sq8_row_dot(const uint8_t* __restrict__ codes, int64_t r, const float* __restrict__ qrow,
                                             const float* __restrict__ trained, int D, int uniform, int lane) {
  const int sub = lane & 31;
  double acc = 0.0;
  for (int i0 = sub * 16; i0 < D; i0 += 512) {
    const sq8_i32x4 cw = __builtin_nontemporal_load((const sq8_i32x4*)(codes + sq8_code_off(r, i0, D)));
    const uint32_t w[4] = {(uint32_t)cw[0], (uint32_t)cw[1], (uint32_t)cw[2], (uint32_t)cw[3]};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = i0 + 4 * g;
      const f32x4 qv = *(const f32x4*)(qrow + i);
      f32x4 mn, df;
      if (uniform) {
        mn = f32x4{trained[0], trained[0], trained[0], trained[0]};
        df = f32x4{trained[1], trained[1], trained[1], trained[1]};
      } else {
        mn = *(const f32x4*)(trained + i);
        df = *(const f32x4*)(trained + D + i);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (double)qv[e] * (double)sq8_dec((w[g] >> (8 * e)) & 255u, mn[e], df[e]);
    }
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  return (float)acc;
}

// Selection + exact rescoring of one query over one row chunk: select_rescore_query (lrx_search_select.h) with the query's own eps and the
// rows rescored from the 8-bit codes.  k rows have filter score >= kth, each of them has an exact score >= kth - eps, so the exact k-th score
// is >= kth - eps and every row of the exact top-k has filter score >= kth - 2 eps: all rows at or above that threshold (lowered by one
// more ulp for the rounding of the subtraction) are rescored and the best k of them returned (rescore_band; its streaming form is counted
// in g_search_fallback_queries).  Row ids are chunk-local + id_base.
__global__ void __launch_bounds__(SEL_THREADS)
k_sq8_select_rescore(const float* __restrict__ scores, int64_t ld, int64_t N, int k, int64_t id_base, const float* __restrict__ blkmax, int nblk,
                     int nblk_ld, const uint8_t* __restrict__ codes, const float* __restrict__ trained, int D, int uniform,
                     const float* __restrict__ q, const float* __restrict__ qeps, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  __shared__ SelShared sh;
  const float* row = scores + (int64_t)blockIdx.x * ld;
  float* os = out_scores + (int64_t)blockIdx.x * k;
  int64_t* oi = out_ids + (int64_t)blockIdx.x * k;
  const int tid = threadIdx.x, lane = tid & 63;
  const int keff = (int)(N < (int64_t)k ? N : (int64_t)k);
  for (int i = keff + tid; i < k; i += SEL_THREADS) { os[i] = -FLT_MAX; oi[i] = -1; }
  if (keff == 0) return;
  const float* qrow = q + (int64_t)blockIdx.x * D;
  const float* bm = blkmax + (int64_t)blockIdx.x * nblk_ld;
  select_topk_sorted(row, N, keff, bm, nblk, sh);            // sh.cand[0..keff): the top-keff by filter score, sorted
  const float kth = key2f((uint32_t)(sh.cand[keff - 1] >> 32));
  float thr = kth - 2.0f * qeps[blockIdx.x];
  thr -= fabsf(thr) * 1.1920929e-7f;                         // (a non-finite query gives a NaN threshold: the filter selection stands)
  const bool streamed = rescore_band(row, N, keff, thr, bm, nblk, id_base, os, oi, sh,
                                     [&](int64_t r) { return sq8_row_dot(codes, r, qrow, trained, D, uniform, lane); });
  if (streamed && tid == 0) atomicAdd(&g_search_fallback_queries, 1u);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int sq8_scan_tiles(int nq) { const int t = (int)lrx_cdiv(nq, 16); return t <= 1 ? 1 : (t <= 2 ? 2 : (t <= 4 ? 4 : 8)); }   // k_sq8_scan<QT>

// the leading regions of the workspace: what k_sq8_prep writes for a chunk of qc queries
struct SQ8Lead { size_t scale_off, bias_off, eps_off, total; };   // (the digit tiles are at 0)
static SQ8Lead sq8_lead(int qc, int32_t dim) {
  const size_t q = (size_t)qc, qpad = (size_t)sq8_scan_tiles(qc) * 16;   // digit tiles of every query tile the scan template reads
  SQ8Lead l;
  l.scale_off = align256(qpad * (size_t)dim * 2);
  l.bias_off = l.scale_off + align256(q * 8);
  l.eps_off = l.bias_off + align256(q * 8);
  l.total = l.eps_off + align256(q * 4);
  return l;
}

static ScanPlan sq8_plan(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k) {
  return scan_plan(n_rows, n_queries, k, SQ8_ROW_CHUNK, SQ8_BLK, SQ8_MATRIX_BYTES, SQ8_QCHUNK, [&](int qc) { return sq8_lead(qc, dim).total; });
}

static bool sq8_qtype_ok(int32_t qtype) { return qtype == SQ8_QT_8BIT || qtype == SQ8_QT_8BIT_UNIFORM; }
#define SQ8_CHECK_DIM(name, dim, qtype)                                                                                         \
  LRX_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= 65536, name ": dim=%d must be a multiple of 64 (at most 65536)", dim); \
  LRX_CHECK_ARG(sq8_qtype_ok(qtype), name ": qtype=%d (0: QT_8bit, 2: QT_8bit_uniform)", qtype)

extern "C" size_t lrx_sq8_ip_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k) {
  return sq8_plan(n_rows, dim > 0 ? dim : 64, n_queries, k).total;
}

extern "C" int32_t lrx_sq8_ip_chunk_queries(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k) {
  return sq8_plan(n_rows, dim > 0 ? dim : 64, n_queries, k).qc;
}

// Where a search of these arguments keeps the state of a query chunk in its workspace (host only; the regions are rewritten per query chunk and
// the matrix per row chunk, so after a search they show its last query chunk and last row chunk).
extern "C" int lrx_sq8_ip_workspace_layout(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int64_t out[LRX_SQ8_LAYOUT_INTS]) {
  LRX_CHECK_ARG(out != nullptr && dim > 0 && dim % 64 == 0 && dim <= 65536 && n_rows >= 0 && n_queries > 0 && k > 0,
                "sq8_ip_workspace_layout: bad arguments (n_rows=%lld, dim=%d, n_queries=%d, k=%d)", (long long)n_rows, dim, n_queries, k);
  const ScanPlan p = sq8_plan(n_rows, dim, n_queries, k);
  const SQ8Lead l = sq8_lead(p.qc, dim);
  const int64_t v[LRX_SQ8_LAYOUT_INTS] = {p.qc, p.rc, p.ld, p.nblk_ld, 16ll * sq8_scan_tiles(p.qc), 0, (int64_t)l.scale_off, (int64_t)l.bias_off,
                                          (int64_t)l.eps_off, (int64_t)p.sc_off, (int64_t)p.bm_off, (int64_t)p.total};
  for (int i = 0; i < LRX_SQ8_LAYOUT_INTS; ++i) out[i] = v[i];
  return LRX_OK;
}

extern "C" int lrx_sq8_train_minmax(const float* x, int64_t n_rows, int64_t ldx, int32_t dim, float* minmax, void* stream) {
  LRX_CHECK_ARG(dim > 0 && n_rows >= 0 && ldx >= dim, "sq8_train_minmax: bad rows (n_rows=%lld, dim=%d, ldx=%lld)", (long long)n_rows, dim, (long long)ldx);
  if (n_rows == 0) return LRX_OK;
  for (int64_t r0 = 0; r0 < n_rows; r0 += 1024 * 32768ll) {   // (grid.y <= 65535)
    const int64_t nr = n_rows - r0 < 1024 * 32768ll ? n_rows - r0 : 1024 * 32768ll;
    hipLaunchKernelGGL(k_sq8_minmax, dim3((unsigned)lrx_cdiv(dim, 64), (unsigned)lrx_cdiv(nr, 1024)), dim3(256), 0, (hipStream_t)stream, x + r0 * ldx, nr,
                       ldx, dim, minmax);
    LRX_LAUNCH_CHECK();
  }
  return LRX_OK;
}

extern "C" int lrx_sq8_encode(const float* x, int64_t n_rows, int64_t ldx, const float* trained, int32_t dim, int32_t qtype, void* codes, int64_t row0,
                              void* stream) {
  SQ8_CHECK_DIM("sq8_encode", dim, qtype);
  LRX_CHECK_ARG(n_rows >= 0 && row0 >= 0 && ldx >= dim, "sq8_encode: bad rows (n_rows=%lld, row0=%lld, ldx=%lld)", (long long)n_rows, (long long)row0,
                (long long)ldx);
  if (n_rows == 0) return LRX_OK;
  const int64_t n = n_rows * (dim / 16);
  hipLaunchKernelGGL(k_sq8_encode, dim3((unsigned)lrx_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n_rows, ldx, trained, dim,
                     qtype == SQ8_QT_8BIT_UNIFORM ? 1 : 0, (uint8_t*)codes, row0);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_sq8_decode_rows(const void* codes, int64_t row0, int64_t n_rows, const float* trained, int32_t dim, int32_t qtype, float* out,
                                   int64_t ldo, void* stream) {
  SQ8_CHECK_DIM("sq8_decode_rows", dim, qtype);
  LRX_CHECK_ARG(row0 >= 0 && ldo >= dim, "sq8_decode_rows: row0=%lld, ldo=%lld", (long long)row0, (long long)ldo);
  if (n_rows <= 0) return LRX_OK;
  const int64_t n = n_rows * dim;
  LRX_CHECK_ARG(lrx_cdiv(n, 256) < (1ll << 31), "sq8_decode_rows: %lld rows at once (decode in pieces)", (long long)n_rows);
  hipLaunchKernelGGL(k_sq8_decode, dim3((unsigned)lrx_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, row0, n_rows, trained, dim,
                     qtype == SQ8_QT_8BIT_UNIFORM ? 1 : 0, out, ldo);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

#define SQ8_SCAN(QT_)                                                                                                                           \
  hipLaunchKernelGGL(k_sq8_scan<QT_>, dim3((unsigned)gx), dim3(256), 0, s, cchunk(r0), nr, (int)dim, (const int8_t*)dig, (const double*)qscale, \
                     (const double*)qbias, nq, sc, p.ld, bm, p.nblk_ld)

extern "C" int lrx_sq8_ip_search(const void* codes, int64_t n_rows, const float* trained, int32_t dim, int32_t qtype, const float* q, int32_t n_queries,
                                 int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace,
                                 size_t workspace_bytes, int32_t flags, void* stream) {
  (void)flags;
  int rc = codes_check_topk("sq8_ip_search", k, n_rows);
  if (rc != LRX_OK) return rc;
  SQ8_CHECK_DIM("sq8_ip_search", dim, qtype);
  if (n_queries <= 0) return LRX_OK;
  const ScanPlan p = sq8_plan(n_rows, dim, n_queries, k);
  if ((rc = codes_check_workspace("sq8_ip_search", workspace_bytes, p.total)) != LRX_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const SQ8Lead l = sq8_lead(p.qc, dim);
  int8_t* dig = (int8_t*)ws;
  double* qscale = (double*)(ws + l.scale_off);
  double* qbias = (double*)(ws + l.bias_off);
  float* qeps = (float*)(ws + l.eps_off);
  const int uniform = qtype == SQ8_QT_8BIT_UNIFORM ? 1 : 0;
  const int ncu = lrx_cu_count();
  auto cchunk = [&](int64_t r0) { return (const uint8_t*)codes + r0 * (int64_t)dim; };   // (r0 is a multiple of 128)
  return scan_search(
      p, workspace, n_rows, n_queries, k, id_base, out_scores, out_ids, row_map, stream,
      [&](int32_t q0, int nq) {
        hipLaunchKernelGGL(k_sq8_prep, dim3(sq8_scan_tiles(nq) * 16), dim3(256), 0, s, q + (int64_t)q0 * dim, nq, trained, (int)dim, uniform, dig, qscale,
                           qbias, qeps);
        LRX_LAUNCH_CHECK();
        return LRX_OK;
      },
      [&](int64_t r0, int64_t nr, int nq, float* sc, float* bm) {
        const int64_t nblk = lrx_cdiv(nr, SQ8_BLK);
        const int64_t gx = nblk < 8 * (int64_t)ncu ? nblk : 8 * (int64_t)ncu;
        switch (sq8_scan_tiles(nq)) {
          case 1: SQ8_SCAN(1); break;
          case 2: SQ8_SCAN(2); break;
          case 4: SQ8_SCAN(4); break;
          default: SQ8_SCAN(8); break;
        }
        LRX_LAUNCH_CHECK();
        return LRX_OK;
      },
      [&](int32_t q0, int64_t r0, int64_t nr, int nq, const float* sc, const float* bm, float* os, int64_t* oi) {
        hipLaunchKernelGGL(k_sq8_select_rescore, dim3(nq), dim3(SEL_THREADS), 0, s, sc, p.ld, nr, k, r0, bm, (int)lrx_cdiv(nr, SQ8_BLK), p.nblk_ld,
                           cchunk(r0), trained, (int)dim, uniform, q + (int64_t)q0 * dim, (const float*)qeps, os, oi);
        LRX_LAUNCH_CHECK();
        return LRX_OK;
      });
}
