// liblrx search, part 5 -- RANGE SEARCH's device side: every row whose exact score is strictly greater than a given radius (faiss
// IndexFlatIP::range_search).  Part of the ONE translation unit lrx_search.hip (included after lrx_search_refine.h; the host driver
// lrx_flat_ip_range_search sits in lrx_search.hip).  Not a stand-alone header.
//
// The chain is the bounded search's with a GIVEN threshold instead of a sampled one:
//   k_range_threshold   thr(q) = radius - eps(q) - margin, rounded down to fp32 (the derivation is next to the kernel)
//   main pass           the register-streaming _emit filter over EVERY 128-row block of the fp16 shadow (FilterMode::range): rows with
//                       s~ >= thr(q) are appended to the query's candidate list (capacity RANGE_CAP)
//   k_range_rescore     every list entry rescored exactly (exact_dot: fp64 accumulation, one rounding -- the score search() reports);
//                       survivors (score > radius) stay in the list as (score bits, row) and set their bit in the query's row bitmap
//   k_range_bitmap_prefix  per query: survivors in front of every 64-row word of the bitmap (exclusive scan of the word popcounts)
//   k_range_lims        lims[q0 + 1 + i] = lims[q0] + inclusive sum of the survivor counts (lims carried across chunks on the device)
//   k_range_fill_list   a survivor's slot = lims[q] + survivors in front of its word + set bits below it in its word: ascending row
//                       order from the atomic order of the list, for any list length, without a sort
//   score-matrix path   queries whose list overflowed (counter > cap) and every state without a list path (no shadow, dim % 64 != 0,
//                       tiny shards): six-product / exact-fp32 score matrix of <= 128 queries, then k_range_scan walks each score row
//                       in row order (count pass, then fill pass) -- ordered by construction.
// RS (ROWS_F32 / ROWS_F16T, lrx_search.hip) is the row source of the exact rescoring in k_range_rescore and k_range_scan, the way
// k_refine_band has it: ROWS_F16T is the fp16 scalar-quantised index (host driver lrx_sq_fp16_ip_range_search), whose tiled codes are the
// filter operand AND the rows the rescoring reads; its threshold is k_range_threshold<ROWS_F16T>, its score matrix the one-product filter scores.
#pragma once

#define RANGE_CAP CAND_CAP_MIN   // candidate-list entries per query (64 Ki); a query with more filter hits takes the score-matrix path

// fp32 value <= t (t rounded toward -inf)
__device__ __forceinline__ float range_round_down(double t) {
  float f = (float)t;
  if ((double)f > t) f = nextafterf(f, -INFINITY);
  return f;
}

// Threshold of the filter pass, one workgroup (256 threads) per query.  Why no row with exact score > radius can have a filter score below it:
//   s      = the exact inner product (real arithmetic) of the fp32 query and row;
//   s64    = the fp64-accumulated sum of the fp32 products; |s64 - s| <= D 2^-52 |q| R  (e64);
//   s_rep  = (float) s64, the score every search path reports; |s_rep - s64| <= 2^-24 |s64|, so s64 >= s_rep - 2^-23 |s_rep|;
//   s~     = the fp32 result of the fp16 filter MFMA, |s~ - s| <= eps(q) (query_eps_block: the fp16 rounding of q and x AND the fp32
//            accumulation / rounding of s~ itself, (D + 32) 2^-23 |q~| R).
// A row in the result has s_rep > radius.  x - 2^-23 |x| is increasing, so s64 >= s_rep - 2^-23 |s_rep| > radius - 2^-23 |radius|, and
//   s~ >= s - eps >= s64 - e64 - eps > radius - 2^-23 |radius| - e64 - eps.
// e64 <= 2^-29 eps (eps holds (D + 32) 2^-23 |q~| R + |q - q~| R >= (D + 32) 2^-23 |q| R (1 - 2^-11)), so e64 < 2^-20 eps.  The threshold
//   t = radius - 2^-23 |radius| - (1 + 2^-20) eps - 1e-30
// is formed in fp64 (its own rounding error, < 2^-52 |t|, is far inside the 2^-24 |radius| and 1e-30 of slack) and rounded DOWN to fp32,
// so thr <= t < s~ for every such row, and the filter keeps s~ >= thr.  radius = +inf: thr = +inf, nothing passes (nothing is > +inf).
// RS = ROWS_F16T: the same threshold over the fp16 CODES of the scalar-quantised index.  The codes are the rows:
//   s      = the exact inner product (real arithmetic) of the fp32 query and the decoded code row c;
//   s64    = the fp64-accumulated sum of the products q_i * (float) c_i; |s64 - s| <= D 2^-52 |q| R16  (e64), R16 >= max |c_row|;
//   s_rep  = (float) s64, the score SQFp16Index.search reports; s64 >= s_rep - 2^-23 |s_rep| as above;
//   s~     = the fp32 result of the fp16 filter MFMA over fp16(q) and c, |s~ - s| <= eps16(q) = |q - q~| R16 + (D + 32) 2^-23 |q~| R16
//            (query_eps_block<ROWS_F16T>, the bound the fp16-SQ top-k filters with).  Nothing is rounded on the row side, so the flat
//            bound's row-rounding term |q~| E is absent; the query-rounding term and the accumulation term stay.
// A row in the result has s_rep > radius, so s~ >= s - eps16 >= s64 - e64 - eps16 > radius - 2^-23 |radius| - e64 - eps16.  And
// e64 <= 2^-29 eps16: |q| <= |q~| + |q - q~| and (D + 32) 2^-23 <= 1 give (D + 32) 2^-23 |q| R16 <= eps16, and D 2^-52 <= 2^-29 (D + 32) 2^-23.
// Hence the same expression with eps16 in the place of eps:
//   t = radius - 2^-23 |radius| - (1 + 2^-20) eps16 - 1e-30,   thr = t rounded DOWN to fp32 (+inf for radius = +inf).
template <int RS>
__global__ void __launch_bounds__(256) k_range_threshold(const float* __restrict__ q, int D, const float* __restrict__ bounds, float radius,
                                                         float* __restrict__ thr) {
  __shared__ float s_red[32];
  const int qi = blockIdx.x;
  const float eps = query_eps_block<RS>(q + (int64_t)qi * D, D, bounds, nullptr, s_red);
  if (threadIdx.x == 0) {
    const double r = (double)radius;
    thr[qi] = radius == INFINITY ? INFINITY : range_round_down(r - fabs(r) * 1.1920928955078125e-7 - (double)eps * (1.0 + 9.5367431640625e-7) - 1e-30);
  }
}

// Exact rescoring of the candidate lists, grid (query, part), 256 threads: a half-wave per entry.  A list whose counter exceeds the capacity
// (entries were dropped) flags its query for the score-matrix path (statistics: lrx_search_fallback_count).  An entry becomes
// (score bits << 32 | row) when its exact score is > radius, ~0 otherwise; survivors set their bit in the query's bitmap.
// RS: the row source (row_dot, lrx_search_select.h).
template <int RS>
__global__ void __launch_bounds__(256)
k_range_rescore(const float* __restrict__ X, int64_t N, int64_t ldx, int D, const float* __restrict__ q, unsigned long long* __restrict__ cand,
                const unsigned int* __restrict__ cnt, unsigned int cap, float radius, unsigned long long* __restrict__ bits, int64_t nw,
                unsigned int* __restrict__ surv, int* __restrict__ qflags, int* __restrict__ any_flag) {
  __shared__ unsigned int s_n;
  const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned int c = cnt[(int64_t)qi * CNT_STRIDE];
  if (c > cap) {
    if (blockIdx.y == 0 && tid == 0) { qflags[qi] = 1; atomicOr(any_flag + (qi >> 7), 1); atomicAdd(&g_search_fallback_queries, 1u); }
    return;
  }
  if (tid == 0) s_n = 0;
  __syncthreads();
  unsigned long long* list = cand + (int64_t)qi * cap;
  const float* qrow = q + (int64_t)qi * D;
  unsigned long long* qbits = bits + (int64_t)qi * nw;
  const int n = (int)c, step = (int)gridDim.y * 8;
  unsigned int mine = 0;
  for (int c0 = ((int)blockIdx.y * 4 + wave) * 2; c0 < n; c0 += step) {   // (wave-uniform trip count: both half-waves take part in the dot)
    const int e = min(c0 + (lane >> 5), n - 1);
    int64_t r = sel_row(list[e]);
    r = r < 0 ? 0 : (r >= N ? N - 1 : r);                                  // (a list entry is always a shard row; clamped all the same)
    const float sc = row_dot<RS>(X, ldx, r, qrow, D, lane);
    if ((lane & 31) == 0 && c0 + (lane >> 5) < n) {
      const bool keep = sc > radius;
      list[e] = keep ? (((unsigned long long)__float_as_uint(sc) << 32) | (unsigned long long)(uint32_t)r) : ~0ull;
      if (keep) {
        atomicOr(qbits + (r >> 6), 1ull << (r & 63));
        ++mine;
      }
    }
  }
  if (mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (tid == 0 && s_n) atomicAdd(surv + qi, s_n);
}

// Per query (one 256-thread workgroup): pre[w] = survivors in words 0 .. w-1 of the query's bitmap.  Queries on the score-matrix path skip.
__global__ void __launch_bounds__(256)
k_range_bitmap_prefix(const unsigned long long* __restrict__ bits, int64_t nw, const unsigned int* __restrict__ cnt, unsigned int cap,
                      unsigned int* __restrict__ pre) {
  __shared__ unsigned int s_sum[256];
  const int qi = blockIdx.x, tid = threadIdx.x;
  if (cnt[(int64_t)qi * CNT_STRIDE] > cap) return;
  const unsigned long long* b = bits + (int64_t)qi * nw;
  unsigned int* p = pre + (int64_t)qi * nw;
  const int64_t seg = (nw + 255) / 256, w0 = tid * seg, w1 = min(nw, w0 + seg);
  unsigned int t = 0;
  for (int64_t w = w0; w < w1; ++w) t += (unsigned int)__popcll(b[w]);
  s_sum[tid] = t;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                                      // inclusive scan (Hillis-Steele)
    const unsigned int v = tid >= o ? s_sum[tid - o] : 0u;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  unsigned int run = s_sum[tid] - t;
  for (int64_t w = w0; w < w1; ++w) {
    p[w] = run;
    run += (unsigned int)__popcll(b[w]);
  }
}

// lims of one chunk: lims[i + 1] = lims[0] + survivors of queries 0..i (one workgroup; nq <= 1024).  first: lims[0] = 0 (first chunk of a call).
__global__ void __launch_bounds__(1024) k_range_lims(const unsigned int* __restrict__ surv, int nq, int64_t* __restrict__ lims, int first) {
  __shared__ int64_t s[1024];
  const int tid = threadIdx.x;
  s[tid] = tid < nq ? (int64_t)surv[tid] : 0;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int64_t v = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  const int64_t base = first ? 0 : lims[0];
  if (first && tid == 0) lims[0] = 0;
  if (tid < nq) lims[tid + 1] = base + s[tid];
}

// Output of the list path, grid (query, part): a survivor's slot follows from the bitmap (ascending row order).  Nothing is written unless the
// chunk's results fit: *lims_end <= capacity.
__global__ void __launch_bounds__(256)
k_range_fill_list(const unsigned long long* __restrict__ cand, const unsigned int* __restrict__ cnt, unsigned int cap,
                  const unsigned long long* __restrict__ bits, const unsigned int* __restrict__ pre, int64_t nw, const int64_t* __restrict__ lims,
                  const int64_t* __restrict__ lims_end, int64_t capacity, int64_t id_base, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  const int qi = blockIdx.x;
  const unsigned int c = cnt[(int64_t)qi * CNT_STRIDE];
  if (c > cap || *lims_end > capacity) return;
  const unsigned long long* list = cand + (int64_t)qi * cap;
  const unsigned long long* b = bits + (int64_t)qi * nw;
  const unsigned int* p = pre + (int64_t)qi * nw;
  const int64_t base = lims[qi];
  for (unsigned int i = blockIdx.y * 256 + threadIdx.x; i < c; i += gridDim.y * 256) {
    const unsigned long long e = list[i];
    if (e == ~0ull) continue;
    const uint32_t r = (uint32_t)e;
    const unsigned long long below = b[r >> 6] & ((1ull << (r & 63)) - 1ull);
    const int64_t pos = base + p[r >> 6] + __popcll(below);
    out_scores[pos] = __uint_as_float((uint32_t)(e >> 32));
    out_ids[pos] = id_base + (int64_t)r;
  }
}

// Score-matrix path (one 1024-thread workgroup per query, after k_flat_ip_scores_split<3> / k_flat_ip_scores over <= 128 queries): the score
// row is walked in 1024-row windows, in row order.  The matrix scores s6 are within eps6(q) = (6 D + 8) 2^-23 |q| R of s (see
// select_rescore_query); with the argument of k_range_threshold a row in the result has s6 > radius - 2^-23 |radius| - eps6, so every row with
// s6 >= thr6 = round_down(radius - 2^-23 |radius| - 2 eps6) is rescored exactly and kept when its score is > radius.  Windows whose 128-row
// block maxima are all below thr6 are skipped.  FILL = false: the query's count goes to surv[qi]; FILL = true: the survivors go to
// out[lims[qi] ..] in row order (a per-window bitmap gives each its slot), unless *lims_end > capacity.  gate / qflags: only flagged queries.
// RS = ROWS_F16T: the matrix holds the one-product fp16 filter scores over the codes, within eps16(q) of s (k_range_threshold<ROWS_F16T>), so the
// rows with a matrix score >= that kernel's thr are rescored from the codes.
template <bool FILL, int RS>
__global__ void __launch_bounds__(1024)
k_range_scan(const float* __restrict__ scores, int64_t ld, int64_t N, const float* __restrict__ blkmax, int nblk, int nblk_ld,
             const float* __restrict__ X, int64_t ldx, int D, const float* __restrict__ q, const float* __restrict__ bounds, float radius,
             const int* __restrict__ gate, const int* __restrict__ qflags, unsigned int* __restrict__ surv, const int64_t* __restrict__ lims,
             const int64_t* __restrict__ lims_end, int64_t capacity, int64_t id_base, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  __shared__ unsigned long long s_c[1024];
  __shared__ unsigned int s_words[32], s_pre[33], s_n;
  __shared__ float s_red[RS == ROWS_F32 ? 16 : 32];             // (query_eps_block: 32)
  const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((gate != nullptr && *gate == 0) || (qflags != nullptr && qflags[qi] == 0)) return;
  if (FILL && *lims_end > capacity) return;
  const float* row = scores + (int64_t)qi * ld;
  const float* bm = blkmax + (int64_t)qi * nblk_ld;
  const float* qrow = q + (int64_t)qi * D;
  float thr6;
  if constexpr (RS == ROWS_F32) {
    float q2 = 0.f;
    for (int i = tid; i < D; i += 1024) { const float v = qrow[i]; q2 += v * v; }
    q2 = wave_sum(q2);
    if (lane == 0) s_red[wave] = q2;
    __syncthreads();
    q2 = 0.f;
    for (int w = 0; w < 16; ++w) q2 += s_red[w];
    const double eps6 = (double)((float)(6 * D + 8) * 1.1920929e-7f * sqrtf(q2) * bounds[0] * 1.01f);
    const double r = (double)radius;
    thr6 = radius == INFINITY ? INFINITY : range_round_down(r - fabs(r) * 1.1920928955078125e-7 - 2.0 * eps6 - 1e-30);
  } else {
    const double eps16 = (double)query_eps_block<RS>(qrow, D, bounds, nullptr, s_red);
    const double r = (double)radius;
    thr6 = radius == INFINITY ? INFINITY : range_round_down(r - fabs(r) * 1.1920928955078125e-7 - eps16 * (1.0 + 9.5367431640625e-7) - 1e-30);
  }
  const int64_t base = FILL ? lims[qi] : 0;
  unsigned int run = 0;                                                    // survivors in the windows before (uniform)
  for (int64_t w0 = 0; w0 < N; w0 += 1024) {
    const int b = (int)(w0 >> 7) + tid;                                    // the window's eight 128-row blocks
    if (!__syncthreads_or(tid < 8 && b < nblk && bm[b] >= thr6)) continue;
    if (tid == 0) s_n = 0;
    if (tid < 32) s_words[tid] = 0;
    __syncthreads();
    const int64_t i = w0 + tid;
    if (i < N && row[i] >= thr6) s_c[atomicAdd(&s_n, 1u)] = (unsigned long long)tid;
    __syncthreads();
    const int n = (int)s_n;
    for (int c0 = wave * 2; c0 < n; c0 += 32) {
      const int e = min(c0 + (lane >> 5), n - 1);
      const int loc = (int)(uint32_t)s_c[e];
      const float sc = row_dot<RS>(X, ldx, w0 + loc, qrow, D, lane);
      if ((lane & 31) == 0 && c0 + (lane >> 5) < n) {
        const bool keep = sc > radius;
        s_c[e] = keep ? (((unsigned long long)__float_as_uint(sc) << 32) | (unsigned long long)loc) : ~0ull;
        if (keep) atomicOr(&s_words[loc >> 5], 1u << (loc & 31));
      }
    }
    __syncthreads();
    if (tid == 0) {
      unsigned int t = run;
      for (int j = 0; j < 32; ++j) { s_pre[j] = t; t += (unsigned int)__popc(s_words[j]); }
      s_pre[32] = t;
    }
    __syncthreads();
    if (FILL && tid < n) {
      const unsigned long long e = s_c[tid];
      if (e != ~0ull) {
        const int loc = (int)(uint32_t)e;
        const int64_t pos = base + s_pre[loc >> 5] + __popc(s_words[loc >> 5] & ((1u << (loc & 31)) - 1u));
        out_scores[pos] = __uint_as_float((uint32_t)(e >> 32));
        out_ids[pos] = id_base + w0 + loc;
      }
    }
    run = s_pre[32];
    __syncthreads();
  }
  if (!FILL && tid == 0) surv[qi] = run;
}
