// liblrx search, part 9 -- IMPACT index: the sparse half of the hybrid retriever (Lucene impact search, `-impact -pretokenized` over a
// JsonVectorCollection), map: section J.
// Part of the ONE translation unit lrx_search.hip (included at its end, after lrx_search_codes.h: it reuses k_topk_select, lrx_cu_count and
// the shared plan, checks and scan driver).  Needs no other index header.  Contract and storage: include/lrx.h (lrx_impact_search),
// DESIGN.md §5.4.6.
//
//     k_impact_scan   THE HOT PATH: one workgroup per (query, window of W consecutive rows); term at a time, the window's piece of each
//                     posting list (lower-bound search on the rows) streamed into int32 accumulators in LDS with non-returning adds;
//                     writes its slice of the [Q, ld] fp32 score matrix (zeros included) and the 128-row block maxima -> k_topk_select
//     k_impact_hits   entries of the [Q, k] result whose score is not positive (rows that share no term with the query) become padding
// Range search (lrx_range_impact_search): the same k_impact_scan under scan_range (lrx_search_codes.h) -- every HIT whose score is > radius,
// never cut at k: the predicate is s > 0 && s > radius on the matrix score (float) S.
#pragma once

#define IMP_MAX_W 32768                 // rows per window at most: 128 KiB of int32 accumulators next to 6 KiB of term ranges
#define IMP_TCHUNK 256                  // query terms whose posting ranges sit in LDS at once; more are walked in passes
#define IMP_ROW_CHUNK (1ll << 22)       // rows per score matrix (16 MiB per query)
#define IMP_MATRIX_BYTES (1ll << 30)    // score matrix budget of one query chunk
#define IMP_QC_MAX 65535                // queries per chunk at most (grid.y)

typedef int imp_i32x2 __attribute__((ext_vector_type(2)));
typedef int imp_i32x4 __attribute__((ext_vector_type(4)));

// first posting of [lo, hi) whose row is >= row (postings of a term ascend by row)
__device__ __forceinline__ int64_t imp_lower_bound(const imp_i32x2* __restrict__ post, int64_t lo, int64_t hi, int64_t row) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)post[mid][0] < row) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// acc[row - base] += cnt * weight.  The result of the add is not used: a non-returning LDS add.  (The range check cannot fail for postings
// sorted as the contract says; it keeps a corrupt index inside the window.)
__device__ __forceinline__ void imp_add(int* acc, int W, int64_t base, int row, int weight, int cnt) {
  const int64_t i = (int64_t)row - base;
  if ((uint64_t)i < (uint64_t)W) atomicAdd(acc + i, cnt * weight);
}

// Grid (windows, queries), W a multiple of 128.  Workgroup (x, q) owns rows [x W, x W + W) of the row chunk [r0, r0 + nr) for query q.
//   1. accumulators to zero;
//   2. per pass of up to IMP_TCHUNK query terms: thread e searches one end of term e / 2's range (both ends of every term at once: the
//      ~log2(list) dependent probes of all terms overlap), then the terms are streamed one after the other WITHOUT barriers between them:
//      thread (tid + 64 term) % threads takes pairs i, i + threads, ... of the term's range, four 16-byte loads (two postings each) in flight
//      before the first add, so a short range occupies one wave and the others run ahead to the next term.  An odd first or last posting
//      is taken alone (the pairs are 16-byte aligned);
//   3. (float) of every accumulator -- one round-to-nearest-even conversion, the contract's score -- as 16-byte stores over the window's
//      whole 128-row blocks (rows past nr are zero like every row without a posting; ld covers whole blocks), and the maximum of each block.
// Integer adds commute: the result does not depend on the order the postings arrive in.  The host has refused every query whose score could
// reach 2^31 (include/lrx.h), so no accumulator wraps.
__global__ void __launch_bounds__(1024)
k_impact_scan(const imp_i32x2* __restrict__ post, const int64_t* __restrict__ term_off, int n_terms, int64_t r0, int64_t nr, int W,
              const int* __restrict__ q_off, const int* __restrict__ q_term, const int* __restrict__ q_cnt, float* __restrict__ scores, int64_t ld,
              float* __restrict__ blkmax, int nblk_ld) {
  extern __shared__ __attribute__((aligned(16))) int imp_acc[];
  __shared__ int64_t s_bnd[IMP_TCHUNK][2];
  __shared__ int s_cnt[IMP_TCHUNK];
  const int tid = threadIdx.x, NT = blockDim.x, qi = blockIdx.y;
  const int64_t w0 = (int64_t)blockIdx.x * W;                  // chunk-local first row of the window
  const int64_t w1 = w0 + W < nr ? w0 + W : nr;
  const int64_t base = r0 + w0;
  for (int i = tid * 4; i < W; i += NT * 4) *(imp_i32x4*)(imp_acc + i) = imp_i32x4{0, 0, 0, 0};
  const int t0 = q_off[qi], t1 = q_off[qi + 1];
  for (int tc = t0; tc < t1; tc += IMP_TCHUNK) {
    const int nt = t1 - tc < IMP_TCHUNK ? t1 - tc : IMP_TCHUNK;
    __syncthreads();                                           // the accumulators are zero / the previous pass has read its ranges
    for (int e = tid; e < 2 * nt; e += NT) {
      const int j = e >> 1, term = q_term[tc + j];
      int64_t b = 0;
      if ((unsigned)term < (unsigned)n_terms) b = imp_lower_bound(post, term_off[term], term_off[term + 1], r0 + ((e & 1) ? w1 : w0));
      s_bnd[j][e & 1] = b;                                     // (a term outside the index: the empty range [0, 0))
      if ((e & 1) == 0) s_cnt[j] = q_cnt[tc + j];
    }
    __syncthreads();
    for (int j = 0; j < nt; ++j) {
      const int64_t a = s_bnd[j][0], b = s_bnd[j][1];
      if (a >= b) continue;
      const int cnt = s_cnt[j];
      const int rt = (tid + 64 * j) & (NT - 1);                // (NT is a power of two)
      if (rt == 0 && (a & 1)) { const imp_i32x2 p = post[a]; imp_add(imp_acc, W, base, p[0], p[1], cnt); }
      if (rt == (64 & (NT - 1)) && (b & 1)) { const imp_i32x2 p = post[b - 1]; imp_add(imp_acc, W, base, p[0], p[1], cnt); }
      const int64_t a2 = (a + 1) & ~1ll, b2 = b & ~1ll;
      const int64_t np = b2 > a2 ? (b2 - a2) >> 1 : 0;
      const imp_i32x4* pp = (const imp_i32x4*)(post + a2);
      for (int64_t i = rt; i < np; i += 4 * (int64_t)NT) {
        imp_i32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i + (int64_t)u * NT < np) v[u] = pp[i + (int64_t)u * NT];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i + (int64_t)u * NT < np) {
            imp_add(imp_acc, W, base, v[u][0], v[u][1], cnt);
            imp_add(imp_acc, W, base, v[u][2], v[u][3], cnt);
          }
      }
    }
  }
  __syncthreads();
  const int64_t nr_blk = (nr + SP_ROWS - 1) / SP_ROWS * SP_ROWS;
  const int nw = (int)(w0 + W < nr_blk ? W : nr_blk - w0);     // a multiple of 128: a half-wave (32 lanes x 4 rows) covers one block
  float* srow = scores + (int64_t)qi * ld + w0;
  for (int i = tid * 4; i < nw; i += NT * 4) {
    const imp_i32x4 v = *(const imp_i32x4*)(imp_acc + i);
    const float f0 = (float)v[0], f1 = (float)v[1], f2 = (float)v[2], f3 = (float)v[3];
    *(float4*)(srow + i) = make_float4(f0, f1, f2, f3);
    float m = fmaxf(fmaxf(f0, f1), fmaxf(f2, f3));
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 31) == 0) blkmax[(int64_t)qi * nblk_ld + (w0 + i) / SP_ROWS] = m;
  }
}

__global__ void __launch_bounds__(256)
k_impact_hits(float* __restrict__ scores, int64_t* __restrict__ ids, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  if (!(scores[t] > 0.f)) { scores[t] = -FLT_MAX; ids[t] = -1; }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// (no regions of the format's own: the queries arrive on the device in CSR form)
static ScanPlan impact_plan(int64_t n_rows, int32_t n_queries, int32_t k) {
  return scan_plan(n_rows, n_queries, k, IMP_ROW_CHUNK, SP_ROWS, IMP_MATRIX_BYTES, IMP_QC_MAX, [](int) { return (size_t)0; });
}

// Rows per window of a scan of nr rows for nq queries: the largest of 32768 / 8192 / 2048 that still gives every CU two workgroups.  A
// larger window means fewer range searches per posting list and fewer, longer streams; a smaller one more workgroups per CU (its LDS share
// shrinks with it).  Measured: DESIGN §5.4.6.
static int impact_window_rows(int64_t nr, int nq, int ncu) {
  const int cand[3] = {IMP_MAX_W, 8192, 2048};
  for (int c = 0; c < 3; ++c)
    if (lrx_cdiv(nr, cand[c]) * nq >= 2 * (int64_t)ncu) return cand[c];
  return cand[2];
}

// The two steps the impact index hands to the scan drivers (scan_search and scan_range, lrx_search_codes.h): prep notes the chunk's first
// query (the queries are on the device already), scan is k_impact_scan over a row chunk.  One place for the window rule and the launch
// geometry of both the top-k and the range search.
struct ImpactSteps {
  const void* postings;
  const int64_t* term_off;
  int32_t n_terms;
  const int32_t *q_off, *q_term, *q_cnt;
  int32_t window_rows;
  int64_t ld;
  int nblk_ld;
  void* stream;
  int ncu;
  int32_t q0_cur;
  int init(const void* postings_, const int64_t* term_off_, int32_t n_terms_, const int32_t* q_off_, const int32_t* q_term_, const int32_t* q_cnt_,
           int32_t window_rows_, const ScanPlan& p, void* stream_) {
    postings = postings_; term_off = term_off_; n_terms = n_terms_; q_off = q_off_; q_term = q_term_; q_cnt = q_cnt_; window_rows = window_rows_;
    ld = p.ld; nblk_ld = p.nblk_ld; stream = stream_; q0_cur = 0;
    LRX_HIP(hipFuncSetAttribute((const void*)k_impact_scan, hipFuncAttributeMaxDynamicSharedMemorySize, IMP_MAX_W * 4));
    ncu = lrx_cu_count();
    return LRX_OK;
  }
  int prep(int32_t q0, int) { q0_cur = q0; return LRX_OK; }
  int scan(int64_t r0, int64_t nr, int nq, float* sc, float* bm) const {
    const int W = window_rows ? window_rows : impact_window_rows(nr, nq, ncu);
    const int threads = W >= IMP_MAX_W ? 1024 : (W >= 8192 ? 512 : 256);
    hipLaunchKernelGGL(k_impact_scan, dim3((unsigned)lrx_cdiv(nr, W), (unsigned)nq), dim3(threads), (size_t)W * 4, (hipStream_t)stream,
                       (const imp_i32x2*)postings, term_off, (int)n_terms, r0, nr, W, q_off + q0_cur, q_term, q_cnt, sc, ld, bm, nblk_ld);
    LRX_LAUNCH_CHECK();
    return LRX_OK;
  }
};

extern "C" size_t lrx_impact_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t k) { return impact_plan(n_rows, n_queries, k).total; }

extern "C" int32_t lrx_impact_chunk_queries(int64_t n_rows, int32_t n_queries, int32_t k) { return impact_plan(n_rows, n_queries, k).qc; }

extern "C" int lrx_impact_search(const void* postings, const int64_t* term_off, int32_t n_terms, int64_t n_rows, const int32_t* q_off,
                                 const int32_t* q_term, const int32_t* q_cnt, int32_t n_queries, int32_t k, int64_t id_base, float* out_scores,
                                 int64_t* out_ids, const int64_t* row_map, void* workspace, size_t workspace_bytes, int32_t window_rows,
                                 void* stream) {
  int rc = codes_check_topk("impact_search", k, n_rows);
  if (rc != LRX_OK) return rc;
  LRX_CHECK_ARG(n_rows < (1ll << 31), "impact_search: rows=%lld do not fit the postings' int32 row", (long long)n_rows);
  LRX_CHECK_ARG(n_terms >= 0 && (n_rows == 0 || n_terms == 0 || (postings != nullptr && term_off != nullptr)), "impact_search: null postings (terms=%d)",
                n_terms);
  LRX_CHECK_ARG(window_rows == 0 || (window_rows > 0 && window_rows <= IMP_MAX_W && window_rows % SP_ROWS == 0),
                "impact_search: window_rows=%d must be 0 (the library's rule) or a multiple of %d up to %d", window_rows, SP_ROWS, IMP_MAX_W);
  if (n_queries <= 0) return LRX_OK;
  LRX_CHECK_ARG(q_off != nullptr, "impact_search: null q_off (queries=%d)", n_queries);
  const ScanPlan p = impact_plan(n_rows, n_queries, k);
  if ((rc = codes_check_workspace("impact_search", workspace_bytes, p.total)) != LRX_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  ImpactSteps st;
  if ((rc = st.init(postings, term_off, n_terms, q_off, q_term, q_cnt, window_rows, p, stream)) != LRX_OK) return rc;
  return scan_search(
      p, workspace, n_rows, n_queries, k, id_base, out_scores, out_ids, row_map, stream,
      [&](int32_t q0, int nq) { return st.prep(q0, nq); },
      [&](int64_t r0, int64_t nr, int nq, float* sc, float* bm) { return st.scan(r0, nr, nq, sc, bm); },
      [&](int32_t, int64_t r0, int64_t nr, int nq, const float* sc, const float* bm, float* os, int64_t* oi) {
        hipLaunchKernelGGL(k_topk_select, dim3(nq), dim3(SEL_THREADS), 0, s, sc, p.ld, nr, k, r0, bm, (int)lrx_cdiv(nr, SP_ROWS), p.nblk_ld, os, oi,
                           (const int*)nullptr, (const int*)nullptr);
        LRX_LAUNCH_CHECK();
        const int64_t n_out = (int64_t)nq * k;
        hipLaunchKernelGGL(k_impact_hits, dim3((unsigned)lrx_cdiv(n_out, 256)), dim3(256), 0, s, os, oi, n_out);
        LRX_LAUNCH_CHECK();
        return LRX_OK;
      });
}

// ---- range search: every hit (S >= 1) with (float) S > radius, in row order (the contract of lrx_flat_ip_range_search; include/lrx.h) ----
static ScanRangePlan impact_range_plan(int64_t n_rows, int32_t n_queries, int64_t row_chunk) {
  return scan_range_plan(n_rows, n_queries, row_chunk > 0 ? row_chunk : IMP_ROW_CHUNK, SP_ROWS, IMP_MATRIX_BYTES, IMP_QC_MAX, [](int) { return (size_t)0; });
}

extern "C" size_t lrx_range_impact_workspace_bytes(int64_t n_rows, int32_t n_queries, int64_t row_chunk) {
  return impact_range_plan(n_rows, n_queries, row_chunk > 0 && row_chunk % SP_ROWS == 0 ? row_chunk : 0).p.total;
}

extern "C" int lrx_range_impact_search(const void* postings, const int64_t* term_off, int32_t n_terms, int64_t n_rows, const int32_t* q_off,
                                       const int32_t* q_term, const int32_t* q_cnt, int32_t n_queries, float radius, int64_t id_base, int64_t* lims,
                                       float* out_scores, int64_t* out_ids, int64_t capacity, void* workspace, size_t workspace_bytes, int32_t window_rows,
                                       void* stream, int64_t row_chunk) {
  int rc = codes_check_range("impact_range_search", n_rows, n_queries, radius, lims, out_scores, out_ids, capacity, row_chunk);
  if (rc != LRX_OK) return rc;
  LRX_CHECK_ARG(n_rows < (1ll << 31), "impact_range_search: rows=%lld do not fit the postings' int32 row", (long long)n_rows);
  LRX_CHECK_ARG(n_terms >= 0 && (n_rows == 0 || n_terms == 0 || (postings != nullptr && term_off != nullptr)), "impact_range_search: null postings (terms=%d)",
                n_terms);
  LRX_CHECK_ARG(window_rows == 0 || (window_rows > 0 && window_rows <= IMP_MAX_W && window_rows % SP_ROWS == 0),
                "impact_range_search: window_rows=%d must be 0 (the library's rule) or a multiple of %d up to %d", window_rows, SP_ROWS, IMP_MAX_W);
  hipStream_t s = (hipStream_t)stream;
  if (n_queries == 0 || n_rows == 0) {
    LRX_HIP(hipMemsetAsync(lims, 0, sizeof(int64_t) * ((size_t)n_queries + 1), s));
    return LRX_OK;
  }
  LRX_CHECK_ARG(q_off != nullptr, "impact_range_search: null q_off (queries=%d)", n_queries);
  const ScanRangePlan rp = impact_range_plan(n_rows, n_queries, row_chunk);
  if ((rc = codes_check_workspace("impact_range_search", workspace_bytes, rp.p.total)) != LRX_OK) return rc;
  ImpactSteps st;
  if ((rc = st.init(postings, term_off, n_terms, q_off, q_term, q_cnt, window_rows, rp.p, stream)) != LRX_OK) return rc;
  return scan_range(
      rp, workspace, n_rows, n_queries, id_base, lims, out_scores, out_ids, capacity, stream,
      [&](int32_t q0, int nq) { return st.prep(q0, nq); },
      [&](int64_t r0, int64_t nr, int nq, float* sc, float* bm) { return st.scan(r0, nr, nq, sc, bm); },
      KeepHitAbove{radius});
}
