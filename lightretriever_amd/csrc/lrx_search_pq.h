// liblrx search, part 6 -- PRODUCT-QUANTISED inner-product index (faiss IndexPQ(d, M, 8, METRIC_INNER_PRODUCT)), map: section G.
// Part of the ONE translation unit lrx_search.hip (included at its end, after lrx_search_codes.h: it reuses k_topk_select, lrx_cu_count and the
// shared plan, checks and scan driver).  Not a stand-alone header.  Contract and code layout: include/lrx.h (lrx_pq_ip_search), DESIGN.md §5.4.3.
//
//     k_pq_encode    code[m] = argmin_j sum_i (x_i - C[m][j][i])^2, fp64 terms summed in order, ties to the lower j (add() and k-means)
//     k_pq_lut       LUT[q][m][j] = (float) sum_i (double) q_i (double) C[m][j][i]
//     k_pq_scan      THE HOT PATH: s(q, r) = fp32 sum of LUT[q][m][code_m(r)] in ascending m, the query's table in LDS; writes the
//                    [Q, ld] score matrix of a row chunk and its 128-row block maxima -> k_topk_select (scan_search, lrx_search_codes.h)
//     k_pq_decode    rows from their codes (reconstruct_n)
// Range search (lrx_pq_ip_range_search): the same lookup tables and the same k_pq_scan under scan_range (lrx_search_codes.h) -- the matrix
// score is the reported score, the predicate is s > radius.
#pragma once

#define PQ_KSUB 256
#define PQ_BLK 128            // rows per code block
#define PQ_GRP 16             // sub-spaces per 16-byte piece of a row
#define PQ_SCAN_THREADS 1024  // one row per lane, 1024-row tiles (8 code blocks)
#define PQ_SCAN_MC 128        // sub-spaces whose tables sit in LDS at once (128 KiB); more are scanned in passes over the tile
#define PQ_ENC_ROWS 256
#define PQ_ENC_MAX_DSUB 64
#define PQ_ROW_CHUNK (1ll << 22)       // rows per score matrix (16 MiB per query)
#define PQ_MATRIX_BYTES (1ll << 30)    // score matrix budget of one query chunk
#define PQ_QC_MAX 65535                // queries per chunk at most (grid.y of k_pq_scan)

static __host__ __device__ __forceinline__ int pq_mp(int M) { return (M + PQ_GRP - 1) / PQ_GRP * PQ_GRP; }
// byte offset of code m of row r in the blocked layout (include/lrx.h): block r / 128, 16-sub-space group m / 16, row r % 128, byte m % 16
static __host__ __device__ __forceinline__ int64_t pq_code_off(int64_t r, int m, int Mp) {
  return (r / PQ_BLK) * PQ_BLK * Mp + (int64_t)(m / PQ_GRP) * (PQ_BLK * PQ_GRP) + (r % PQ_BLK) * PQ_GRP + (m % PQ_GRP);
}

// One thread per (row, sub-space): the sub-space's 256 x dsub centroids and the workgroup's 256 row pieces are staged in LDS (row pieces
// padded by one float: lane t reads row t's piece, stride dsub + 1 keeps the banks apart; centroid reads are broadcasts).  The distance is
// formed exactly as the contract writes it: fp64 subtract, square, add, in order over i -- no contraction (a fused multiply-add would round
// differently from numpy's separate operations), so the codes equal the numpy yardstick's bit for bit.
__global__ void __launch_bounds__(PQ_ENC_ROWS)
k_pq_encode(const float* __restrict__ X, int64_t n_rows, int64_t ldx, const float* __restrict__ C, int dsub, int Mp,
            uint8_t* __restrict__ codes, int64_t row0) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float pq_enc_smem[];
  float* Cs = pq_enc_smem;                          // [256][dsub]
  float* Xs = pq_enc_smem + PQ_KSUB * dsub;         // [256][dsub + 1]
  const int m = blockIdx.y, tid = threadIdx.x;
  const int64_t r_base = (int64_t)blockIdx.x * PQ_ENC_ROWS;
  const float* Cm = C + (int64_t)m * PQ_KSUB * dsub;
  for (int e = tid; e < PQ_KSUB * dsub; e += PQ_ENC_ROWS) Cs[e] = Cm[e];
  for (int e = tid; e < PQ_ENC_ROWS * dsub; e += PQ_ENC_ROWS) {
    const int rr = e / dsub, i = e - rr * dsub;
    const int64_t r = r_base + rr;
    Xs[rr * (dsub + 1) + i] = r < n_rows ? X[r * ldx + (int64_t)m * dsub + i] : 0.f;
  }
  __syncthreads();
  const int64_t r = r_base + tid;
  if (r >= n_rows) return;
  const float* xr = Xs + tid * (dsub + 1);
  double best = 0.0;
  int bj = 0;
  for (int j = 0; j < PQ_KSUB; ++j) {
    const float* cj = Cs + j * dsub;
    double acc = 0.0;
    for (int i = 0; i < dsub; ++i) {
      const double t = (double)xr[i] - (double)cj[i];
      acc = acc + t * t;
    }
    if (j == 0 || acc < best) { best = acc; bj = j; }   // strict: ties keep the lower j
  }
  codes[pq_code_off(row0 + r, m, Mp)] = (uint8_t)bj;
}

// One thread per (query, sub-space, centroid).  The fp32 x fp32 products are exact in fp64, so a contracted fma(q, c, acc) rounds exactly
// like acc + q * c: contraction cannot change the table.  The sum runs in order over i, one final rounding to fp32.
__global__ void __launch_bounds__(256)
k_pq_lut(const float* __restrict__ q, int nq, const float* __restrict__ C, int dim, int M, int dsub, float* __restrict__ lut) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nq * M * PQ_KSUB) return;
  const int j = (int)(t % PQ_KSUB);
  const int m = (int)((t / PQ_KSUB) % M);
  const int qi = (int)(t / ((int64_t)PQ_KSUB * M));
  const float* qm = q + (int64_t)qi * dim + (int64_t)m * dsub;
  const float* cj = C + ((int64_t)m * PQ_KSUB + j) * dsub;
  double acc = 0.0;
  for (int i = 0; i < dsub; ++i) acc += (double)qm[i] * (double)cj[i];
  lut[t] = (float)acc;
}

// The ADC scan.  Grid (gx, queries): workgroup (x, q) keeps query q's table -- up to PQ_SCAN_MC sub-spaces of it, 1 KiB each -- in LDS and
// walks the 1024-row tiles x, x + gx, ...; lane t scores row 1024 tile + t.  Its codes are one 16-byte load per 16 sub-spaces (64 lanes:
// 1 KiB contiguous, the next group prefetched while the current one is looked up); the score is ((0 + LUT[0][c0]) + LUT[1][c1]) + ... in
// ascending m, fp32.  More than PQ_SCAN_MC sub-spaces: the table is loaded in passes per tile and the partial sum stays in a register, so
// the order of the adds is the same.  Writes scores[q][r] for r < n_rows and the maximum of every 128-row block over its valid rows.
__global__ void __launch_bounds__(PQ_SCAN_THREADS)
k_pq_scan(const uint8_t* __restrict__ codes, int64_t n_rows, int M, int Mp, const float* __restrict__ lut, float* __restrict__ scores, int64_t ld,
          float* __restrict__ blkmax, int nblk_ld) {
  extern __shared__ __attribute__((aligned(16))) float pq_lut_s[];
  __shared__ float wmax[PQ_SCAN_THREADS / 64];
  const int tid = threadIdx.x, qi = blockIdx.y;
  const float* lq = lut + (int64_t)qi * M * PQ_KSUB;
  const int mc = M < PQ_SCAN_MC ? M : PQ_SCAN_MC;
  const bool one_pass = mc == M;
  const int64_t ntiles = (n_rows + PQ_SCAN_THREADS - 1) / PQ_SCAN_THREADS;
  if (one_pass) {
    for (int e = tid * 4; e < M * PQ_KSUB; e += PQ_SCAN_THREADS * 4) *(float4*)(pq_lut_s + e) = *(const float4*)(lq + e);
    __syncthreads();
  }
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * PQ_SCAN_THREADS + tid;
    const bool valid = r < n_rows;
    const uint8_t* rc = codes + (r / PQ_BLK) * PQ_BLK * Mp + (r % PQ_BLK) * PQ_GRP;
    float acc = 0.f;
    for (int m0 = 0; m0 < M; m0 += mc) {
      const int m1 = m0 + mc < M ? m0 + mc : M;
      if (!one_pass) {
        __syncthreads();
        for (int e = tid * 4; e < (m1 - m0) * PQ_KSUB; e += PQ_SCAN_THREADS * 4)
          *(float4*)(pq_lut_s + e) = *(const float4*)(lq + (int64_t)m0 * PQ_KSUB + e);
        __syncthreads();
      }
      if (valid) {
        uint4 cur = *(const uint4*)(rc + (int64_t)(m0 / PQ_GRP) * (PQ_BLK * PQ_GRP));
        for (int g = m0; g < m1; g += PQ_GRP) {
          uint4 nxt = cur;
          if (g + PQ_GRP < m1) nxt = *(const uint4*)(rc + (int64_t)((g + PQ_GRP) / PQ_GRP) * (PQ_BLK * PQ_GRP));
          const float* tg = pq_lut_s + (g - m0) * PQ_KSUB;
          const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
          if (g + PQ_GRP <= m1) {
#pragma unroll
            for (int u = 0; u < PQ_GRP; ++u) acc += tg[u * PQ_KSUB + ((w[u >> 2] >> (8 * (u & 3))) & 255u)];
          } else {                                     // (M % 16 != 0: the last group's padding bytes are not sub-spaces)
#pragma unroll
            for (int u = 0; u < PQ_GRP; ++u)
              if (g + u < m1) acc += tg[u * PQ_KSUB + ((w[u >> 2] >> (8 * (u & 3))) & 255u)];
          }
          cur = nxt;
        }
      }
    }
    if (valid) scores[(int64_t)qi * ld + r] = acc;
    const float wm = wave_max(valid ? acc : -INFINITY);
    if ((tid & 63) == 0) wmax[tid >> 6] = wm;
    __syncthreads();
    if (tid < PQ_SCAN_THREADS / PQ_BLK) {
      const int64_t b = tile * (PQ_SCAN_THREADS / PQ_BLK) + tid;
      if (b * PQ_BLK < n_rows) blkmax[(int64_t)qi * nblk_ld + b] = fmaxf(wmax[2 * tid], wmax[2 * tid + 1]);
    }
    __syncthreads();
  }
}

// out[i * ldo + m * dsub + e] = C[m][code_m(row0 + i)][e]: one thread per output element.
__global__ void __launch_bounds__(256)
k_pq_decode(const uint8_t* __restrict__ codes, int64_t row0, int64_t n_rows, const float* __restrict__ C, int dim, int dsub, int Mp,
            float* __restrict__ out, int64_t ldo) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * dim) return;
  const int64_t i = t / dim;
  const int col = (int)(t - i * dim), m = col / dsub;
  const int c = codes[pq_code_off(row0 + i, m, Mp)];
  out[i * ldo + col] = C[((int64_t)m * PQ_KSUB + c) * dsub + (col - m * dsub)];
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// the leading region of the workspace is the chunk's lookup tables [qc, M, 256] fp32
static ScanPlan pq_plan(int64_t n_rows, int32_t M, int32_t n_queries, int32_t k) {
  return scan_plan(n_rows, n_queries, k, PQ_ROW_CHUNK, 64, PQ_MATRIX_BYTES, PQ_QC_MAX, [&](int qc) { return align256((size_t)qc * M * PQ_KSUB * 4); });
}

extern "C" size_t lrx_pq_ip_workspace_bytes(int64_t n_rows, int32_t dim, int32_t M, int32_t n_queries, int32_t k) {
  (void)dim;
  return pq_plan(n_rows, M > 0 ? M : 1, n_queries, k).total;
}

extern "C" int32_t lrx_pq_ip_chunk_queries(int64_t n_rows, int32_t dim, int32_t M, int32_t n_queries, int32_t k) {
  (void)dim;
  return pq_plan(n_rows, M > 0 ? M : 1, n_queries, k).qc;
}

extern "C" int lrx_pq_lut(const float* q, int32_t n_queries, const float* centroids, int32_t dim, int32_t M, float* lut, void* stream) {
  LRX_CHECK_ARG(M > 0 && dim > 0 && dim % M == 0, "pq_lut: dim=%d is not a multiple of M=%d", dim, M);
  if (n_queries <= 0) return LRX_OK;
  const int64_t n = (int64_t)n_queries * M * PQ_KSUB;
  hipLaunchKernelGGL(k_pq_lut, dim3((unsigned)lrx_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, q, n_queries, centroids, dim, M, dim / M, lut);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

// The two steps PQ hands to the scan drivers (scan_search and scan_range, lrx_search_codes.h): the chunk's lookup tables into the head of the
// workspace, and k_pq_scan over a row chunk.  One place for the launch geometry of both the top-k and the range search.
struct PqSteps {
  const void* codes;
  const float* centroids;
  const float* q;
  int32_t dim, M;
  float* lut;
  int64_t ld;
  int nblk_ld;
  void* stream;
  int Mp, ncu;
  size_t smem;
  int init(const void* codes_, const float* centroids_, const float* q_, int32_t dim_, int32_t M_, void* workspace, const ScanPlan& p, void* stream_) {
    codes = codes_; centroids = centroids_; q = q_; dim = dim_; M = M_; lut = (float*)workspace; ld = p.ld; nblk_ld = p.nblk_ld; stream = stream_;
    Mp = pq_mp(M);
    smem = (size_t)(M < PQ_SCAN_MC ? M : PQ_SCAN_MC) * PQ_KSUB * 4;
    LRX_HIP(hipFuncSetAttribute((const void*)k_pq_scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    ncu = lrx_cu_count();
    return LRX_OK;
  }
  int prep(int32_t q0, int nq) const { return lrx_pq_lut(q + (int64_t)q0 * dim, nq, centroids, dim, M, lut, stream); }
  int scan(int64_t r0, int64_t nr, int nq, float* sc, float* bm) const {
    const int64_t ntiles = lrx_cdiv(nr, PQ_SCAN_THREADS);
    int64_t gx = lrx_cdiv(2 * (int64_t)ncu, nq);
    gx = gx > ntiles ? ntiles : gx;
    hipLaunchKernelGGL(k_pq_scan, dim3((unsigned)gx, (unsigned)nq), dim3(PQ_SCAN_THREADS), smem, (hipStream_t)stream,
                       (const uint8_t*)codes + (r0 / PQ_BLK) * PQ_BLK * Mp, nr, M, Mp, (const float*)lut, sc, ld, bm, nblk_ld);
    LRX_LAUNCH_CHECK();
    return LRX_OK;
  }
};

extern "C" int lrx_pq_ip_search(const void* codes, int64_t n_rows, const float* centroids, int32_t dim, int32_t M, const float* q, int32_t n_queries,
                                int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace,
                                size_t workspace_bytes, int32_t flags, void* stream) {
  (void)flags;
  int rc = codes_check_topk("pq_ip_search", k, n_rows);
  if (rc != LRX_OK) return rc;
  LRX_CHECK_ARG(M > 0 && dim > 0 && dim % M == 0, "pq_ip_search: dim=%d is not a multiple of M=%d", dim, M);
  if (n_queries <= 0) return LRX_OK;
  const ScanPlan p = pq_plan(n_rows, M, n_queries, k);
  if ((rc = codes_check_workspace("pq_ip_search", workspace_bytes, p.total)) != LRX_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  PqSteps st;
  if ((rc = st.init(codes, centroids, q, dim, M, workspace, p, stream)) != LRX_OK) return rc;
  return scan_search(
      p, workspace, n_rows, n_queries, k, id_base, out_scores, out_ids, row_map, stream,
      [&](int32_t q0, int nq) { return st.prep(q0, nq); },
      [&](int64_t r0, int64_t nr, int nq, float* sc, float* bm) { return st.scan(r0, nr, nq, sc, bm); },
      [&](int32_t, int64_t r0, int64_t nr, int nq, const float* sc, const float* bm, float* os, int64_t* oi) {
        hipLaunchKernelGGL(k_topk_select, dim3(nq), dim3(SEL_THREADS), 0, s, sc, p.ld, nr, k, r0, bm, (int)lrx_cdiv(nr, PQ_BLK), p.nblk_ld, os, oi,
                           (const int*)nullptr, (const int*)nullptr);
        LRX_LAUNCH_CHECK();
        return LRX_OK;
      });
}

// ---- range search: every row with s(q, r) > radius (the contract of lrx_flat_ip_range_search; include/lrx.h) ----
static ScanRangePlan pq_range_plan(int64_t n_rows, int32_t M, int32_t n_queries, int64_t row_chunk) {
  return scan_range_plan(n_rows, n_queries, row_chunk > 0 ? row_chunk : PQ_ROW_CHUNK, 64, PQ_MATRIX_BYTES, PQ_QC_MAX,
                         [&](int qc) { return align256((size_t)qc * M * PQ_KSUB * 4); });
}

extern "C" size_t lrx_pq_ip_range_workspace_bytes(int64_t n_rows, int32_t dim, int32_t M, int32_t n_queries, int64_t row_chunk) {
  (void)dim;
  return pq_range_plan(n_rows, M > 0 ? M : 1, n_queries, row_chunk > 0 && row_chunk % SP_ROWS == 0 ? row_chunk : 0).p.total;
}

extern "C" int lrx_pq_ip_range_search(const void* codes, int64_t n_rows, const float* centroids, int32_t dim, int32_t M, const float* q, int32_t n_queries,
                                      float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity, void* workspace,
                                      size_t workspace_bytes, void* stream, int64_t row_chunk) {
  int rc = codes_check_range("pq_ip_range_search", n_rows, n_queries, radius, lims, out_scores, out_ids, capacity, row_chunk);
  if (rc != LRX_OK) return rc;
  LRX_CHECK_ARG(M > 0 && dim > 0 && dim % M == 0, "pq_ip_range_search: dim=%d is not a multiple of M=%d", dim, M);
  hipStream_t s = (hipStream_t)stream;
  if (n_queries == 0 || n_rows == 0) {
    LRX_HIP(hipMemsetAsync(lims, 0, sizeof(int64_t) * ((size_t)n_queries + 1), s));
    return LRX_OK;
  }
  LRX_CHECK_ARG(codes != nullptr && centroids != nullptr && q != nullptr, "pq_ip_range_search: null codes / centroids / queries");
  const ScanRangePlan rp = pq_range_plan(n_rows, M, n_queries, row_chunk);
  if ((rc = codes_check_workspace("pq_ip_range_search", workspace_bytes, rp.p.total)) != LRX_OK) return rc;
  PqSteps st;
  if ((rc = st.init(codes, centroids, q, dim, M, workspace, rp.p, stream)) != LRX_OK) return rc;
  return scan_range(
      rp, workspace, n_rows, n_queries, id_base, lims, out_scores, out_ids, capacity, stream,
      [&](int32_t q0, int nq) { return st.prep(q0, nq); },
      [&](int64_t r0, int64_t nr, int nq, float* sc, float* bm) { return st.scan(r0, nr, nq, sc, bm); },
      KeepAbove{radius});
}

extern "C" int lrx_pq_encode(const float* x, int64_t n_rows, int64_t ldx, const float* centroids, int32_t dim, int32_t M, void* codes, int64_t row0,
                             void* stream) {
  LRX_CHECK_ARG(M > 0 && dim > 0 && dim % M == 0, "pq_encode: dim=%d is not a multiple of M=%d", dim, M);
  LRX_CHECK_ARG(dim / M <= PQ_ENC_MAX_DSUB, "pq_encode: dsub=%d > %d is not served", dim / M, PQ_ENC_MAX_DSUB);
  LRX_CHECK_ARG(n_rows >= 0 && row0 >= 0 && ldx >= dim, "pq_encode: bad rows (n_rows=%lld, row0=%lld, ldx=%lld)", (long long)n_rows,
                (long long)row0, (long long)ldx);
  if (n_rows == 0) return LRX_OK;
  const int dsub = dim / M;
  const size_t smem = ((size_t)PQ_KSUB * dsub + (size_t)PQ_ENC_ROWS * (dsub + 1)) * 4;
  LRX_HIP(hipFuncSetAttribute((const void*)k_pq_encode, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(k_pq_encode, dim3((unsigned)lrx_cdiv(n_rows, PQ_ENC_ROWS), (unsigned)M), dim3(PQ_ENC_ROWS), smem, (hipStream_t)stream, x, n_rows,
                     ldx, centroids, dsub, pq_mp(M), (uint8_t*)codes, row0);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_pq_decode_rows(const void* codes, int64_t row0, int64_t n_rows, const float* centroids, int32_t dim, int32_t M, float* out,
                                  int64_t ldo, void* stream) {
  LRX_CHECK_ARG(M > 0 && dim > 0 && dim % M == 0 && ldo >= dim, "pq_decode_rows: dim=%d, M=%d, ldo=%lld", dim, M, (long long)ldo);
  if (n_rows <= 0) return LRX_OK;
  const int64_t n = n_rows * dim;
  hipLaunchKernelGGL(k_pq_decode, dim3((unsigned)lrx_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, row0, n_rows, centroids,
                     dim, dim / M, pq_mp(M), out, ldo);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}
