// liblrx search, part K -- RERANK: exact rescoring of a CALLER's candidate rows (faiss IndexRefineFlat's second stage): k_rerank_score,
// k_rerank_merge, lrx_flat_ip_rerank / lrx_sq_fp16_ip_rerank (contract: include/lrx.h).
// Part of the ONE translation unit lrx_search.hip (included at its end: it reuses refine_rescore / row_dot, the sorts and lrx_cu_count).  Not a
// stand-alone header.
#pragma once

#define RERANK_MAX_CAND 2048              // candidates per query: the most any base search here delivers (SEL_MAXK)
#define RERANK_MAX_SPLIT 16               // workgroups per query of the scoring step

// Candidate entries >= n_rows the rerank skipped since the last reset: part of lrx_device_error_count (lrx_elementwise.hip).
__device__ unsigned int g_rerank_bad_rows = 0;
unsigned int lrx_rerank_bad_rows(int* ok, int reset) {
  unsigned int v = 0;
  *ok = hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_rerank_bad_rows), sizeof(v)) == hipSuccess;
  if (*ok && reset && v) {
    const unsigned int z = 0;
    *ok = hipMemcpyToSymbol(HIP_SYMBOL(g_rerank_bad_rows), &z, sizeof(z)) == hipSuccess;
  }
  return v;
}

// Scoring step, grid (n_queries, nsplit): part s of query q takes candidates s, s + nsplit, ... of the query's list, drops the entries that
// name no row (< 0: the base search's padding; >= N: never dereferenced, counted), rescores the others exactly -- one half-wave per row, the
// random 8-KiB-row gather of refine_rescore (lrx_search_refine.h) -- and publishes the packed (score, row) words with their count.  The order
// in which a part lists its rows is not fixed (an LDS counter); k_rerank_merge sorts, so the result does not depend on it or on nsplit.
template <int RS>
__global__ void __launch_bounds__(1024)
k_rerank_score(const float* __restrict__ X, int64_t N, int64_t ldx, int D, const float* __restrict__ q, const int64_t* __restrict__ cand, int n_cand,
               int64_t ld_cand, unsigned long long* __restrict__ parts, int* __restrict__ part_cnt, int nsplit, int pcap) {
  __shared__ unsigned long long s_cand[RERANK_MAX_CAND];         // (a part holds at most pcap = ceil(n_cand / nsplit) of them)
  __shared__ __attribute__((aligned(16))) float s_q[REF_QLDS];   // the query row (every rescoring re-reads it; from global its loads serialise)
  __shared__ unsigned int s_ncand, s_bad;
  const int tid = threadIdx.x;
  const int qi = blockIdx.x, part = blockIdx.y;
  const float* qglob = q + (int64_t)qi * D;
  const float* qrow = D <= REF_QLDS ? s_q : qglob;
  if (D <= REF_QLDS)
    for (int i = tid; i < D; i += 1024) s_q[i] = qglob[i];
  if (tid == 0) { s_ncand = 0; s_bad = 0; }
  __syncthreads();
  const int64_t* list = cand + (int64_t)qi * ld_cand;
  for (int j = part + nsplit * tid; j < n_cand; j += nsplit * 1024) {
    const int64_t row = list[j];
    if (row < 0) continue;
    if (row >= N) atomicAdd(&s_bad, 1u);
    else s_cand[atomicAdd(&s_ncand, 1u)] = (unsigned long long)row;      // (at most pcap entries: the part looks at no more)
  }
  __syncthreads();
  const int nc = (int)s_ncand;
  refine_rescore<RS>(X, ldx, D, qrow, s_cand, nc, parts + ((int64_t)qi * nsplit + part) * pcap);
  if (tid == 0) {
    part_cnt[qi * nsplit + part] = nc;
    if (s_bad) atomicAdd(&g_rerank_bad_rows, s_bad);
  }
}

// Merge of a query's published lists (one workgroup per query; the kernel boundary orders it after the scoring step): sort the words --
// (score desc, row asc), the order of k_refine_merge / lrx_merge_topk -- and write the top k, (-FLT_MAX, -1) beyond the valid candidates.
// A row named twice is two equal words and is reported twice.
__global__ void __launch_bounds__(1024)
k_rerank_merge(const unsigned long long* __restrict__ parts, const int* __restrict__ part_cnt, int k, int64_t id_base, const int64_t* __restrict__ row_map,
               float* __restrict__ out_scores, int64_t* __restrict__ out_ids, int nsplit, int pcap) {
  __shared__ unsigned long long s_cand[RERANK_MAX_CAND];
  __shared__ int s_off[RERANK_MAX_SPLIT + 1];
  const int tid = threadIdx.x, qi = blockIdx.x;
  float* os = out_scores + (int64_t)qi * k;
  int64_t* oi = out_ids + (int64_t)qi * k;
  if (tid == 0) {
    int run = 0;
    for (int p = 0; p < nsplit; ++p) { s_off[p] = run; run += part_cnt[qi * nsplit + p]; }
    s_off[nsplit] = run;
  }
  __syncthreads();
  const int tot = s_off[nsplit];                       // <= n_cand <= RERANK_MAX_CAND
  for (int p = 0; p < nsplit; ++p) {
    const unsigned long long* src = parts + ((int64_t)qi * nsplit + p) * pcap;
    const int base = s_off[p], n = s_off[p + 1] - base;
    for (int i = tid; i < n; i += 1024) s_cand[base + i] = src[i];
  }
  for (int i = tot + tid; i < k; i += 1024) { os[i] = -FLT_MAX; oi[i] = -1; }
  __syncthreads();
  auto put = [&](int r, unsigned long long c) {
    const int64_t row = sel_row(c);
    os[r] = key2f((uint32_t)(c >> 32));
    oi[r] = row_map != nullptr ? row_map[row] : id_base + row;
  };
  if (tot <= 1024) {
    // rank by counting, as k_refine_merge does for its short lists; equal words (a row named twice) take consecutive ranks by list position
    if (tid < tot) {
      const unsigned long long me = s_cand[tid];
      int r = 0;
      for (int j = 0; j < tot; ++j) {
        const unsigned long long o = s_cand[j];
        r += (o > me || (o == me && j < tid)) ? 1 : 0;
      }
      if (r < k) put(r, me);
    }
    return;
  }
  for (int i = tot + tid; i < RERANK_MAX_CAND; i += 1024) s_cand[i] = 0ull;
  bitonic_sort_desc_regs<2>(s_cand, RERANK_MAX_CAND);  // (loads after its own barrier: the zero fill above is seen)
  const int n_out = tot < k ? tot : k;
  for (int i = tid; i < n_out; i += 1024) put(i, s_cand[i]);
}

// workgroups per query of the scoring step: the 1024-thread workgroups run one per CU, so parts beyond the CU count only queue; a part
// keeps at least one row per half-wave (32)
static int rerank_split(int32_t n_queries, int32_t n_cand) {
  int s = lrx_cu_count() / (n_queries > 0 ? n_queries : 1);
  const int by_rows = (n_cand + 31) / 32;
  s = s < by_rows ? s : by_rows;
  return s < 1 ? 1 : (s > RERANK_MAX_SPLIT ? RERANK_MAX_SPLIT : s);
}

// words[n_queries * (n_cand + RERANK_MAX_SPLIT)] | counts[n_queries * RERANK_MAX_SPLIT]: enough for any split (nsplit * ceil(n_cand / nsplit)
// < n_cand + nsplit), so the size depends on the arguments alone
extern "C" size_t lrx_ip_rerank_workspace_bytes(int32_t n_queries, int32_t n_cand, int32_t k) {
  (void)k;
  const size_t nq = n_queries > 0 ? (size_t)n_queries : 1, nc = n_cand > 0 ? (size_t)n_cand : 1;
  return align256(nq * (nc + RERANK_MAX_SPLIT) * 8) + align256(nq * RERANK_MAX_SPLIT * sizeof(int));
}

template <int RS>
static int rerank_launch(const char* who, const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const float* q, int32_t n_queries,
                         const int64_t* cand_rows, int32_t n_cand, int64_t ld_cand, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids,
                         const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream) {
  LRX_CHECK_ARG(n_cand >= 1 && n_cand <= RERANK_MAX_CAND && k >= 1 && k <= n_cand, "%s: need 1 <= k <= n_cand <= %d, got k=%d, n_cand=%d", who,
                RERANK_MAX_CAND, k, n_cand);
  LRX_CHECK_ARG(ld_cand >= n_cand, "%s: ld_cand=%lld < n_cand=%d", who, (long long)ld_cand, n_cand);
  LRX_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 32), "%s: rows=%lld out of range", who, (long long)n_rows);
  LRX_CHECK_ARG(n_queries >= 0, "%s: n_queries=%d", who, n_queries);
  if (n_queries == 0) return LRX_OK;
  LRX_CHECK_ARG(q != nullptr && cand_rows != nullptr && out_scores != nullptr && out_ids != nullptr && (X != nullptr || n_rows == 0), "%s: null pointer", who);
  LRX_CHECK_ARG((uintptr_t)q % 16 == 0, "%s: q must be 16-byte aligned", who);
  const size_t need = lrx_ip_rerank_workspace_bytes(n_queries, n_cand, k);
  if (workspace == nullptr || workspace_bytes < need) {
    lrx_set_error("%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
    return LRX_ERR_WORKSPACE;
  }
  const int nsplit = rerank_split(n_queries, n_cand);
  const int pcap = (n_cand + nsplit - 1) / nsplit;
  unsigned long long* parts = (unsigned long long*)workspace;
  int* part_cnt = (int*)((char*)workspace + align256((size_t)n_queries * ((size_t)n_cand + RERANK_MAX_SPLIT) * 8));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rerank_score<RS>, dim3(n_queries, nsplit), dim3(1024), 0, s, X, n_rows, ldx, (int)dim, q, cand_rows, (int)n_cand, ld_cand, parts,
                     part_cnt, nsplit, pcap);
  LRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rerank_merge, dim3(n_queries), dim3(1024), 0, s, (const unsigned long long*)parts, (const int*)part_cnt, (int)k, id_base, row_map,
                     out_scores, out_ids, nsplit, pcap);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_flat_ip_rerank(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const float* q, int32_t n_queries, const int64_t* cand_rows,
                                  int32_t n_cand, int64_t ld_cand, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  LRX_CHECK_ARG(dim > 0 && dim % 4 == 0, "flat_ip_rerank: dim=%d must be a positive multiple of 4", dim);
  LRX_CHECK_ARG(ldx >= dim && ldx % 4 == 0 && (uintptr_t)X % 16 == 0, "flat_ip_rerank: rows must be 16-byte aligned (ldx=%lld >= dim=%d, ldx %% 4 == 0)",
                (long long)ldx, dim);
  return rerank_launch<ROWS_F32>("flat_ip_rerank", X, n_rows, ldx, dim, q, n_queries, cand_rows, n_cand, ld_cand, k, id_base, out_scores, out_ids, row_map,
                                 workspace, workspace_bytes, stream);
}

extern "C" int lrx_sq_fp16_ip_rerank(const void* codes, int64_t n_rows, int32_t dim, const float* q, int32_t n_queries, const int64_t* cand_rows,
                                     int32_t n_cand, int64_t ld_cand, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids,
                                     const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream) {
  LRX_CHECK_ARG(dim > 0 && dim % 64 == 0, "sq_fp16_ip_rerank: dim=%d must be a positive multiple of 64", dim);
  return rerank_launch<ROWS_F16T>("sq_fp16_ip_rerank", (const float*)codes, n_rows, dim, dim, q, n_queries, cand_rows, n_cand, ld_cand, k, id_base,
                                  out_scores, out_ids, row_map, workspace, workspace_bytes, stream);
}
