// liblrx search, part M -- INVERTED FILE over PRODUCT-QUANTISED codes (faiss IndexIVFPQ, inner product): the top k under the ADC score over
// the rows of the cells a query probes.  k_ivf_pq_scan, lrx_ivf_pq_ip_search (contract: include/lrx.h).
// Part of the ONE translation unit lrx_search.hip (included at its end, after lrx_search_ivf.h: it reuses k_pq_lut and the blocked code layout
// of lrx_search_pq.h, and k_ivf_plan / k_ivf_select, the chunking and the error counter of lrx_search_ivf.h).  Not a stand-alone header.
//
// A call walks its queries in chunks; per chunk, on one stream, four kernels and nothing else:
//   k_pq_lut          the chunk's lookup tables [queries, M, 256] fp32 into the head of the workspace (unchanged)
//   k_ivf_plan<true>  one workgroup per query: the probe list checked as the flat index's plan checks it, and a DENSE offset per slot -- where
//                     the slot's cell starts in the query's segment of score words; a skipped slot holds no words
//   k_ivf_pq_scan     QUERY-MAJOR: the large operand of a PQ scan is the query's table (M KiB), the codes are small (M bytes per row), so a
//                     workgroup keeps ONE query's table in LDS and walks 1024-position tiles of that query's segment -- the concatenation of
//                     its probed non-empty cells in probe order
//   k_ivf_select      one workgroup per query: sorted top k of its segment (unchanged); lrx_ivf_pq_ip_range_search ends the chunk with
//                     k_ivf_range<false>, k_range_lims and k_ivf_range<true> instead (lrx_search_ivf.h)
// Nothing needs zeroing (the dense plan emits no pairs and no counts), so there is no clear kernel and no memset.  Every size depends on the
// arguments alone; nothing is read back to the host.
#pragma once

#define IVFPQ_TILE PQ_SCAN_THREADS        // positions per tile: one per lane

// The scan.  Grid (gx, queries of the chunk): workgroup (x, q) holds query q's slot table (offset, cell, base term: at most 2048 entries) and
// lookup table -- up to PQ_SCAN_MC sub-spaces of it at once -- in LDS and walks the tiles x, x + gx, ... of the query's segment.  Lane t of a
// tile owns segment position s = 1024 tile + t:
//   slot j          the last slot with off[j] <= s: a binary search in LDS.  Offsets ascend and a skipped slot shares its successor's, so j is
//                   the one non-empty slot that holds s.
//   stored position p = list_off[cell_j] + (s - off[j]); lanes next to each other inside a cell are rows next to each other, so the 16-byte
//                   code pieces of a wave are one contiguous KiB wherever the cell starts inside its 128-row block.
//   score           acc = base_j (the caller's coarse score of the cell, or 0.f), then acc += LUT[m][code_m(p)] for m = 0 .. M - 1, fp32, in
//                   order; more than PQ_SCAN_MC sub-spaces: the table is loaded in passes per tile and acc stays in its register, so the
//                   order of the adds is the same.  The lookups are k_pq_scan's, its M % 16 != 0 tail included.
// The lane writes sel_pack(score, original row) to words[q * max_scan + s]; a position outside [0, n_rows) or an original row outside it
// becomes a word of 0 (nobody's row: the selection drops it) and is counted.  No position outside [0, n_rows) is read.
// SEL (the *_sel entries): `sel` is a row selector's bitmap over the original rows (lrx_search_selector.h); the lane tests the bit
// of its position's original row BEFORE the adds and, when the row is deselected, does none and writes the null word 0ull (the words are not
// cleared between calls).  The table passes and their barriers stay workgroup-uniform.  SEL = false is the scan without a selector, unchanged.
template <bool SEL>
__global__ void __launch_bounds__(PQ_SCAN_THREADS)
k_ivf_pq_scan(const uint8_t* __restrict__ codes, int64_t n_rows, int M, int Mp, const float* __restrict__ lut, const int64_t* __restrict__ probes,
              const float* __restrict__ probe_scores, int nprobe, int64_t ld_probe, const int64_t* __restrict__ list_off,
              const int64_t* __restrict__ row_ids, int nlist, const unsigned int* __restrict__ seg_off, const int64_t* __restrict__ q_tot,
              int64_t max_scan, unsigned long long* __restrict__ words, const uint32_t* __restrict__ sel) {
  extern __shared__ __attribute__((aligned(16))) float ivfpq_lut_s[];
  __shared__ unsigned int s_off[IVF_MAX_NPROBE];
  __shared__ int s_cell[IVF_MAX_NPROBE];
  __shared__ float s_base[IVF_MAX_NPROBE];
  const int tid = threadIdx.x, qi = blockIdx.y;
  const int64_t tot = q_tot[qi];
  const int64_t ntiles = (tot + IVFPQ_TILE - 1) / IVFPQ_TILE;
  if ((int64_t)blockIdx.x >= ntiles) return;                 // (workgroup-uniform; covers tot <= 0: nothing probed, or over max_scan)
  const float* lq = lut + (int64_t)qi * M * PQ_KSUB;
  const int mc = M < PQ_SCAN_MC ? M : PQ_SCAN_MC;
  const bool one_pass = mc == M;
  for (int j = tid; j < nprobe; j += PQ_SCAN_THREADS) {
    const int64_t c = probes[(int64_t)qi * ld_probe + j];
    s_off[j] = seg_off[(int64_t)qi * nprobe + j];
    s_cell[j] = (c >= 0 && c < (int64_t)nlist) ? (int)c : -1;
    s_base[j] = probe_scores != nullptr ? probe_scores[(int64_t)qi * ld_probe + j] : 0.f;
  }
  if (one_pass)
    for (int e = tid * 4; e < M * PQ_KSUB; e += PQ_SCAN_THREADS * 4) *(float4*)(ivfpq_lut_s + e) = *(const float4*)(lq + e);
  __syncthreads();
  unsigned long long* wq = words + (int64_t)qi * max_scan;
  unsigned int bad = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s = tile * IVFPQ_TILE + tid;
    const bool in_seg = s < tot;
    int lo = 0, hi = nprobe;                                 // the last slot with s_off[j] <= s (s_off[0] == 0)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)s_off[mid] <= s) lo = mid; else hi = mid;
    }
    const int c = s_cell[lo];
    const int64_t p = c >= 0 ? list_off[c] + (s - (int64_t)s_off[lo]) : -1;
    const bool valid = in_seg && p >= 0 && p < n_rows;
    const int64_t pv = valid ? p : 0;
    const uint8_t* rc = codes + (pv / PQ_BLK) * PQ_BLK * Mp + (pv % PQ_BLK) * PQ_GRP;   // (dereferenced only when valid)
    bool skip = false;                                       // SEL: an original row inside the shard whose bit is clear
    if constexpr (SEL) {
      if (valid) {
        const int64_t o = row_ids != nullptr ? row_ids[p] : p;
        skip = o >= 0 && o < n_rows && !sel_test(sel, o);
      }
    }
    float acc = s_base[lo];
    for (int m0 = 0; m0 < M; m0 += mc) {
      const int m1 = m0 + mc < M ? m0 + mc : M;
      if (!one_pass) {
        __syncthreads();
        for (int e = tid * 4; e < (m1 - m0) * PQ_KSUB; e += PQ_SCAN_THREADS * 4)
          *(float4*)(ivfpq_lut_s + e) = *(const float4*)(lq + (int64_t)m0 * PQ_KSUB + e);
        __syncthreads();
      }
      if (valid && !skip) {
        uint4 cur = *(const uint4*)(rc + (int64_t)(m0 / PQ_GRP) * (PQ_BLK * PQ_GRP));
        for (int g = m0; g < m1; g += PQ_GRP) {
          uint4 nxt = cur;
          if (g + PQ_GRP < m1) nxt = *(const uint4*)(rc + (int64_t)((g + PQ_GRP) / PQ_GRP) * (PQ_BLK * PQ_GRP));
          const float* tg = ivfpq_lut_s + (g - m0) * PQ_KSUB;
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
    if (in_seg) {
      const int64_t orig = valid ? (row_ids != nullptr ? row_ids[p] : p) : -1;
      const bool ok = orig >= 0 && orig < n_rows;
      if (!ok) ++bad;
      wq[s] = (ok && !skip) ? sel_pack(f2key(acc), orig) : 0ull;
    }
  }
  if (bad) atomicAdd(&g_ivf_bad, bad);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// tables [chunk, M, 256] fp32   seg_off [chunk, nprobe]   q_tot [chunk]   words [chunk, max_scan_rows]
// The chunk is the flat index's (ivf_chunk_queries).  Every region but the words is sized for min(n_queries, 1024) queries and the words for
// min(that many segments, the 768 MiB budget or one segment), so the size never decreases in n_queries or in max_scan_rows.
struct IvfPqPlan {
  int chunk;
  size_t off_seg, off_tot, off_words, total;
};
static IvfPqPlan ivf_pq_plan(int32_t M, int32_t n_queries, int32_t nprobe, int64_t max_scan_rows) {
  IvfPqPlan p;
  p.chunk = ivf_chunk_queries(n_queries, max_scan_rows);
  const size_t nq = n_queries < 1 ? 1 : (n_queries > IVF_MAX_CHUNK ? IVF_MAX_CHUNK : (size_t)n_queries);
  const size_t per = (size_t)(max_scan_rows > 0 ? max_scan_rows : 0) * 8;
  const size_t budget = IVF_WORDS_BYTES > per ? IVF_WORDS_BYTES : per;
  const size_t wbytes = nq * per < budget ? nq * per : budget;
  p.off_seg = align256(nq * (size_t)(M > 0 ? M : 1) * PQ_KSUB * 4);
  p.off_tot = p.off_seg + align256(nq * (size_t)(nprobe > 0 ? nprobe : 1) * sizeof(unsigned int));
  p.off_words = p.off_tot + align256(nq * sizeof(int64_t));
  p.total = p.off_words + align256(wbytes + 8);
  return p;
}

extern "C" size_t lrx_ivf_pq_ip_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t M, int32_t n_queries, int32_t nprobe, int32_t k,
                                                int64_t max_scan_rows) {
  (void)n_rows; (void)nlist; (void)dim; (void)k;
  return ivf_pq_plan(M, n_queries, nprobe, max_scan_rows).total;
}

// lrx_ivf_pq_ip_search and lrx_ivf_pq_ip_range_search: the QUERY-MAJOR host driver.  `out` (IvfOut, lrx_search_ivf.h) is how the segments leave:
// k_ivf_select, or the range search's count, lims and fill, whose hit counts lie behind the search's workspace.
static int ivf_pq_run(const char* who, const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                      const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores,
                      int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, const IvfOut& out, const IvfSel& sel, void* workspace,
                      size_t workspace_bytes, void* stream) {
  LRX_CHECK_ARG(M > 0 && dim > 0 && dim % M == 0, "%s: dim=%d is not a multiple of M=%d", who, dim, M);
  if (int rc = ivf_out_check(who, out)) return rc;
  LRX_CHECK_ARG(nlist >= 1, "%s: nlist=%d must be >= 1", who, nlist);
  LRX_CHECK_ARG(nprobe >= 1 && nprobe <= IVF_MAX_NPROBE && nprobe <= nlist, "%s: nprobe=%d out of range (1..min(nlist=%d, %d))", who, nprobe, nlist,
                IVF_MAX_NPROBE);
  LRX_CHECK_ARG(ld_probe >= nprobe, "%s: ld_probe=%lld < nprobe=%d", who, (long long)ld_probe, nprobe);
  LRX_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 32), "%s: rows=%lld out of range", who, (long long)n_rows);
  LRX_CHECK_ARG(max_scan_rows >= 0 && max_scan_rows < (1ll << 31), "%s: max_scan_rows=%lld out of range (0..2^31 - 1)", who, (long long)max_scan_rows);
  if (int rc = ivf_sel_check(who, sel, n_rows)) return rc;
  LRX_CHECK_ARG(n_queries >= 0, "%s: n_queries=%d", who, n_queries);
  hipStream_t s = (hipStream_t)stream;
  if (n_queries == 0) return ivf_out_empty(out, s);
  LRX_CHECK_ARG(q != nullptr && probes != nullptr && list_off != nullptr && pq_centroids != nullptr && ivf_out_ptrs_ok(out) &&
                    (codes != nullptr || n_rows == 0),
                "%s: null pointer", who);
  LRX_CHECK_ARG(by_residual == 0 || probe_scores != nullptr, "%s: by_residual=%d needs probe_scores", who, by_residual);
  const IvfPqPlan p = ivf_pq_plan(M, n_queries, nprobe, max_scan_rows);
  const size_t need = p.total + ivf_out_ws_bytes(out.range, p.chunk);
  if (workspace == nullptr || workspace_bytes < need) {
    lrx_set_error("%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
    return LRX_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  float* lut = (float*)ws;
  unsigned int* seg_off = (unsigned int*)(ws + p.off_seg);
  int64_t* q_tot = (int64_t*)(ws + p.off_tot);
  unsigned long long* words = (unsigned long long*)(ws + p.off_words);
  unsigned int* surv = (unsigned int*)(ws + p.total);        // (the range search's)
  const int Mp = pq_mp(M);
  const size_t smem = (size_t)(M < PQ_SCAN_MC ? M : PQ_SCAN_MC) * PQ_KSUB * 4;
  auto* scan = sel.bits != nullptr ? k_ivf_pq_scan<true> : k_ivf_pq_scan<false>;
  if (smem > (32u << 10)) LRX_HIP(hipFuncSetAttribute((const void*)scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  const int64_t max_tiles = lrx_cdiv(max_scan_rows, IVFPQ_TILE);
  const int ncu = lrx_cu_count();
  for (int q0 = 0; q0 < n_queries; q0 += p.chunk) {
    const int nq = n_queries - q0 < p.chunk ? n_queries - q0 : p.chunk;
    const int64_t* pc = probes + (int64_t)q0 * ld_probe;
    int rc = lrx_pq_lut(q + (int64_t)q0 * dim, nq, pq_centroids, dim, M, lut, stream);
    if (rc != LRX_OK) return rc;
    hipLaunchKernelGGL(k_ivf_plan<true>, dim3(nq), dim3(IVF_PLAN_THREADS), 0, s, pc, (int)nprobe, ld_probe, list_off, (int)nlist, max_scan_rows,
                       (unsigned long long*)nullptr, 0u, (unsigned int*)nullptr, (unsigned int*)nullptr, seg_off, q_tot);
    LRX_LAUNCH_CHECK();
    if (max_tiles > 0) {                                       // (no rows: every word of a segment becomes 0 and is counted)
      int64_t gx = lrx_cdiv(2 * (int64_t)ncu, nq);             // two workgroups' worth of tiles per CU over the chunk, as k_pq_scan's grid
      gx = gx > max_tiles ? max_tiles : gx;
      hipLaunchKernelGGL(scan, dim3((unsigned)gx, (unsigned)nq), dim3(PQ_SCAN_THREADS), smem, s, (const uint8_t*)codes, n_rows, (int)M, Mp,
                         (const float*)lut, pc, by_residual ? probe_scores + (int64_t)q0 * ld_probe : (const float*)nullptr, (int)nprobe, ld_probe, list_off,
                         row_ids, (int)nlist, (const unsigned int*)seg_off, (const int64_t*)q_tot, max_scan_rows, words, sel.bits);
      LRX_LAUNCH_CHECK();
    }
    if (int rc = ivf_out_launch(out, s, words, max_scan_rows, q_tot, surv, q0, nq, 1)) return rc;
  }
  return LRX_OK;
}

extern "C" int lrx_ivf_pq_ip_search(const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                                    const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                    const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k,
                                    int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return ivf_pq_run("ivf_pq_ip_search", codes, n_rows, pq_centroids, dim, M, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe, ld_probe,
                    by_residual, max_scan_rows, ivf_out_topk(k, id_base, out_scores, out_ids, row_map), IVF_NO_SEL, workspace, workspace_bytes, stream);
}

// The search under a row selector (lrx_search_selector.h): sel_bits == NULL is lrx_ivf_pq_ip_search.
extern "C" int lrx_ivf_pq_ip_search_sel(const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                                        const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                        const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k,
                                        int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, const uint32_t* sel_bits,
                                        int64_t sel_rows, void* workspace, size_t workspace_bytes, void* stream) {
  return ivf_pq_run("ivf_pq_ip_search_sel", codes, n_rows, pq_centroids, dim, M, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe,
                    ld_probe, by_residual, max_scan_rows, ivf_out_topk(k, id_base, out_scores, out_ids, row_map), IvfSel{sel_bits, sel_rows}, workspace,
                    workspace_bytes, stream);
}

extern "C" size_t lrx_ivf_pq_ip_range_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t M, int32_t n_queries, int32_t nprobe,
                                                      int64_t max_scan_rows) {
  (void)n_rows; (void)nlist; (void)dim;
  const IvfPqPlan p = ivf_pq_plan(M, n_queries, nprobe, max_scan_rows);
  return p.total + ivf_out_ws_bytes(true, p.chunk);
}

extern "C" int lrx_ivf_pq_ip_range_search(const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                                          const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                          const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows,
                                          float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity,
                                          const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream) {
  return ivf_pq_run("ivf_pq_ip_range_search", codes, n_rows, pq_centroids, dim, M, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe,
                    ld_probe, by_residual, max_scan_rows, ivf_out_range(radius, id_base, lims, out_scores, out_ids, capacity, row_map), IVF_NO_SEL, workspace,
                    workspace_bytes, stream);
}

extern "C" int lrx_ivf_pq_ip_range_search_sel(const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                                              const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                              const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows,
                                              float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity,
                                              const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  return ivf_pq_run("ivf_pq_ip_range_search_sel", codes, n_rows, pq_centroids, dim, M, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe,
                    ld_probe, by_residual, max_scan_rows, ivf_out_range(radius, id_base, lims, out_scores, out_ids, capacity, row_map),
                    IvfSel{sel_bits, sel_rows}, workspace, workspace_bytes, stream);
}
