// liblrx search, part N -- INVERTED FILE over fp16 SCALAR-QUANTISED codes (faiss IndexIVFScalarQuantizer, QT_fp16, inner product): the exact
// top k under the fp16 store's score over the rows of the cells a query probes.  k_ivf_sq_scan, k_ivf_sq_encode, lrx_ivf_sq_fp16_ip_search,
// lrx_ivf_sq_fp16_encode_rows (contract: include/lrx.h).
// Part of the ONE translation unit lrx_search.hip (included at its end, after lrx_search_ivfpq.h: it reuses the whole cell-major chain of
// lrx_search_ivf.h -- ivf_cell_major_search: clear, plan, items, scatter, select, the chunking, the workspace and the error counter -- and
// f2h_sat of lrx_search_filter.h).  Not a stand-alone header.
//
// The only kernel of the chain that is this file's is the scan: k_ivf_scan's item walk over codes of 2 bytes per element, row-major [n_rows, dim]
// by stored position (NOT the tiled layout of the flat fp16 index: a cell's rows are consecutive, so a group is one contiguous run of bytes).
#pragma once

#define IVFSQ_LDS_HALVES 32768            // 64 KiB of codes per workgroup, as k_ivf_scan's rows: twice its rows per group

static int ivf_sq_group_rows(int32_t dim) {
  const int g = IVFSQ_LDS_HALVES / dim;
  return g > IVF_MAX_GROUP_ROWS ? IVF_MAX_GROUP_ROWS : (g < 1 ? 1 : g);
}
extern "C" int32_t lrx_ivf_sq_fp16_group_rows(int32_t dim) { return dim >= 1 ? ivf_sq_group_rows(dim) : 0; }

// exact_dot_lds over a row of fp16 codes (row-major in LDS), each code decoded exactly to fp32: the partial products and their order are
// exact_dot_codes', and with base = 0 so are the bits.
__device__ __forceinline__ float exact_dot_lds_codes(const _Float16* c_lds, const float* __restrict__ qglob, int D, int lane, double base) {
  return exact_dot_lds<true>([=](int i) { const f16x4 h = *(const f16x4*)(c_lds + i); return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]}; },
                             qglob, D, lane, base);
}

// The scan: ivf_scan_items (lrx_search_ivf.h) over fp16 codes.  A group's code rows -- one contiguous run of nrows * D halves, 16-byte aligned
// since D % 32 == 0, nrows * D <= IVFSQ_LDS_HALVES -- are staged in LDS AS fp16 (coalesced non-temporal 16-byte loads); a pair's score is
// the dot over the codes plus its base term (ivf_probe_base).  SEL: the walk under a row selector (ivf_scan_items).
template <bool SEL>
__global__ void __launch_bounds__(ROWGRP_THREADS)
k_ivf_sq_scan(const _Float16* __restrict__ C, int64_t N, int D, int G, const int64_t* __restrict__ list_off, const int64_t* __restrict__ row_ids, int nlist,
              const float* __restrict__ q, const float* __restrict__ probe_scores, int nprobe, int64_t ld_probe,
              const unsigned long long* __restrict__ sorted, const unsigned int* __restrict__ cell_off, const unsigned int* __restrict__ item_off,
              unsigned int item_cap, const unsigned int* __restrict__ seg_off, int64_t max_scan, unsigned long long* __restrict__ words,
              const uint32_t* __restrict__ sel) {
  __shared__ __attribute__((aligned(16))) _Float16 s_c[IVFSQ_LDS_HALVES];
  const int tid = threadIdx.x, lane = tid & 63;
  ivf_scan_items<SEL>(N, G, list_off, row_ids, nlist, nprobe, sorted, cell_off, item_off, item_cap, seg_off, max_scan, words, sel,
    [&](int64_t ra, int nrows) {
      const _Float16* src = C + ra * D;
      for (int i = tid * 8; i < nrows * D; i += ROWGRP_THREADS * 8) *(f16x8*)(s_c + i) = __builtin_nontemporal_load((const f16x8*)(src + i));
    },
    [&](int rr, unsigned int qi, unsigned int slot) {
      return exact_dot_lds_codes(s_c + rr * D, q + (int64_t)qi * D, D, lane, ivf_probe_base(probe_scores, ld_probe, nprobe, qi, slot));
    });
}

// The codes of n rows, one workgroup per row in turn: v = x - centroid[cell] (one fp32 subtraction; cent == NULL: v = x), code = fp16(v) by
// f2h_sat (round-to-nearest-even, saturating at +-65504), into code row row0 + i.  A cell outside [0, nlist) is never dereferenced: the row's
// codes are zeros and it is counted.
__global__ void __launch_bounds__(256)
k_ivf_sq_encode(const float* __restrict__ x, int64_t ldx, int64_t n, int D, const float* __restrict__ cent, const int64_t* __restrict__ cells, int nlist,
                _Float16* __restrict__ codes, int64_t row0) {
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t c = cells != nullptr ? cells[i] : 0;
    const bool ok = cells == nullptr || (c >= 0 && c < (int64_t)nlist);
    const float* xr = x + i * ldx;
    const float* cr = (ok && cent != nullptr) ? cent + c * D : nullptr;
    _Float16* o = codes + (row0 + i) * D;
    for (int e = threadIdx.x * 4; e < D; e += 256 * 4) {
      f16x4 h = {0, 0, 0, 0};
      if (ok) {
        const f32x4 xv = *(const f32x4*)(xr + e);
        const f32x4 cv = cr != nullptr ? *(const f32x4*)(cr + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) h[t] = f2h_sat(cr != nullptr ? xv[t] - cv[t] : xv[t]);
      }
      *(f16x4*)(o + e) = h;
    }
    if (!ok && threadIdx.x == 0) atomicAdd(&g_ivf_bad, 1u);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
extern "C" size_t lrx_ivf_sq_fp16_ip_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int32_t k,
                                                     int64_t max_scan_rows) {
  return lrx_ivf_flat_ip_workspace_bytes(n_rows, nlist, dim, n_queries, nprobe, k, max_scan_rows);
}

// lrx_ivf_sq_fp16_ip_search and lrx_ivf_sq_fp16_ip_range_search: the driver over k_ivf_sq_scan
static int ivf_sq_run(const char* who, const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                      const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores, int32_t nprobe, int64_t ld_probe,
                      int32_t by_residual, int64_t max_scan_rows, const IvfOut& out, const IvfSel& sel, void* workspace, size_t workspace_bytes, void* stream) {
  LRX_CHECK_ARG(by_residual == 0 || probe_scores != nullptr, "%s: by_residual=%d needs probe_scores", who, by_residual);
  return ivf_cell_major_search(who, codes, (uintptr_t)codes % 16 == 0, "codes must be 16-byte aligned", dim > 0 ? ivf_sq_group_rows(dim) : 1, n_rows, dim,
                               list_off, nlist, q, n_queries, probes, nprobe, ld_probe, max_scan_rows, out, sel, workspace, workspace_bytes, stream,
                               [&](const IvfScanArgs& a) {
    auto* kern = a.sel != nullptr ? k_ivf_sq_scan<true> : k_ivf_sq_scan<false>;
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(ROWGRP_THREADS), 0, a.stream, (const _Float16*)codes, n_rows, (int)dim, a.G, list_off, row_ids,
                       (int)nlist, a.q, by_residual ? probe_scores + (int64_t)a.q0 * ld_probe : (const float*)nullptr, (int)nprobe, ld_probe, a.sorted,
                       a.cell_off, a.item_off, a.item_cap, a.seg_off, max_scan_rows, a.words, a.sel);
  });
}

extern "C" int lrx_ivf_sq_fp16_ip_search(const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                                         const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores, int32_t nprobe,
                                         int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k, int64_t id_base, float* out_scores,
                                         int64_t* out_ids, const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream) {
  return ivf_sq_run("ivf_sq_fp16_ip_search", codes, n_rows, dim, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe, ld_probe, by_residual,
                    max_scan_rows, ivf_out_topk(k, id_base, out_scores, out_ids, row_map), IVF_NO_SEL, workspace, workspace_bytes, stream);
}

// The search under a row selector (lrx_search_selector.h): sel_bits == NULL is lrx_ivf_sq_fp16_ip_search.
extern "C" int lrx_ivf_sq_fp16_ip_search_sel(const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                                             const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores, int32_t nprobe,
                                             int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k, int64_t id_base, float* out_scores,
                                             int64_t* out_ids, const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  return ivf_sq_run("ivf_sq_fp16_ip_search_sel", codes, n_rows, dim, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe, ld_probe,
                    by_residual, max_scan_rows, ivf_out_topk(k, id_base, out_scores, out_ids, row_map), IvfSel{sel_bits, sel_rows}, workspace, workspace_bytes,
                    stream);
}

extern "C" size_t lrx_ivf_sq_fp16_ip_range_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe,
                                                           int64_t max_scan_rows) {
  return lrx_ivf_flat_ip_range_workspace_bytes(n_rows, nlist, dim, n_queries, nprobe, max_scan_rows);
}

extern "C" int lrx_ivf_sq_fp16_ip_range_search(const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                                               const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores, int32_t nprobe,
                                               int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, float radius, int64_t id_base, int64_t* lims,
                                               float* out_scores, int64_t* out_ids, int64_t capacity, const int64_t* row_map, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  return ivf_sq_run("ivf_sq_fp16_ip_range_search", codes, n_rows, dim, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe, ld_probe,
                    by_residual, max_scan_rows, ivf_out_range(radius, id_base, lims, out_scores, out_ids, capacity, row_map), IVF_NO_SEL, workspace,
                    workspace_bytes, stream);
}

extern "C" int lrx_ivf_sq_fp16_ip_range_search_sel(const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids,
                                                   int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores,
                                                   int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, float radius,
                                                   int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity,
                                                   const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace,
                                                   size_t workspace_bytes, void* stream) {
  return ivf_sq_run("ivf_sq_fp16_ip_range_search_sel", codes, n_rows, dim, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe, ld_probe,
                    by_residual, max_scan_rows, ivf_out_range(radius, id_base, lims, out_scores, out_ids, capacity, row_map), IvfSel{sel_bits, sel_rows},
                    workspace, workspace_bytes, stream);
}

extern "C" int lrx_ivf_sq_fp16_encode_rows(const float* x, int64_t ldx, int64_t n, int32_t dim, const float* centroids, const int64_t* cells, int32_t nlist,
                                           void* codes, int64_t row0, void* stream) {
  LRX_CHECK_ARG(dim >= 32 && dim <= 8192 && dim % 32 == 0, "ivf_sq_fp16_encode_rows: dim=%d must be a multiple of 32 in 32..8192", dim);
  LRX_CHECK_ARG(n >= 0 && row0 >= 0 && row0 + n < (1ll << 32), "ivf_sq_fp16_encode_rows: rows [%lld, %lld + %lld) out of range", (long long)row0,
                (long long)row0, (long long)n);
  LRX_CHECK_ARG(nlist >= 1, "ivf_sq_fp16_encode_rows: nlist=%d must be >= 1", nlist);
  LRX_CHECK_ARG(centroids == nullptr || cells != nullptr, "ivf_sq_fp16_encode_rows: centroids need cells");
  if (n == 0) return LRX_OK;
  LRX_CHECK_ARG(x != nullptr && codes != nullptr, "ivf_sq_fp16_encode_rows: null pointer");
  LRX_CHECK_ARG(ldx >= dim && ldx % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)centroids % 16 == 0 && (uintptr_t)codes % 16 == 0,
                "ivf_sq_fp16_encode_rows: x, centroids and codes must be 16-byte aligned (ldx=%lld >= dim=%d, ldx %% 4 == 0)", (long long)ldx, dim);
  const int64_t wgs = n < 8 * (int64_t)lrx_cu_count() * 8 ? n : 8 * (int64_t)lrx_cu_count() * 8;
  hipLaunchKernelGGL(k_ivf_sq_encode, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, x, ldx, n, (int)dim, centroids, cells, (int)nlist,
                     (_Float16*)codes, row0);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}
