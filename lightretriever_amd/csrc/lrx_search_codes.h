// liblrx search, part 5 -- what the CODE-BASED indexes (product-quantised, binary, 8-bit scalar-quantised) share on the host.
// Part of the ONE translation unit lrx_search.hip (included after merge_launch, before the three index headers: it reuses align256 and
// merge_launch).  Not a stand-alone header.
//
//     codes_check_*   the argument checks the search entry points have in common (the caller's name prefixes the message)
//     ScanPlan        workspace layout of a row-chunked scan: [the format's own regions][scores qc x ld][block maxima qc x nblk_ld][merge parts]
//     scan_search     the driver: query chunks x row chunks, scan -> select per row chunk, running top-k merged across row chunks, k_map_ids
#pragma once

__global__ void k_map_ids(int64_t* __restrict__ ids, int64_t n, int64_t id_base, const int64_t* __restrict__ row_map) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t r = ids[t];
  if (r >= 0) ids[t] = row_map != nullptr ? row_map[r] : id_base + r;
}

static int codes_check_rows(const char* who, int64_t n_rows) {
  LRX_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 32) - 1, "%s: shard rows=%lld out of range", who, (long long)n_rows);
  return LRX_OK;
}

static int codes_check_topk(const char* who, int32_t k, int64_t n_rows) {
  LRX_CHECK_ARG(k > 0 && k <= SEL_MAXK, "%s: k=%d out of range (1..%d)", who, k, SEL_MAXK);
  return codes_check_rows(who, n_rows);
}

static int codes_check_workspace(const char* who, size_t have, size_t need) {
  if (have >= need) return LRX_OK;
  lrx_set_error("%s: workspace %zu B < required %zu B", who, have, need);
  return LRX_ERR_WORKSPACE;
}

struct ScanPlan {
  int64_t rc, ld;         // rows per score matrix, its row stride
  int nblk_ld, qc;        // block maxima stride, queries per chunk
  bool merge;             // more than one row chunk: running top-k merged with each chunk's
  size_t sc_off, bm_off, part_s_off, part_i_off, total;
};

// row_chunk: rows per score matrix; ld_align: granularity of its row stride; matrix_bytes: budget of one query chunk's matrix + maxima;
// qc_cap: most queries per chunk; lead_bytes(qc): size of the format's own regions, which come first (a multiple of 256).  Block maxima are
// per SP_ROWS = 128 rows, the granularity the selection walks them at.
template <class Lead>
static ScanPlan scan_plan(int64_t n_rows, int32_t n_queries, int32_t k, int64_t row_chunk, int ld_align, int64_t matrix_bytes, int64_t qc_cap, Lead lead_bytes) {
  ScanPlan p;
  p.rc = n_rows < row_chunk ? (n_rows > 0 ? n_rows : 1) : row_chunk;
  p.ld = lrx_cdiv(p.rc, ld_align) * ld_align;
  p.nblk_ld = ((int)lrx_cdiv(p.rc, SP_ROWS) + 3) & ~3;
  p.merge = n_rows > row_chunk;
  int64_t qc = matrix_bytes / (p.ld * 4 + (int64_t)p.nblk_ld * 4);
  const int64_t nq = n_queries > 0 ? n_queries : 1;
  qc = qc > qc_cap ? qc_cap : qc;
  p.qc = (int)(qc < 1 ? 1 : (qc > nq ? nq : qc));
  const size_t q = (size_t)p.qc;
  p.sc_off = lead_bytes(p.qc);
  p.bm_off = p.sc_off + align256(q * (size_t)p.ld * 4);
  p.part_s_off = p.bm_off + align256(q * (size_t)p.nblk_ld * 4);
  p.part_i_off = p.part_s_off + (p.merge ? align256(2 * q * k * 4) : 0);
  p.total = p.part_i_off + (p.merge ? align256(2 * q * k * 8) : 0);
  return p;
}

// The three steps of a format, each returning an LRX status after its launch:
//     prep(q0, nq)                                      the chunk's queries [q0, q0 + nq) into the format's own regions
//     scan(r0, nr, nq, sc, bm)                          rows [r0, r0 + nr): the [nq, p.ld] scores and their block maxima (nr > 0)
//     select(q0, r0, nr, nq, sc, bm, os, oi)            the chunk's top-k per query, rows numbered from r0, into os / oi [nq, k]
// The first row chunk selects straight into the output; a later one into part 1, merged with the running result (copied to part 0).
template <class Prep, class Scan, class Select>
static int scan_search(const ScanPlan& p, void* workspace, int64_t n_rows, int32_t n_queries, int32_t k, int64_t id_base, float* out_scores,
                       int64_t* out_ids, const int64_t* row_map, void* stream, Prep prep, Scan scan, Select select) {
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* sc = (float*)(ws + p.sc_off);
  float* bm = (float*)(ws + p.bm_off);
  float* part_s = (float*)(ws + p.part_s_off);
  int64_t* part_i = (int64_t*)(ws + p.part_i_off);
  for (int32_t q0 = 0; q0 < n_queries; q0 += p.qc) {
    const int nq = n_queries - q0 < p.qc ? n_queries - q0 : p.qc;
    float* os = out_scores + (int64_t)q0 * k;
    int64_t* oi = out_ids + (int64_t)q0 * k;
    int rc = prep(q0, nq);
    if (rc != LRX_OK) return rc;
    int64_t r0 = 0;
    do {
      const int64_t nr = n_rows - r0 < p.rc ? n_rows - r0 : p.rc;
      if (nr > 0 && (rc = scan(r0, nr, nq, sc, bm)) != LRX_OK) return rc;
      const bool into_part = r0 > 0;
      rc = select(q0, r0, nr, nq, (const float*)sc, (const float*)bm, into_part ? part_s + (int64_t)nq * k : os, into_part ? part_i + (int64_t)nq * k : oi);
      if (rc != LRX_OK) return rc;
      if (into_part) {
        LRX_HIP(hipMemcpyAsync(part_s, os, (size_t)nq * k * 4, hipMemcpyDeviceToDevice, s));
        LRX_HIP(hipMemcpyAsync(part_i, oi, (size_t)nq * k * 8, hipMemcpyDeviceToDevice, s));
        if ((rc = merge_launch(part_s, part_i, nullptr, 2, nq, k, os, oi, stream)) != LRX_OK) return rc;
      }
      r0 += nr;
    } while (r0 < n_rows);
    const int64_t n_out = (int64_t)nq * k;
    hipLaunchKernelGGL(k_map_ids, dim3((unsigned)lrx_cdiv(n_out, 256)), dim3(256), 0, s, oi, n_out, id_base, row_map);
    LRX_LAUNCH_CHECK();
  }
  return LRX_OK;
}
