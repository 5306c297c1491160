// liblrx search, part 5 -- what the CODE-BASED indexes (product-quantised, binary, 8-bit scalar-quantised) share on the host.
// Part of the ONE translation unit lrx_search.hip (included after merge_launch, before the three index headers: it reuses align256 and
// merge_launch).  Not a stand-alone header.
//
//     codes_check_*   the argument checks the search entry points have in common (the caller's name prefixes the message)
//     ScanPlan        workspace layout of a row-chunked scan: [the format's own regions][scores qc x ld][block maxima qc x nblk_ld][merge parts]
//     scan_search     the driver: query chunks x row chunks, scan -> select per row chunk, running top-k merged across row chunks, k_map_ids
//     scan_range      RANGE search over the same prep / scan steps (every row whose matrix score passes a predicate, in row order): two sweeps
//                     over (query chunk x row chunk) -- scan + count per segment, lims, scan again + fill (k_scan_range, k_scan_range_bases)
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

// ---------------------------------------------------------------------------------------------------------------
// Range search over the scan driver: (lims, scores, ids) of every row whose matrix score passes `Keep`, ids = id_base + row, ascending rows
// inside a query (the contract of lrx_flat_ip_range_search; for the formats served here the matrix score IS the reported score).
// A query's results must be contiguous across row chunks, and the matrix of a chunk is gone when the next one is scanned, so the driver
// makes two sweeps over (query chunk x row chunk) and scans twice: sweep 1 counts per (query, segment), one pass turns the counts into
// per-segment bases and the lims of the whole call, sweep 2 scans again and fills.  (Keeping the matrices between the sweeps would cost
// Q x rows x 4 bytes -- the memory a quantised index exists to save.)
// ---------------------------------------------------------------------------------------------------------------
#define SR_THREADS 256
#define SR_SEG 4096          // rows per segment: one workgroup per (query, segment), 16 tiles of 256 rows

// the two predicates on a matrix score (monotone: a 128-row block holds a kept row iff its maximum is kept)
struct KeepAbove {           // PQ: s > radius
  float radius;
  __device__ __forceinline__ bool operator()(float s) const { return s > radius; }
};
struct KeepHitAbove {        // impact: a hit (S >= 1) whose score is > radius
  float radius;
  __device__ __forceinline__ bool operator()(float s) const { return s > 0.f && s > radius; }
};

// Grid nq * nseg workgroups of SR_THREADS: workgroup (query qi, segment sg) walks rows [sg SR_SEG, min(nr, (sg + 1) SR_SEG)) of the row
// chunk's score row in tiles of 256 rows (thread t <-> row tile + t) and skips a tile whose two 128-row block maxima both fail the predicate
// (uniform for the workgroup).  A kept row's slot: the segment's base + kept rows in the tiles before (run) + kept rows of the waves before
// in this tile (popcounts through LDS, double-buffered: one barrier per tile) + kept lanes below in its wave (ballot) -- ascending row order
// by construction, no sort, no atomics.  FILL = false: seg[qi * seg_ld + sg] = the segment's count.  FILL = true: seg[..] holds the kept rows of
// the query in front of the segment (k_scan_range_bases); (score, id0 + row) go to lims[qi] + that + slot with plain stores, and nothing is
// written unless the whole call's result fits: *lims_end <= capacity.
template <bool FILL, class Keep>
__global__ void __launch_bounds__(SR_THREADS)
k_scan_range(const float* __restrict__ scores, int64_t ld, int64_t nr, const float* __restrict__ blkmax, int nblk_ld, int nseg, Keep keep,
             unsigned int* __restrict__ seg, int64_t seg_ld, const int64_t* __restrict__ lims, const int64_t* __restrict__ lims_end, int64_t capacity,
             int64_t id0, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  __shared__ unsigned int s_w[2][SR_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = (int)(blockIdx.x / (unsigned)nseg), sg = (int)(blockIdx.x % (unsigned)nseg);
  if (FILL && *lims_end > capacity) return;
  const float* row = scores + (int64_t)qi * ld;
  const float* bm = blkmax + (int64_t)qi * nblk_ld;
  unsigned int* sq = seg + (int64_t)qi * seg_ld;
  const int64_t s0 = (int64_t)sg * SR_SEG, s1 = s0 + SR_SEG < nr ? s0 + SR_SEG : nr;
  const int64_t base = FILL ? lims[qi] + (int64_t)sq[sg] : 0;
  unsigned int run = 0;
  int par = 0;
  for (int64_t t0 = s0; t0 < s1; t0 += SR_THREADS) {
    const int64_t b = t0 / SP_ROWS;
    if (!(keep(bm[b]) || ((b + 1) * SP_ROWS < s1 && keep(bm[b + 1])))) continue;
    const int64_t i = t0 + tid;
    const float v = i < s1 ? row[i] : 0.f;
    const bool kp = i < s1 && keep(v);
    const unsigned long long bal = __ballot(kp);
    if (lane == 0) s_w[par][wave] = (unsigned int)__popcll(bal);
    __syncthreads();
    unsigned int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SR_THREADS / 64; ++w) {
      const unsigned int c = s_w[par][w];
      before += w < wave ? c : 0u;
      total += c;
    }
    if (FILL && kp) {
      const int64_t pos = base + run + before + (unsigned int)__popcll(bal & ((1ull << lane) - 1ull));
      out_scores[pos] = v;
      out_ids[pos] = id0 + i;
    }
    run += total;
    par ^= 1;
  }
  if (!FILL && tid == 0) sq[sg] = run;
}

// Per query (one 256-thread workgroup): the nseg segment counts become the kept rows in front of every segment (exclusive scan, in place) and
// surv[q] = the query's total.
__global__ void __launch_bounds__(256) k_scan_range_bases(unsigned int* __restrict__ seg, int64_t nseg, unsigned int* __restrict__ surv) {
  __shared__ unsigned int s_sum[256];
  const int tid = threadIdx.x;
  unsigned int* c = seg + (int64_t)blockIdx.x * nseg;
  const int64_t per = (nseg + 255) / 256, w0 = tid * per, w1 = nseg < w0 + per ? nseg : w0 + per;
  unsigned int t = 0;
  for (int64_t w = w0; w < w1; ++w) t += c[w];
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
    const unsigned int n = c[w];
    c[w] = run;
    run += n;
  }
  if (tid == 255) surv[blockIdx.x] = s_sum[255];
}

// ScanPlan of a range call plus its own two regions, which sit at the end of the plan's leading part (after the format's regions, before the
// score matrix): seg [n_queries, nseg] and surv [n_queries] for ALL queries of the call -- the counts of sweep 1 outlive its query chunks.
struct ScanRangePlan {
  ScanPlan p;
  int spc;                // segments per row chunk
  int64_t nseg;           // segments per query: row chunks x spc
  size_t seg_off, surv_off;
};

template <class Lead>
static ScanRangePlan scan_range_plan(int64_t n_rows, int32_t n_queries, int64_t row_chunk, int ld_align, int64_t matrix_bytes, int64_t qc_cap, Lead lead_bytes) {
  ScanRangePlan rp;
  const int64_t rc = n_rows < row_chunk ? (n_rows > 0 ? n_rows : 1) : row_chunk;          // (= ScanPlan::rc)
  rp.spc = (int)lrx_cdiv(rc, SR_SEG);
  rp.nseg = lrx_cdiv(n_rows > 0 ? n_rows : 1, rc) * rp.spc;
  const size_t nq = (size_t)(n_queries > 0 ? n_queries : 1);
  const size_t seg_bytes = align256(nq * (size_t)rp.nseg * 4), surv_bytes = align256(nq * 4);
  rp.p = scan_plan(n_rows, n_queries, 1, row_chunk, ld_align, matrix_bytes, qc_cap, [&](int qc) { return lead_bytes(qc) + seg_bytes + surv_bytes; });
  rp.seg_off = rp.p.sc_off - seg_bytes - surv_bytes;
  rp.surv_off = rp.p.sc_off - surv_bytes;
  return rp;
}

static int codes_check_range(const char* who, int64_t n_rows, int32_t n_queries, float radius, const int64_t* lims, const float* out_scores,
                             const int64_t* out_ids, int64_t capacity, int64_t row_chunk) {
  LRX_CHECK_ARG(n_queries >= 0 && capacity >= 0, "%s: n_queries=%d / capacity=%lld must be >= 0", who, n_queries, (long long)capacity);
  LRX_CHECK_ARG(radius == radius, "%s: radius is NaN", who);
  LRX_CHECK_ARG(lims != nullptr, "%s: null lims", who);
  LRX_CHECK_ARG(capacity == 0 || (out_scores != nullptr && out_ids != nullptr), "%s: null outputs with capacity=%lld", who, (long long)capacity);
  LRX_CHECK_ARG(row_chunk == 0 || (row_chunk > 0 && row_chunk % SP_ROWS == 0), "%s: row_chunk=%lld must be 0 (the library's rule) or a positive multiple of %d",
                who, (long long)row_chunk, SP_ROWS);
  return codes_check_rows(who, n_rows);
}

// prep / scan: the steps of scan_search (the same lambdas serve both).  n_rows > 0 and n_queries > 0 (the callers answer the empty cases).
template <class Prep, class Scan, class Keep>
static int scan_range(const ScanRangePlan& rp, void* workspace, int64_t n_rows, int32_t n_queries, int64_t id_base, int64_t* lims, float* out_scores,
                      int64_t* out_ids, int64_t capacity, void* stream, Prep prep, Scan scan, Keep keep) {
  hipStream_t s = (hipStream_t)stream;
  const ScanPlan& p = rp.p;
  char* ws = (char*)workspace;
  float* sc = (float*)(ws + p.sc_off);
  float* bm = (float*)(ws + p.bm_off);
  unsigned int* seg = (unsigned int*)(ws + rp.seg_off);
  unsigned int* surv = (unsigned int*)(ws + rp.surv_off);
  // (a row chunk shorter than the others has fewer segments: the slots it leaves out must count as empty)
  LRX_HIP(hipMemsetAsync(seg, 0, (size_t)n_queries * (size_t)rp.nseg * 4, s));
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int32_t q0 = 0; q0 < n_queries; q0 += p.qc) {
      const int nq = n_queries - q0 < p.qc ? n_queries - q0 : p.qc;
      int rc = prep(q0, nq);
      if (rc != LRX_OK) return rc;
      int64_t chunk = 0;
      for (int64_t r0 = 0; r0 < n_rows; r0 += p.rc, ++chunk) {
        const int64_t nr = n_rows - r0 < p.rc ? n_rows - r0 : p.rc;
        if ((rc = scan(r0, nr, nq, sc, bm)) != LRX_OK) return rc;
        const int nseg = (int)lrx_cdiv(nr, SR_SEG);
        unsigned int* sq = seg + (int64_t)q0 * rp.nseg + chunk * rp.spc;
        if (sweep == 0)
          hipLaunchKernelGGL((k_scan_range<false, Keep>), dim3((unsigned)((int64_t)nq * nseg)), dim3(SR_THREADS), 0, s, (const float*)sc, p.ld, nr, (const float*)bm,
                             p.nblk_ld, nseg, keep, sq, rp.nseg, (const int64_t*)lims + q0, (const int64_t*)lims + n_queries, capacity, id_base + r0, out_scores,
                             out_ids);
        else
          hipLaunchKernelGGL((k_scan_range<true, Keep>), dim3((unsigned)((int64_t)nq * nseg)), dim3(SR_THREADS), 0, s, (const float*)sc, p.ld, nr, (const float*)bm,
                             p.nblk_ld, nseg, keep, sq, rp.nseg, (const int64_t*)lims + q0, (const int64_t*)lims + n_queries, capacity, id_base + r0, out_scores,
                             out_ids);
        LRX_LAUNCH_CHECK();
      }
    }
    if (sweep == 0) {
      hipLaunchKernelGGL(k_scan_range_bases, dim3((unsigned)n_queries), dim3(256), 0, s, seg, rp.nseg, surv);
      LRX_LAUNCH_CHECK();
      for (int32_t q0 = 0; q0 < n_queries; q0 += 1024) {
        hipLaunchKernelGGL(k_range_lims, dim3(1), dim3(1024), 0, s, (const unsigned int*)surv + q0, n_queries - q0 < 1024 ? n_queries - q0 : 1024, lims + q0,
                           q0 == 0 ? 1 : 0);
        LRX_LAUNCH_CHECK();
      }
    }
  }
  return LRX_OK;
}
