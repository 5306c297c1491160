// liblrx search, part L -- INVERTED FILE (faiss IndexIVFFlat, inner product): the exact top k over the rows of the cells a query probes.
// k_ivf_plan, k_ivf_scan, k_ivf_select, lrx_ivf_flat_ip_search (contract: include/lrx.h); and the range search over the same
// cells: k_ivf_range, lrx_ivf_flat_ip_range_search.
// Part of the ONE translation unit lrx_search.hip (included at its end: it reuses exact_dot_lds_row, the counting sort k_pairs_scan /
// k_pairs_scatter, the radix select and the register sort).  Not a stand-alone header.
//
// A call walks its queries in chunks; per chunk, on one stream:
//   k_ivf_clear    zeroes the pair counter and the per-cell pair counts (a kernel, not a memset: under HIP-graph capture every step of the
//                  chain is then a kernel node, the only node kind the captured searches of this library use)
//   k_ivf_plan     one workgroup per query: its probe list is checked (< 0 skipped, >= nlist counted and skipped, a cell named twice kept once),
//                  the sizes of its cells are scanned into the offsets of its segment of score words, and one (cell, slot) pair per probed
//                  non-empty cell is emitted; a query whose cells hold more than max_scan_rows emits nothing and is counted
//   k_ivf_items / k_pairs_scatter   the pairs grouped by cell (the counting sort of k_pairs_scan / k_pairs_scatter; the scan kernel here also
//                  lays out the work items: a probed cell is ceil(rows / G) groups of G consecutive stored rows)
//   k_ivf_scan     CELL-MAJOR, persistent (ivf_scan_items, the walk of the three scans): a workgroup stages a group of a probed cell in LDS once
//                  and scores it against every query that probes the cell -- one half-wave per (query, row), the query row streamed from L2
//                  (exact_dot_lds_row: the bits of exact_dot) -- writing packed (score, ORIGINAL row) words into the queries' segments.
//                  Cells nobody probes cost nothing.
//   k_ivf_select   one workgroup per query: sorted top k of its segment (counting ranks / register sort up to 2048 words, radix select above).
//   (a range search ends the chunk differently: k_ivf_range<false> counts the words above the radius, k_range_lims turns the counts into
//   lims, k_ivf_range<true> writes them in segment order -- see k_ivf_range)
// Every size depends on the arguments alone; nothing is read back to the host.  The host driver of this chain is ivf_cell_major_search, shared
// with the scans over fp16 and 8-bit codes (lrx_search_ivfsq.h, lrx_search_ivfsq8.h): an entry brings its row check, its group size and the
// launch of its scan, and an IvfOut that says how the segments leave (top k, or everything above a radius).
#pragma once

#define IVF_MAX_NPROBE 2048
#define IVF_PLAN_THREADS 256
#define IVF_MAX_GROUP_ROWS 128            // rows per workgroup of the scan at small D (64 KiB of rows otherwise: ROWGRP_LDS_FLOATS)
#define IVF_WORDS_BYTES ((size_t)768 << 20)   // score words of one query chunk (the workspace stays under 1 GiB)
#define IVF_MAX_CHUNK 1024                // queries per chunk
#define IVF_SEL_SORT 2048                 // segments up to this many words are sorted whole

// Probe entries >= nlist, queries over max_scan_rows and stored rows whose original number is outside the shard, since the last reset: part
// of lrx_device_error_count (lrx_elementwise.hip).
__device__ unsigned int g_ivf_bad = 0;
unsigned int lrx_ivf_bad_entries(int* ok, int reset) {
  unsigned int v = 0;
  *ok = hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_ivf_bad), sizeof(v)) == hipSuccess;
  if (*ok && reset && v) {
    const unsigned int z = 0;
    *ok = hipMemcpyToSymbol(HIP_SYMBOL(g_ivf_bad), &z, sizeof(z)) == hipSuccess;
  }
  return v;
}

static int ivf_group_rows(int32_t dim) {
  const int g = ROWGRP_LDS_FLOATS / dim;
  return g > IVF_MAX_GROUP_ROWS ? IVF_MAX_GROUP_ROWS : (g < 1 ? 1 : g);
}

__global__ void k_ivf_clear(unsigned int* __restrict__ ints, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ints[i] = 0u;
}

// Plan of one query (see the head of the file).  pairs: (cell << 32 | slot), slot = query * nprobe + j; seg_off[slot]: where the cell's rows
// start in the query's segment (cells in probe order); q_tot[query]: words of the segment, -1 = over max_scan_rows.
// DENSE (the query-major scan of lrx_search_ivfpq.h): seg_off is written for EVERY slot of a query that is not over the bound -- a skipped
// entry (< 0, >= nlist, a repeat, an empty cell) holds no words, so its offset is its successor's and the offsets ascend -- and nothing
// else is: no pairs, no per-cell counts (pairs / total / cell_cnt may be NULL).  DENSE = false is the plan of the cell-major scan, unchanged.
template <bool DENSE>
__global__ void __launch_bounds__(IVF_PLAN_THREADS)
k_ivf_plan(const int64_t* __restrict__ probes, int nprobe, int64_t ld_probe, const int64_t* __restrict__ list_off, int nlist, int64_t max_scan,
           unsigned long long* __restrict__ pairs, unsigned int pair_cap, unsigned int* __restrict__ total, unsigned int* __restrict__ cell_cnt,
           unsigned int* __restrict__ seg_off, int64_t* __restrict__ q_tot) {
  __shared__ int s_cell[IVF_MAX_NPROBE];
  __shared__ int64_t s_size[IVF_MAX_NPROBE];                 // rows of the entry's cell; -1: the entry names no cell of its own
  __shared__ int64_t s_wrows[IVF_PLAN_THREADS / 64];
  __shared__ unsigned int s_wcnt[IVF_PLAN_THREADS / 64];
  __shared__ unsigned int s_bad, s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, qi = blockIdx.x;
  const int64_t* pl = probes + (int64_t)qi * ld_probe;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  for (int j = tid; j < nprobe; j += IVF_PLAN_THREADS) {
    const int64_t c = pl[j];
    int v = -1;
    if (c >= (int64_t)nlist) atomicAdd(&s_bad, 1u);          // never dereferenced
    else if (c >= 0) v = (int)c;
    s_cell[j] = v;
  }
  __syncthreads();
  // every thread owns a run of consecutive entries, so the offsets follow the probe order
  const int per = (nprobe + IVF_PLAN_THREADS - 1) / IVF_PLAN_THREADS;
  const int j0 = min(tid * per, nprobe), j1 = min(j0 + per, nprobe);
  int64_t mine = 0;
  unsigned int myn = 0;
  for (int j = j0; j < j1; ++j) {
    const int c = s_cell[j];
    int64_t sz = -1;
    if (c >= 0) {
      bool dup = false;
      for (int jj = 0; jj < j && !dup; ++jj) dup = s_cell[jj] == c;
      if (!dup) {
        sz = list_off[c + 1] - list_off[c];
        sz = sz < 0 ? 0 : (sz > max_scan ? max_scan + 1 : sz);
      }
    }
    s_size[j] = sz;
    if (sz > 0) { mine += sz; ++myn; }
  }
  int64_t xr = mine;                                         // inclusive scans of the threads' totals inside the wave
  unsigned int xn = myn;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t yr = __shfl_up(xr, o, 64);
    const unsigned int yn = __shfl_up(xn, o, 64);
    if (lane >= o) { xr += yr; xn += yn; }
  }
  if (lane == 63) { s_wrows[wave] = xr; s_wcnt[wave] = xn; }
  __syncthreads();
  int64_t run = xr - mine, tot = 0;
  unsigned int pos = xn - myn, npairs = 0;
#pragma unroll
  for (int w = 0; w < IVF_PLAN_THREADS / 64; ++w) {
    if (w < wave) { run += s_wrows[w]; pos += s_wcnt[w]; }
    tot += s_wrows[w];
    npairs += s_wcnt[w];
  }
  const bool over = tot > max_scan;
  if (tid == 0) {
    q_tot[qi] = over ? -1 : tot;
    const unsigned int bad = s_bad + (over ? 1u : 0u);
    if (bad) atomicAdd(&g_ivf_bad, bad);
    s_base = (!DENSE && !over && npairs) ? atomicAdd(total, npairs) : 0u;
  }
  __syncthreads();
  if (over) return;
  const unsigned int base = s_base;
  for (int j = j0; j < j1; ++j) {
    const int64_t sz = s_size[j];
    if (DENSE) {
      seg_off[(unsigned int)qi * (unsigned int)nprobe + (unsigned int)j] = (unsigned int)run;
      if (sz > 0) run += sz;
      continue;
    }
    if (sz <= 0) continue;
    const unsigned int slot = (unsigned int)qi * (unsigned int)nprobe + (unsigned int)j;
    const unsigned int c = (unsigned int)s_cell[j];
    seg_off[slot] = (unsigned int)run;
    if (base + pos < pair_cap) {                             // (always: the chunk emits at most one pair per probe entry)
      pairs[base + pos] = ((unsigned long long)c << 32) | (unsigned long long)slot;
      atomicAdd(&cell_cnt[c], 1u);
    }
    run += sz;
    ++pos;
  }
}

// Work list of the scan (one workgroup): per cell, the exclusive scans of its pair count (cell_off: where its pairs lie in `sorted`) and of
// its work items (item_off) -- a probed cell is ceil(rows / G) items of G consecutive rows, a cell nobody probes is none.  k_pairs_scan's
// one-pass scheme (every thread owns a run of consecutive cells, wave scan, wave totals) over two quantities.
__global__ void __launch_bounds__(1024)
k_ivf_items(const unsigned int* __restrict__ cell_cnt, const int64_t* __restrict__ list_off, int nlist, int64_t N, int G, unsigned int* __restrict__ cell_off,
            unsigned int* __restrict__ item_off) {
  __shared__ unsigned int s_wp[16], s_wi[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (nlist + 1 + 1023) / 1024;
  const int g0 = min(tid * per, nlist + 1), g1 = min(g0 + per, nlist + 1);
  auto items_of = [&](int c) -> unsigned int {
    if (c >= nlist || cell_cnt[c] == 0) return 0u;
    int64_t sz = list_off[c + 1] - list_off[c];
    sz = sz < 0 ? 0 : (sz > N ? N : sz);
    return (unsigned int)((sz + G - 1) / G);
  };
  unsigned int mp = 0, mi = 0;
  for (int c = g0; c < g1; ++c) { mp += c < nlist ? cell_cnt[c] : 0u; mi += items_of(c); }
  unsigned int xp = mp, xi = mi;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned int yp = __shfl_up(xp, o, 64), yi = __shfl_up(xi, o, 64);
    if (lane >= o) { xp += yp; xi += yi; }
  }
  if (lane == 63) { s_wp[wave] = xp; s_wi[wave] = xi; }
  __syncthreads();
  unsigned int rp = xp - mp, ri = xi - mi;
  for (int w = 0; w < wave; ++w) { rp += s_wp[w]; ri += s_wi[w]; }
  for (int c = g0; c < g1; ++c) {
    cell_off[c] = rp;
    item_off[c] = ri;
    rp += c < nlist ? cell_cnt[c] : 0u;
    ri += items_of(c);
  }
}

// The walk of the CELL-MAJOR scans (k_ivf_scan below, k_ivf_sq_scan, k_ivf_sq8_scan), persistent: the workgroups walk the work items (item i
// of the grid-strided list belongs to the cell c with item_off[c] <= i < item_off[c + 1]: a binary search) -- only rows somebody probes are
// ever touched, so a call's cost follows the rows it scans, not the shard.  Per item: `stage(ra, nrows)` puts its nrows <= G consecutive stored
// rows, from position ra, in the kernel's LDS ONCE (coalesced: the store is in cell order), between two barriers; then every (pair, row) unit
// -- a query that probes the cell, named by the pair's slot = query * nprobe + j, and row rr of the group -- is scored by one half-wave:
// `score(rr, query, slot)`, the query row streamed from L2.  The word goes to words[query * max_scan + seg_off[slot] + (row's position inside
// its cell)] -- the contract with k_ivf_plan, k_ivf_select and k_ivf_range: inside the query's segment by the plan's own sums over the same
// list_off, whatever list_off holds; rows outside [0, N) are never read, and an original row outside it becomes a word of 0 and is counted.
// SEL (the *_sel entries): `sel` is a row selector's bitmap over the original rows [0, N) (lrx_search_selector.h).  Per item the
// first two waves test the group's rows ONCE -- row_ids[r] -> bit, a ballot per wave -- into a workgroup-shared mask of <= 128 bits; a group
// with no selected row is NOT staged (the skip is workgroup-uniform and both barriers stay), and a unit whose row is deselected writes the
// null word 0ull WITHOUT calling score(): the words are not cleared between calls or chunks, so a word left unwritten would be an earlier
// search's hit.  An original row outside [0, N) has no bit: it stays on the unfiltered path (a word of 0, counted).  SEL = false is the walk
// without a selector, the only one the plain entries launch: no mask, no extra barrier, `sel` never read.
template <bool SEL, class Stage, class Score>
__device__ __forceinline__ void ivf_scan_items(int64_t N, int G, const int64_t* __restrict__ list_off, const int64_t* __restrict__ row_ids, int nlist,
                                               int nprobe, const unsigned long long* __restrict__ sorted, const unsigned int* __restrict__ cell_off,
                                               const unsigned int* __restrict__ item_off, unsigned int item_cap, const unsigned int* __restrict__ seg_off,
                                               int64_t max_scan, unsigned long long* __restrict__ words, const uint32_t* __restrict__ sel, Stage stage, Score score) {
  const int lane = threadIdx.x & 63, hw = threadIdx.x >> 5;
  const unsigned int n_items = min(item_off[nlist], item_cap);
  unsigned int bad = 0;
  for (unsigned int it = blockIdx.x; it < n_items; it += gridDim.x) {
    int lo = 0, hi = nlist;                                  // the last cell with item_off[c] <= it
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (item_off[mid] <= it) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int64_t ca = list_off[c], cb = list_off[c + 1];
    const int64_t ra = ca + (int64_t)(it - item_off[c]) * G;
    int64_t rb = ra + G;
    rb = rb < cb ? rb : cb;
    rb = rb < N ? rb : N;
    const unsigned int p0 = cell_off[c], np = cell_off[c + 1] - p0;
    if (ra < ca || ra < 0 || rb <= ra || np == 0) continue;  // (workgroup-uniform)
    const int nrows = (int)(rb - ra);
    __syncthreads();                                         // the previous item's rows are no longer read
    unsigned long long m0 = ~0ull, m1 = ~0ull;               // SEL: rows 0..63 / 64..127 of the group that are scored
    if constexpr (SEL) {
      __shared__ unsigned long long s_on[IVF_MAX_GROUP_ROWS / 64];
      if (threadIdx.x < IVF_MAX_GROUP_ROWS) {                // (two whole waves)
        bool on = false;
        if ((int)threadIdx.x < nrows) {
          const int64_t r = ra + threadIdx.x;
          const int64_t orig = row_ids != nullptr ? row_ids[r] : r;
          on = !(orig >= 0 && orig < N) || sel_test(sel, orig);
        }
        const unsigned long long bal = __ballot(on);
        if (lane == 0) s_on[threadIdx.x >> 6] = bal;
      }
      __syncthreads();
      m0 = s_on[0];
      m1 = s_on[1];
    }
    if (!SEL || (m0 | m1) != 0ull) stage(ra, nrows);         // (workgroup-uniform: the mask is the workgroup's)
    __syncthreads();
    const unsigned int units = np * (unsigned int)nrows;     // (at most IVF_MAX_CHUNK pairs x 128 rows)
    for (unsigned int u = hw; u < units; u += ROWGRP_THREADS / 32) {
      const unsigned int pi = u / (unsigned int)nrows;
      const int rr = (int)(u - pi * (unsigned int)nrows);
      const int64_t r = ra + rr;
      const unsigned int slot = (unsigned int)sorted[p0 + pi];
      const unsigned int qi = slot / (unsigned int)nprobe;
      if constexpr (SEL) {
        if (!(((rr < 64 ? m0 : m1) >> (rr & 63)) & 1ull)) {  // (uniform over the half-wave)
          if ((lane & 31) == 0) words[(int64_t)qi * max_scan + seg_off[slot] + (r - ca)] = 0ull;
          continue;
        }
      }
      const float sc = score(rr, qi, slot);
      if ((lane & 31) == 0) {
        const int64_t orig = row_ids != nullptr ? row_ids[r] : r;
        const bool ok = orig >= 0 && orig < N;               // (a word of 0 is nobody's row: the selection drops it)
        if (!ok) ++bad;
        words[(int64_t)qi * max_scan + seg_off[slot] + (r - ca)] = ok ? sel_pack(f2key(sc), orig) : 0ull;
      }
    }
  }
  if (bad) atomicAdd(&g_ivf_bad, bad);
}

// The base term of a pair in the scans over residual codes: the caller's score of the cell for that query, read through the pair's slot --
// probe_scores[query * ld_probe + slot % nprobe] (NULL: 0).
__device__ __forceinline__ double ivf_probe_base(const float* __restrict__ probe_scores, int64_t ld_probe, int nprobe, unsigned int qi, unsigned int slot) {
  return probe_scores != nullptr ? (double)probe_scores[(int64_t)qi * ld_probe + (slot - qi * (unsigned int)nprobe)] : 0.0;
}

// The scan over fp32 rows: a group is staged as it is stored, a pair's score is exact_dot_lds_row's (the bits of exact_dot).
template <bool SEL>
__global__ void __launch_bounds__(ROWGRP_THREADS)
k_ivf_scan(const float* __restrict__ X, int64_t N, int64_t ldx, int D, int G, const int64_t* __restrict__ list_off, const int64_t* __restrict__ row_ids,
           int nlist, const float* __restrict__ q, int nprobe, const unsigned long long* __restrict__ sorted, const unsigned int* __restrict__ cell_off,
           const unsigned int* __restrict__ item_off, unsigned int item_cap, const unsigned int* __restrict__ seg_off, int64_t max_scan,
           unsigned long long* __restrict__ words, const uint32_t* __restrict__ sel) {
  __shared__ __attribute__((aligned(16))) float s_x[ROWGRP_LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63;
  ivf_scan_items<SEL>(N, G, list_off, row_ids, nlist, nprobe, sorted, cell_off, item_off, item_cap, seg_off, max_scan, words, sel,
    [&](int64_t ra, int nrows) {
      for (int i = tid * 4; i < nrows * D; i += ROWGRP_THREADS * 4) {
        const int rr = i / D, cc = i - rr * D;
        *(f32x4*)(s_x + i) = REF_ROW_LOAD((const f32x4*)(X + (ra + rr) * ldx + cc));
      }
    },
    [&](int rr, unsigned int qi, unsigned int) { return exact_dot_lds_row(s_x + rr * D, q + (int64_t)qi * D, D, lane); });
}

// radix_select_kth_list over the LOW words of the entries whose key is `key_hi`: the kk-th largest of them (ties inside one score)
template <class SH>
__device__ uint32_t ivf_select_kth_low(const unsigned long long* __restrict__ list, int n, uint32_t key_hi, unsigned int kk, SH& sh) {
  const int tid = threadIdx.x, wave = tid >> 6, NT = blockDim.x;
  uint32_t prefix = 0, mask = 0;
  unsigned int neq;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 16 * 256; i += NT) (&sh.hist[0][0])[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
      const unsigned long long w = list[i];
      const uint32_t low = (uint32_t)w;
      if ((uint32_t)(w >> 32) == key_hi && (low & mask) == prefix) atomicAdd(&sh.hist[wave][(low >> shift) & 255], 1u);
    }
    prefix |= (uint32_t)radix_pick(sh, kk, neq) << shift;
    mask |= 0xFFu << shift;
  }
  return prefix;
}

// One workgroup per query: the top k of its segment, (score desc, original row asc) -- the packed words are distinct, so the order is total --
// and (-FLT_MAX, -1) beyond the rows it scanned.
__global__ void __launch_bounds__(1024)
k_ivf_select(const unsigned long long* __restrict__ words, int64_t max_scan, const int64_t* __restrict__ q_tot, int k, int64_t id_base,
             const int64_t* __restrict__ row_map, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  __shared__ RadixShared rs;
  __shared__ unsigned long long s_cand[IVF_SEL_SORT];
  __shared__ unsigned int s_ngt, s_neq, s_take;
  const int tid = threadIdx.x, qi = blockIdx.x;
  float* os = out_scores + (int64_t)qi * k;
  int64_t* oi = out_ids + (int64_t)qi * k;
  const unsigned long long* list = words + (int64_t)qi * max_scan;
  const int64_t tot = q_tot[qi];
  const int n = tot < 0 ? 0 : (int)tot;
  for (int i = tid; i < k; i += 1024) { os[i] = -FLT_MAX; oi[i] = -1; }
  if (n == 0) return;
  __syncthreads();                                           // the padding above is written before any result lands on it
  auto put = [&](int r, unsigned long long c) {
    const int64_t row = sel_row(c);
    os[r] = key2f((uint32_t)(c >> 32));
    oi[r] = row_map != nullptr ? row_map[row] : id_base + row;
  };
  int nc = n;                                                // entries of s_cand
  if (n <= IVF_SEL_SORT) {
    for (int i = tid; i < n; i += 1024) s_cand[i] = list[i];
  } else {
    // the k-th largest word: its score by the radix select over the keys, then -- only when equal scores straddle rank k -- its row
    const unsigned int kk = (unsigned int)k;                 // (k <= 2048 < n)
    const uint32_t kth = radix_select_kth_list(list, n, kk, rs);
    if (tid == 0) { s_ngt = 0; s_neq = 0; s_take = 0; }
    __syncthreads();
    unsigned int gt = 0, eq = 0;
    for (int i = tid; i < n; i += 1024) {
      const uint32_t key = (uint32_t)(list[i] >> 32);
      gt += key > kth ? 1u : 0u;
      eq += key == kth ? 1u : 0u;
    }
    if (gt) atomicAdd(&s_ngt, gt);
    if (eq) atomicAdd(&s_neq, eq);
    __syncthreads();
    const unsigned int need = kk - s_ngt, neq = s_neq;       // 1 <= need <= neq
    __syncthreads();
    const uint32_t low_thr = neq > need ? ivf_select_kth_low(list, n, kth, need, rs) : 0u;
    for (int i = tid; i < n; i += 1024) {
      const unsigned long long w = list[i];
      const uint32_t key = (uint32_t)(w >> 32);
      if (w != 0ull && (key > kth || (key == kth && (uint32_t)w >= low_thr))) {
        const unsigned int p = atomicAdd(&s_take, 1u);
        if (p < IVF_SEL_SORT) s_cand[p] = w;
      }
    }
    __syncthreads();
    nc = (int)min(s_take, (unsigned int)IVF_SEL_SORT);
  }
  __syncthreads();
  if (nc <= 1024) {
    // rank by counting, as k_rerank_merge does for its short lists (words of 0 -- rows outside the shard -- are equal: ranks by position)
    if (tid < nc) {
      const unsigned long long me = s_cand[tid];
      int r = 0;
      for (int j = 0; j < nc; ++j) {
        const unsigned long long o = s_cand[j];
        r += (o > me || (o == me && j < tid)) ? 1 : 0;
      }
      if (r < k && me != 0ull) put(r, me);
    }
    return;
  }
  for (int i = nc + tid; i < IVF_SEL_SORT; i += 1024) s_cand[i] = 0ull;
  bitonic_sort_desc_regs<2>(s_cand, IVF_SEL_SORT);           // (loads after its own barrier: the zero fill above is seen)
  const int n_out = nc < k ? nc : k;
  for (int i = tid; i < n_out; i += 1024) {
    const unsigned long long c = s_cand[i];
    if (c != 0ull) put(i, c);
  }
}

// RANGE SEARCH over the probed cells (faiss IndexIVF::range_search_preassigned): the chain above with k_ivf_select replaced
// by k_ivf_range<false> (count), k_range_lims (lrx_search_range.h) and k_ivf_range<true> (fill).  One workgroup per query walks its segment
// in 1024-word tiles, word i of a tile on thread i; a hit is a non-null word whose score -- key2f of its key, the value k_ivf_select reports --
// is > radius as a float comparison.  scanned == 0: the scan did not run (a shard without rows), the segment holds nothing.
//   FILL = false   surv[query] = its hits (0 for a query over max_scan_rows).
//   FILL = true    the hits leave in SEGMENT order -- cells in probe order, rows by stored position -- by a stable compaction: the rank of a
//                  hit is the hits of the tiles before (a running base, uniform over the workgroup) + those of the waves before it in its
//                  tile (wave totals through LDS) + those of the lanes below it (ballot and popcount).  No atomics: the order is by
//                  construction, and the slot lims[query] + rank is below lims[query + 1] <= *lims_end <= capacity because both passes
//                  evaluate one predicate over the same words.  Nothing is written when the chunk's results do not fit: *lims_end > capacity.
template <bool FILL>
__global__ void __launch_bounds__(1024)
k_ivf_range(const unsigned long long* __restrict__ words, int64_t max_scan, const int64_t* __restrict__ q_tot, int scanned, float radius,
            unsigned int* __restrict__ surv, const int64_t* __restrict__ lims, const int64_t* __restrict__ lims_end, int64_t capacity, int64_t id_base,
            const int64_t* __restrict__ row_map, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  __shared__ unsigned int s_w[2][16];                        // wave totals, double-buffered: one barrier per tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, qi = blockIdx.x;
  if (FILL && *lims_end > capacity) return;                  // (workgroup-uniform)
  const int64_t tot = scanned ? q_tot[qi] : 0;
  const int n = tot < 0 ? 0 : (int)tot;
  const unsigned long long* list = words + (int64_t)qi * max_scan;
  const int64_t base = FILL ? lims[qi] : 0;
  unsigned int run = 0;                                      // FILL: hits of the tiles before (uniform); else: this thread's hits
  int buf = 0;
  for (int64_t t0 = 0; t0 < n; t0 += 1024, buf ^= 1) {        // (64-bit: n may lie within 1024 of 2^31)
    const int64_t i = t0 + tid;
    const unsigned long long w = i < n ? list[i] : 0ull;
    const float sc = key2f((uint32_t)(w >> 32));
    const bool hit = w != 0ull && sc > radius;
    if (!FILL) {
      run += hit ? 1u : 0u;
      continue;
    }
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_w[buf][wave] = (unsigned int)__popcll(bal);
    __syncthreads();
    unsigned int before = 0, all = 0;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const unsigned int c = s_w[buf][v];
      before += v < wave ? c : 0u;
      all += c;
    }
    if (hit) {
      const int64_t pos = base + run + before + (unsigned int)__popcll(bal & ((1ull << lane) - 1ull));
      const int64_t row = sel_row(w);
      out_scores[pos] = sc;
      out_ids[pos] = row_map != nullptr ? row_map[row] : id_base + row;
    }
    run += all;
  }
  if (!FILL) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) run += __shfl_down(run, o, 64);
    if (lane == 0) s_w[0][wave] = run;
    __syncthreads();
    if (tid == 0) {
      unsigned int all = 0;
      for (int v = 0; v < 16; ++v) all += s_w[0][v];
      surv[qi] = all;
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
static int ivf_chunk_queries(int32_t n_queries, int64_t max_scan_rows) {
  const size_t per = (size_t)(max_scan_rows > 0 ? max_scan_rows : 1) * 8;
  size_t c = IVF_WORDS_BYTES / per;
  c = c < 1 ? 1 : (c > IVF_MAX_CHUNK ? IVF_MAX_CHUNK : c);
  const size_t nq = n_queries > 0 ? (size_t)n_queries : 1;
  return (int)(c < nq ? c : nq);
}

// ints: total | cell_cnt[nlist]   cell_off[nlist + 1]   item_off[nlist + 1]   pairs   sorted   seg_off   q_tot   words
struct IvfPlan {
  size_t off_celloff, off_itemoff, off_pairs, off_sorted, off_seg, off_tot, off_words, total;
};
static IvfPlan ivf_plan(int32_t nlist, int32_t nq, int32_t nprobe, int64_t max_scan_rows) {
  IvfPlan p;
  const size_t nl = nlist > 0 ? (size_t)nlist : 1, np = (size_t)nq * (size_t)(nprobe > 0 ? nprobe : 1);
  p.off_celloff = align256((nl + 1) * sizeof(unsigned int));
  p.off_itemoff = p.off_celloff + align256((nl + 1) * sizeof(unsigned int));
  p.off_pairs = p.off_itemoff + align256((nl + 1) * sizeof(unsigned int));
  p.off_sorted = p.off_pairs + align256(np * 8);
  p.off_seg = p.off_sorted + align256(np * 8);
  p.off_tot = p.off_seg + align256(np * sizeof(unsigned int));
  p.off_words = p.off_tot + align256((size_t)nq * sizeof(int64_t));
  p.total = p.off_words + align256((size_t)nq * (size_t)(max_scan_rows > 0 ? max_scan_rows : 0) * 8 + 8);
  return p;
}

extern "C" size_t lrx_ivf_flat_ip_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int32_t k,
                                                  int64_t max_scan_rows) {
  (void)n_rows; (void)dim; (void)k;
  return ivf_plan(nlist, ivf_chunk_queries(n_queries, max_scan_rows), nprobe, max_scan_rows).total;
}

// How the segments of a call leave the chain: the sorted top k of each (k_ivf_select), or every word above a radius (k_ivf_range; contract of
// lrx_ivf_flat_ip_range_search in include/lrx.h).  The two host drivers -- ivf_cell_major_search below and ivf_pq_run (lrx_search_ivfpq.h) --
// take one, so a search and its range search are ONE chain and one set of argument checks up to this point.
struct IvfOut {
  bool range;
  int32_t k;                                // top k: out_scores / out_ids are [n_queries, k]
  float radius;                             // range: hits are the words with a score > radius, ...
  int64_t* lims;                            //   ... query i's at [lims[i], lims[i + 1]) of out_scores / out_ids (device, [n_queries + 1]) ...
  int64_t capacity;                         //   ... which hold this many entries: a chunk that does not fit writes lims alone
  int64_t id_base;
  const int64_t* row_map;
  float* out_scores;
  int64_t* out_ids;
};
static IvfOut ivf_out_topk(int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map) {
  return IvfOut{false, k, 0.f, nullptr, 0, id_base, row_map, out_scores, out_ids};
}
static IvfOut ivf_out_range(float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity, const int64_t* row_map) {
  return IvfOut{true, 0, radius, lims, capacity, id_base, row_map, out_scores, out_ids};
}

// The checks of the output side that need no pointer but lims (made before the n_queries == 0 return)
static int ivf_out_check(const char* who, const IvfOut& o) {
  if (!o.range) {
    LRX_CHECK_ARG(o.k >= 1 && o.k <= SEL_MAXK, "%s: k=%d out of range (1..%d)", who, o.k, SEL_MAXK);
    return LRX_OK;
  }
  LRX_CHECK_ARG(o.radius == o.radius, "%s: radius is NaN", who);
  LRX_CHECK_ARG(o.capacity >= 0, "%s: capacity=%lld must be >= 0", who, (long long)o.capacity);
  LRX_CHECK_ARG(o.lims != nullptr, "%s: null lims", who);
  return LRX_OK;
}
// ... and of its pointers (a range search with capacity 0 writes lims alone)
static bool ivf_out_ptrs_ok(const IvfOut& o) { return (o.out_scores != nullptr && o.out_ids != nullptr) || (o.range && o.capacity == 0); }
// n_queries == 0: a top-k search has nothing to write, a range search writes lims[0] = 0
static int ivf_out_empty(const IvfOut& o, hipStream_t s) {
  if (o.range) LRX_HIP(hipMemsetAsync(o.lims, 0, sizeof(int64_t), s));
  return LRX_OK;
}
// The range search's own workspace, behind the search's: one uint32 hit count per query of a chunk
static size_t ivf_out_ws_bytes(bool range, int chunk) { return range ? align256((size_t)(chunk > 0 ? chunk : 1) * sizeof(unsigned int)) : 0; }

// The end of a chunk (its queries start at q0 of the call's): surv is the range search's workspace; scanned: the scan ran.
static int ivf_out_launch(const IvfOut& o, hipStream_t s, const unsigned long long* words, int64_t max_scan_rows, const int64_t* q_tot, unsigned int* surv,
                          int q0, int nq, int scanned) {
  if (!o.range) {
    hipLaunchKernelGGL(k_ivf_select, dim3(nq), dim3(1024), 0, s, words, max_scan_rows, q_tot, (int)o.k, o.id_base, o.row_map,
                       o.out_scores + (int64_t)q0 * o.k, o.out_ids + (int64_t)q0 * o.k);
    LRX_LAUNCH_CHECK();
    return LRX_OK;
  }
  int64_t* lc = o.lims + q0;                                 // this chunk's lims: lc[0] was written by the chunk before
  hipLaunchKernelGGL(k_ivf_range<false>, dim3(nq), dim3(1024), 0, s, words, max_scan_rows, q_tot, scanned, o.radius, surv, (const int64_t*)lc,
                     (const int64_t*)lc + nq, o.capacity, o.id_base, o.row_map, o.out_scores, o.out_ids);
  LRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_range_lims, dim3(1), dim3(1024), 0, s, (const unsigned int*)surv, nq, lc, q0 == 0 ? 1 : 0);
  LRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ivf_range<true>, dim3(nq), dim3(1024), 0, s, words, max_scan_rows, q_tot, scanned, o.radius, surv, (const int64_t*)lc,
                     (const int64_t*)lc + nq, o.capacity, o.id_base, o.row_map, o.out_scores, o.out_ids);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

// What a cell-major scan is handed per chunk (ivf_cell_major_search below): the chunk's queries start at q0 of the call's.
struct IvfScanArgs {
  hipStream_t stream;
  unsigned int grid;
  int q0, G;
  const float* q;                           // the chunk's query rows
  const unsigned long long* sorted;
  const unsigned int *cell_off, *item_off, *seg_off;
  unsigned int item_cap;
  unsigned long long* words;
  const uint32_t* sel;                      // the selector's bitmap (the scan's SEL instantiation), or NULL (the plain one)
};

// A row selector as the *_sel entries take it: `bits` NULL = none (the plain entry); otherwise a bitmap over `rows` == n_rows original rows.
struct IvfSel {
  const uint32_t* bits;
  int64_t rows;
};
static const IvfSel IVF_NO_SEL = {nullptr, 0};
static int ivf_sel_check(const char* who, const IvfSel& sel, int64_t n_rows) {
  LRX_CHECK_ARG(sel.bits == nullptr || sel.rows == n_rows, "%s: sel_rows=%lld is not the rows of the index (n_rows=%lld)", who, (long long)sel.rows,
                (long long)n_rows);
  return LRX_OK;
}

// The host driver of the CELL-MAJOR chain, shared by lrx_ivf_flat_ip_search and lrx_ivf_sq_fp16_ip_search (lrx_search_ivfsq.h): the argument
// checks both contracts have in common (`who` names the entry in the messages; rows_ok / rows_why: the entry's own check of its row store, made
// by the caller), the workspace, and per chunk k_ivf_clear, k_ivf_plan<false>, k_ivf_items, k_pairs_scatter, the entry's scan -- launched by
// `scan(const IvfScanArgs&)` over groups of G stored rows -- and the end `out` asks for: k_ivf_select, or the three kernels of the range search
// (the *_range_search entries are this driver with an IvfOut of the other kind).  Kernels only, one stream, nothing read back.
template <class Scan>
static int ivf_cell_major_search(const char* who, const void* rows, bool rows_ok, const char* rows_why, int G, int64_t n_rows, int32_t dim,
                                 const int64_t* list_off, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe,
                                 int64_t ld_probe, int64_t max_scan_rows, const IvfOut& out, const IvfSel& sel, void* workspace, size_t workspace_bytes,
                                 void* stream, Scan scan) {
  LRX_CHECK_ARG(dim >= 32 && dim <= 8192 && dim % 32 == 0, "%s: dim=%d must be a multiple of 32 in 32..8192", who, dim);
  if (int rc = ivf_out_check(who, out)) return rc;
  LRX_CHECK_ARG(nlist >= 1, "%s: nlist=%d must be >= 1", who, nlist);
  LRX_CHECK_ARG(nprobe >= 1 && nprobe <= IVF_MAX_NPROBE && nprobe <= nlist, "%s: nprobe=%d out of range (1..min(nlist=%d, %d))", who, nprobe, nlist,
                IVF_MAX_NPROBE);
  LRX_CHECK_ARG(ld_probe >= nprobe, "%s: ld_probe=%lld < nprobe=%d", who, (long long)ld_probe, nprobe);
  LRX_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 32), "%s: rows=%lld out of range", who, (long long)n_rows);
  LRX_CHECK_ARG(max_scan_rows >= 0 && max_scan_rows < (1ll << 31), "%s: max_scan_rows=%lld out of range (0..2^31 - 1)", who, (long long)max_scan_rows);
  LRX_CHECK_ARG(rows_ok, "%s: %s", who, rows_why);
  if (int rc = ivf_sel_check(who, sel, n_rows)) return rc;
  LRX_CHECK_ARG(n_queries >= 0, "%s: n_queries=%d", who, n_queries);
  hipStream_t s = (hipStream_t)stream;
  if (n_queries == 0) return ivf_out_empty(out, s);
  LRX_CHECK_ARG(q != nullptr && probes != nullptr && list_off != nullptr && ivf_out_ptrs_ok(out) && (rows != nullptr || n_rows == 0), "%s: null pointer", who);
  LRX_CHECK_ARG((uintptr_t)q % 16 == 0, "%s: q must be 16-byte aligned", who);
  const int chunk = ivf_chunk_queries(n_queries, max_scan_rows);
  const IvfPlan p = ivf_plan(nlist, chunk, nprobe, max_scan_rows);
  const size_t need = p.total + ivf_out_ws_bytes(out.range, chunk);
  if (workspace == nullptr || workspace_bytes < need) {
    lrx_set_error("%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
    return LRX_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  unsigned int* total = (unsigned int*)ws;
  unsigned int* cell_cnt = total + 1;
  unsigned int* cell_off = (unsigned int*)(ws + p.off_celloff);
  unsigned int* item_off = (unsigned int*)(ws + p.off_itemoff);
  unsigned long long* pairs = (unsigned long long*)(ws + p.off_pairs);
  unsigned long long* sorted = (unsigned long long*)(ws + p.off_sorted);
  unsigned int* seg_off = (unsigned int*)(ws + p.off_seg);
  int64_t* q_tot = (int64_t*)(ws + p.off_tot);
  unsigned long long* words = (unsigned long long*)(ws + p.off_words);
  unsigned int* surv = (unsigned int*)(ws + p.total);        // (the range search's)
  const int64_t ngroups = lrx_cdiv(n_rows, G);
  const int64_t item_cap = ngroups + nlist;                  // a cell's last group may be partial
  const int64_t scan_wgs = item_cap < 8 * (int64_t)lrx_cu_count() ? item_cap : 8 * (int64_t)lrx_cu_count();
  for (int q0 = 0; q0 < n_queries; q0 += chunk) {
    const int nq = n_queries - q0 < chunk ? n_queries - q0 : chunk;
    hipLaunchKernelGGL(k_ivf_clear, dim3((unsigned)lrx_cdiv((int64_t)nlist + 1, 256)), dim3(256), 0, s, total, (int)nlist + 1);
    LRX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ivf_plan<false>, dim3(nq), dim3(IVF_PLAN_THREADS), 0, s, probes + (int64_t)q0 * ld_probe, (int)nprobe, ld_probe, list_off, (int)nlist,
                       max_scan_rows, pairs, (unsigned int)((int64_t)nq * nprobe), total, cell_cnt, seg_off, q_tot);
    LRX_LAUNCH_CHECK();
    if (ngroups > 0) {
      hipLaunchKernelGGL(k_ivf_items, dim3(1), dim3(1024), 0, s, (const unsigned int*)cell_cnt, list_off, (int)nlist, n_rows, G, cell_off, item_off);
      LRX_LAUNCH_CHECK();
      const int64_t sb = lrx_cdiv((int64_t)nq * nprobe, 256);
      hipLaunchKernelGGL(k_pairs_scatter, dim3((unsigned)(sb < 1024 ? sb : 1024)), dim3(256), 0, s, (const unsigned long long*)pairs, (const unsigned int*)total,
                         cell_cnt, (const unsigned int*)cell_off, 0, sorted);
      LRX_LAUNCH_CHECK();
      IvfScanArgs a;
      a.stream = s; a.grid = (unsigned)scan_wgs; a.q0 = q0; a.G = G; a.q = q + (int64_t)q0 * dim;
      a.sorted = sorted; a.cell_off = cell_off; a.item_off = item_off; a.seg_off = seg_off;
      a.item_cap = (unsigned int)(item_cap < 0xFFFFFFFFll ? item_cap : 0xFFFFFFFFll);
      a.words = words;
      a.sel = sel.bits;
      scan(a);
      LRX_LAUNCH_CHECK();
    }
    if (int rc = ivf_out_launch(out, s, words, max_scan_rows, q_tot, surv, q0, nq, ngroups > 0 ? 1 : 0)) return rc;
  }
  return LRX_OK;
}

// lrx_ivf_flat_ip_search and lrx_ivf_flat_ip_range_search: the driver over k_ivf_scan
static int ivf_flat_run(const char* who, const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                        const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe, int64_t max_scan_rows, const IvfOut& out,
                        const IvfSel& sel, void* workspace, size_t workspace_bytes, void* stream) {
  char why[128];
  snprintf(why, sizeof(why), "rows must be 16-byte aligned (ldx=%lld >= dim=%d, ldx %% 4 == 0)", (long long)ldx, dim);
  return ivf_cell_major_search(who, X, ldx >= dim && ldx % 4 == 0 && (uintptr_t)X % 16 == 0, why, dim > 0 ? ivf_group_rows(dim) : 1, n_rows, dim, list_off, nlist,
                               q, n_queries, probes, nprobe, ld_probe, max_scan_rows, out, sel, workspace, workspace_bytes, stream, [&](const IvfScanArgs& a) {
    auto* kern = a.sel != nullptr ? k_ivf_scan<true> : k_ivf_scan<false>;
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(ROWGRP_THREADS), 0, a.stream, X, n_rows, ldx, (int)dim, a.G, list_off, row_ids, (int)nlist, a.q,
                       (int)nprobe, a.sorted, a.cell_off, a.item_off, a.item_cap, a.seg_off, max_scan_rows, a.words, a.sel);
  });
}

extern "C" int lrx_ivf_flat_ip_search(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                                      const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe, int64_t max_scan_rows,
                                      int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return ivf_flat_run("ivf_flat_ip_search", X, n_rows, ldx, dim, list_off, row_ids, nlist, q, n_queries, probes, nprobe, ld_probe, max_scan_rows,
                      ivf_out_topk(k, id_base, out_scores, out_ids, row_map), IVF_NO_SEL, workspace, workspace_bytes, stream);
}

// The search under a row selector (lrx_search_selector.h): sel_bits == NULL is lrx_ivf_flat_ip_search.
extern "C" int lrx_ivf_flat_ip_search_sel(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids,
                                          int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe,
                                          int64_t max_scan_rows, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map,
                                          const uint32_t* sel_bits, int64_t sel_rows, void* workspace, size_t workspace_bytes, void* stream) {
  return ivf_flat_run("ivf_flat_ip_search_sel", X, n_rows, ldx, dim, list_off, row_ids, nlist, q, n_queries, probes, nprobe, ld_probe, max_scan_rows,
                      ivf_out_topk(k, id_base, out_scores, out_ids, row_map), IvfSel{sel_bits, sel_rows}, workspace, workspace_bytes, stream);
}

// The workspace of the cell-major range searches (flat, fp16 codes, 8-bit codes): the search's plus the hit counts of a chunk
extern "C" size_t lrx_ivf_flat_ip_range_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int64_t max_scan_rows) {
  return lrx_ivf_flat_ip_workspace_bytes(n_rows, nlist, dim, n_queries, nprobe, 1, max_scan_rows) +
         ivf_out_ws_bytes(true, ivf_chunk_queries(n_queries, max_scan_rows));
}

extern "C" int lrx_ivf_flat_ip_range_search(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids,
                                            int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe,
                                            int64_t max_scan_rows, float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids,
                                            int64_t capacity, const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream) {
  return ivf_flat_run("ivf_flat_ip_range_search", X, n_rows, ldx, dim, list_off, row_ids, nlist, q, n_queries, probes, nprobe, ld_probe, max_scan_rows,
                      ivf_out_range(radius, id_base, lims, out_scores, out_ids, capacity, row_map), IVF_NO_SEL, workspace, workspace_bytes, stream);
}

extern "C" int lrx_ivf_flat_ip_range_search_sel(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids,
                                                int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe,
                                                int64_t max_scan_rows, float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids,
                                                int64_t capacity, const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace,
                                                size_t workspace_bytes, void* stream) {
  return ivf_flat_run("ivf_flat_ip_range_search_sel", X, n_rows, ldx, dim, list_off, row_ids, nlist, q, n_queries, probes, nprobe, ld_probe, max_scan_rows,
                      ivf_out_range(radius, id_base, lims, out_scores, out_ids, capacity, row_map), IvfSel{sel_bits, sel_rows}, workspace, workspace_bytes,
                      stream);
}
