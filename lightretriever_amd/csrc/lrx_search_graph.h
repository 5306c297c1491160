// liblrx search, part G -- GRAPH: beam search over a fixed-degree neighbour graph (the role of faiss GpuIndexCagra / IndexHNSWCagra) and the
// one integer kernel of its build: k_graph_search, lrx_graph_ip_search, k_graph_detours, lrx_graph_detour_counts (contract: include/lrx.h).
// Part of the ONE translation unit lrx_search.hip (included at its end: it reuses row_dot / f2key / key2f).  Not a stand-alone header.
#pragma once

#define GRAPH_THREADS 512                 // 16 half-waves: 16 rows in flight per workgroup, two workgroups per CU
#define GRAPH_MAX_BEAM 2048
#define GRAPH_MAX_CAND 1024               // rows one step (width * degree) or one slice of the entry list can bring
#define GRAPH_QLDS 4096                   // query rows up to this many floats sit in LDS; longer ones are read from global memory (L2)
#define GRAPH_HASH 4096                   // slots of the visited table (int32 rows, open addressing)
#define GRAPH_HASH_FILL 3072              // most rows it ever holds (GRAPH_MAX_BEAM + GRAPH_MAX_CAND: a clear followed by one full gather)
#define GRAPH_ITEMS ((GRAPH_MAX_BEAM + GRAPH_MAX_CAND) / GRAPH_THREADS)   // words per thread of the merge

// Entry-list and graph entries >= n_rows the search skipped since the last reset: part of lrx_device_error_count (lrx_elementwise.hip).
__device__ unsigned int g_graph_bad_rows = 0;
unsigned int lrx_graph_bad_rows(int* ok, int reset) {
  unsigned int v = 0;
  *ok = hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_graph_bad_rows), sizeof(v)) == hipSuccess;
  if (*ok && reset && v) {
    const unsigned int z = 0;
    *ok = hipMemcpyToSymbol(HIP_SYMBOL(g_graph_bad_rows), &z, sizeof(z)) == hipSuccess;
  }
  return v;
}

// The beam's words: sel_pack's order -- an unsigned sort is (score desc, row asc) -- with the row in 31 bits and the EXPANDED mark in bit 0,
// so the mark travels with its entry.  A row is in the beam at most once, so the mark never decides a comparison.  0 = no entry.
__device__ __forceinline__ unsigned long long graph_pack(uint32_t key, int32_t row) {
  return ((unsigned long long)key << 32) | (unsigned long long)((0x7FFFFFFFu - (uint32_t)row) << 1);
}
__device__ __forceinline__ int32_t graph_row(unsigned long long w) { return (int32_t)(0x7FFFFFFFu - ((uint32_t)w >> 1)); }

struct GraphShared {
  unsigned long long beam[GRAPH_MAX_BEAM];        // sorted descending, nb entries
  unsigned long long cand[GRAPH_MAX_CAND];        // rows to score (low word), then their words; unordered
  int32_t hash[GRAPH_HASH];                       // the visited table: -1 = free
  __attribute__((aligned(16))) float q[GRAPH_QLDS];
  int32_t par[8];                                 // the rows a step expands
  unsigned int npar, ncand, bad;
};

// row -> the table; true when it was not there
__device__ __forceinline__ bool graph_visit(int32_t* hash, int32_t row) {
  unsigned int s = ((uint32_t)row * 2654435761u) >> 20;       // 12 bits: GRAPH_HASH slots
  for (;;) {
    const int32_t old = atomicCAS(&hash[s], -1, row);
    if (old == -1) return true;
    if (old == row) return false;
    s = (s + 1) & (GRAPH_HASH - 1);                            // (terminates: the table is never more than 3/4 full)
  }
}

// Score the sh.ncand rows of sh.cand (one half-wave per row, the gather of refine_rescore) and merge them into the beam: the beam becomes
// the best `beam` of (beam U rows).  Ranks by counting: the beam is sorted and the words are distinct, so an entry's place in the union is
// its place among its own kind plus the entries of the other kind above it -- one pass of broadcast LDS reads over the new words instead of
// the barrier-separated stages of a sort.  Every thread holds its words in registers across the one barrier that separates reading the old
// beam from writing the new one.  Returns the new beam length.
__device__ __forceinline__ int graph_score_merge(GraphShared& sh, const float* __restrict__ X, int64_t ldx, int D, const float* qrow, int nb, int beam) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nc = (int)sh.ncand;
  for (int c0 = wave * 2; c0 < nc; c0 += GRAPH_THREADS / 32) {
    const int c = min(c0 + (lane >> 5), nc - 1);
    const int32_t row = (int32_t)(uint32_t)sh.cand[c];
    const float sc = row_dot<ROWS_F32>(X, ldx, (int64_t)row, qrow, D, lane);
    // (a half-wave past the end rescored the last row, which its own wave holds: both halves read it before either writes)
    if ((lane & 31) == 0 && c0 + (lane >> 5) < nc) sh.cand[c] = graph_pack(f2key(sc), row);
  }
  __syncthreads();
  const int tot = nb + nc;
  unsigned long long w[GRAPH_ITEMS];
  int rank[GRAPH_ITEMS];
#pragma unroll
  for (int r = 0; r < GRAPH_ITEMS; ++r) {
    const int e = tid + r * GRAPH_THREADS;
    w[r] = e < nb ? sh.beam[e] : (e < tot ? sh.cand[e - nb] : 0ull);
    rank[r] = 0;
    if (e < nb) rank[r] = e;
    else if (e < tot) {                           // beam entries above a new word: the first position whose word is smaller
      int lo = 0, hi = nb;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sh.beam[mid] > w[r]) lo = mid + 1; else hi = mid;
      }
      rank[r] = lo;
    }
  }
  if (tid < tot)                                  // (a thread's first word is its only one unless tot > GRAPH_THREADS)
    for (int j = 0; j < nc; ++j) {
      const unsigned long long o = sh.cand[j];
#pragma unroll
      for (int r = 0; r < GRAPH_ITEMS; ++r) rank[r] += o > w[r] ? 1 : 0;   // (empty words, 0, are above nothing and are not written)
    }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < GRAPH_ITEMS; ++r)
    if (tid + r * GRAPH_THREADS < tot && rank[r] < beam) sh.beam[rank[r]] = w[r];
  __syncthreads();
  return tot < beam ? tot : beam;
}

// Forget every visited row but the beam's when the table could not take `incoming` more rows.
__device__ __forceinline__ void graph_make_room(GraphShared& sh, int& nvisited, int incoming, int nb) {
  if (nvisited + incoming <= GRAPH_HASH_FILL) return;
  for (int i = threadIdx.x; i < GRAPH_HASH; i += GRAPH_THREADS) sh.hash[i] = -1;
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += GRAPH_THREADS) graph_visit(sh.hash, graph_row(sh.beam[i]));
  __syncthreads();
  nvisited = nb;
}

// One workgroup per query; all state of the traversal lives in LDS (56 KiB), nothing is shared between workgroups.
__global__ void __launch_bounds__(GRAPH_THREADS)
k_graph_search(const float* __restrict__ X, int32_t N, int64_t ldx, int D, const int32_t* __restrict__ graph, int degree, const float* __restrict__ q,
               const int64_t* __restrict__ entry_rows, int n_entry, int64_t ld_entry, int k, int beam, int width, int max_iterations, int64_t id_base,
               float* __restrict__ out_scores, int64_t* __restrict__ out_ids, const int64_t* __restrict__ row_map, int32_t* __restrict__ out_stats) {
  __shared__ GraphShared sh;
  const int tid = threadIdx.x, qi = blockIdx.x;
  const float* qglob = q + (int64_t)qi * D;
  const float* qrow = D <= GRAPH_QLDS ? sh.q : qglob;
  if (D <= GRAPH_QLDS)
    for (int i = tid * 4; i < D; i += GRAPH_THREADS * 4) *(f32x4*)(sh.q + i) = *(const f32x4*)(qglob + i);
  for (int i = tid; i < GRAPH_HASH; i += GRAPH_THREADS) sh.hash[i] = -1;
  if (tid == 0) { sh.ncand = 0; sh.bad = 0; }
  __syncthreads();
  int nb = 0, nvisited = 0, scored = 0, iterations = 0;

  // start: the best `beam` of the distinct valid entry rows, a slice of GRAPH_MAX_CAND entries at a time
  const int64_t* entries = entry_rows + (int64_t)qi * ld_entry;
  for (int e0 = 0; e0 < n_entry; e0 += GRAPH_MAX_CAND) {
    const int ne = min(GRAPH_MAX_CAND, n_entry - e0);
    graph_make_room(sh, nvisited, ne, nb);
    for (int i = tid; i < ne; i += GRAPH_THREADS) {
      const int64_t row = entries[e0 + i];
      if (row < 0) continue;
      if (row >= (int64_t)N) atomicAdd(&sh.bad, 1u);
      else if (graph_visit(sh.hash, (int32_t)row)) sh.cand[atomicAdd(&sh.ncand, 1u)] = (unsigned long long)row;
    }
    __syncthreads();
    const int nc = (int)sh.ncand;
    nb = graph_score_merge(sh, X, ldx, D, qrow, nb, beam);
    nvisited += nc;
    scored += nc;
    if (tid == 0) sh.ncand = 0;
    __syncthreads();
  }

  for (; iterations < max_iterations; ++iterations) {
    // the first `width` beam entries not yet expanded, in beam order (wave 0: a ballot over 64 entries at a time)
    if (tid < 64) {
      int found = 0;
      for (int b0 = 0; b0 < nb && found < width; b0 += 64) {
        const int i = b0 + tid;
        const unsigned long long w = i < nb ? sh.beam[i] : 1ull;
        const bool open = (w & 1ull) == 0;
        const unsigned long long m = __ballot(open);
        const int r = found + __popcll(m & ((1ull << tid) - 1ull));
        if (open && r < width) {
          sh.par[r] = graph_row(w);
          sh.beam[i] = w | 1ull;
        }
        found += __popcll(m);
      }
      if (tid == 0) sh.npar = (unsigned int)(found < width ? found : width);
    }
    __syncthreads();
    const int npar = (int)sh.npar;
    if (npar == 0) break;                          // (uniform: every thread read the same word after the barrier)
    graph_make_room(sh, nvisited, npar * degree, nb);
    for (int i = tid; i < npar * degree; i += GRAPH_THREADS) {
      const int p = i / degree;
      const int32_t row = graph[(int64_t)sh.par[p] * degree + (i - p * degree)];
      if (row < 0) continue;
      if (row >= N) atomicAdd(&sh.bad, 1u);
      else if (graph_visit(sh.hash, row)) sh.cand[atomicAdd(&sh.ncand, 1u)] = (unsigned long long)(uint32_t)row;
    }
    __syncthreads();
    const int nc = (int)sh.ncand;
    nb = graph_score_merge(sh, X, ldx, D, qrow, nb, beam);
    nvisited += nc;
    scored += nc;
    if (tid == 0) sh.ncand = 0;
    __syncthreads();
  }

  float* os = out_scores + (int64_t)qi * k;
  int64_t* oi = out_ids + (int64_t)qi * k;
  for (int i = tid; i < k; i += GRAPH_THREADS) {
    if (i < nb) {
      const unsigned long long w = sh.beam[i];
      const int64_t row = graph_row(w);
      os[i] = key2f((uint32_t)(w >> 32));
      oi[i] = row_map != nullptr ? row_map[row] : id_base + row;
    } else {
      os[i] = -FLT_MAX;
      oi[i] = -1;
    }
  }
  if (tid == 0) {
    if (out_stats != nullptr) { out_stats[2 * qi] = iterations; out_stats[2 * qi + 1] = scored; }
    if (sh.bad) atomicAdd(&g_graph_bad_rows, sh.bad);
  }
}

// The traversal keeps everything in LDS: no global scratch is needed, whatever the arguments.
extern "C" size_t lrx_graph_ip_workspace_bytes(int32_t n_queries, int32_t n_entry, int32_t degree, int32_t beam, int32_t width) {
  (void)n_queries; (void)n_entry; (void)degree; (void)beam; (void)width;
  return 0;
}

extern "C" int lrx_graph_ip_search(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int32_t* graph, int32_t degree, const float* q,
                                   int32_t n_queries, const int64_t* entry_rows, int32_t n_entry, int64_t ld_entry, int32_t k, int32_t beam, int32_t width,
                                   int32_t max_iterations, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map,
                                   int32_t* out_stats, void* workspace, size_t workspace_bytes, void* stream) {
  LRX_CHECK_ARG(dim % 32 == 0 && dim >= 32 && dim <= 8192, "graph_ip_search: dim=%d must be a multiple of 32 (32 .. 8192)", dim);
  LRX_CHECK_ARG(ldx >= dim && ldx % 4 == 0 && (uintptr_t)X % 16 == 0, "graph_ip_search: rows must be 16-byte aligned (ldx=%lld >= dim=%d, ldx %% 4 == 0)",
                (long long)ldx, dim);
  LRX_CHECK_ARG(degree >= 8 && degree <= 128 && degree % 8 == 0, "graph_ip_search: degree=%d must be a multiple of 8 (8 .. 128)", degree);
  LRX_CHECK_ARG(beam >= 1 && beam <= GRAPH_MAX_BEAM && k >= 1 && k <= beam, "graph_ip_search: need 1 <= k <= beam <= %d, got k=%d, beam=%d", GRAPH_MAX_BEAM,
                k, beam);
  LRX_CHECK_ARG(width >= 1 && width <= 8 && width * degree <= GRAPH_MAX_CAND, "graph_ip_search: width=%d out of range (1 .. 8, width * degree=%d <= %d)",
                width, degree, GRAPH_MAX_CAND);
  LRX_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31), "graph_ip_search: n_rows=%lld out of range (0 .. 2^31 - 1)", (long long)n_rows);
  LRX_CHECK_ARG(n_entry >= 1 && n_entry <= 2048, "graph_ip_search: n_entry=%d out of range (1 .. 2048)", n_entry);
  LRX_CHECK_ARG(ld_entry >= n_entry, "graph_ip_search: ld_entry=%lld < n_entry=%d", (long long)ld_entry, n_entry);
  LRX_CHECK_ARG(max_iterations >= 0 && max_iterations <= 65536, "graph_ip_search: max_iterations=%d out of range (0 .. 65536)", max_iterations);
  LRX_CHECK_ARG(n_queries >= 0, "graph_ip_search: n_queries=%d", n_queries);
  if (n_queries == 0) return LRX_OK;
  LRX_CHECK_ARG(q != nullptr && entry_rows != nullptr && out_scores != nullptr && out_ids != nullptr && ((X != nullptr && graph != nullptr) || n_rows == 0),
                "graph_ip_search: null pointer");
  LRX_CHECK_ARG((uintptr_t)q % 16 == 0, "graph_ip_search: q must be 16-byte aligned");
  const size_t need = lrx_graph_ip_workspace_bytes(n_queries, n_entry, degree, beam, width);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need)) {
    lrx_set_error("graph_ip_search: workspace %zu B < required %zu B", workspace_bytes, need);
    return LRX_ERR_WORKSPACE;
  }
  const int iters = max_iterations > 0 ? max_iterations : (beam + width - 1) / width + 32;
  hipLaunchKernelGGL(k_graph_search, dim3(n_queries), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, X, (int32_t)n_rows, ldx, (int)dim, graph, (int)degree, q,
                     entry_rows, (int)n_entry, ld_entry, (int)k, (int)beam, (int)width, iters, id_base, out_scores, out_ids, row_map, out_stats);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

// ---- the build's detour counts ------------------------------------------------------------------------------------------------------
#define GRAPH_MAX_K 256                   // intermediate degree
#define DETOUR_SLOTS 1024                 // lookup of a row's own list: row -> its first position (load factor <= 1/4)

// One workgroup per row u.  u's list sits in LDS as a lookup (row -> position); thread b walks the lists of u's neighbours v = knn[u][a],
// a = 0 .. K - 1, one coalesced row of K entries per step, and counts w = knn[v][b] at its position c in u's list when c > max(a, b): the
// two-hop path u -> v -> w is a detour around the edge u -> w.  Integer work only; a list entry outside [0, n_rows) takes no part and is
// never turned into an address.
__global__ void __launch_bounds__(GRAPH_MAX_K)        // (launched with K rounded up to whole waves)
k_graph_detours(const int32_t* __restrict__ knn, int64_t N, int K, int32_t* __restrict__ counts) {
  __shared__ int32_t s_list[GRAPH_MAX_K], s_cnt[GRAPH_MAX_K];
  __shared__ int32_t s_key[DETOUR_SLOTS], s_pos[DETOUR_SLOTS];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  for (int i = tid; i < DETOUR_SLOTS; i += blockDim.x) { s_key[i] = -1; s_pos[i] = K; }
  int32_t mine = -1;
  if (tid < K) {
    mine = knn[u * K + tid];
    if (mine < 0 || (int64_t)mine >= N) mine = -1;
    s_list[tid] = mine;
    s_cnt[tid] = 0;
  }
  __syncthreads();
  if (mine >= 0) {
    unsigned int s = ((uint32_t)mine * 2654435761u) >> 22;     // 10 bits: DETOUR_SLOTS
    for (;;) {
      const int32_t old = atomicCAS(&s_key[s], -1, mine);
      if (old == -1 || old == mine) break;
      s = (s + 1) & (DETOUR_SLOTS - 1);
    }
    atomicMin(&s_pos[s], tid);                                 // (a row listed twice answers with its first position)
  }
  __syncthreads();
  if (tid < K)
    for (int a = 0; a < K; ++a) {
      const int32_t v = s_list[a];
      if (v < 0) continue;
      const int32_t w = knn[(int64_t)v * K + tid];
      if (w < 0) continue;
      unsigned int s = ((uint32_t)w * 2654435761u) >> 22;
      for (;;) {
        const int32_t key = s_key[s];
        if (key == w) {
          const int c = s_pos[s];
          if (c > (a > tid ? a : tid)) atomicAdd(&s_cnt[c], 1);
          break;
        }
        if (key == -1) break;
        s = (s + 1) & (DETOUR_SLOTS - 1);
      }
    }
  __syncthreads();
  if (tid < K) counts[u * K + tid] = s_cnt[tid];
}

extern "C" int lrx_graph_detour_counts(const int32_t* knn, int64_t n_rows, int32_t K, int32_t* counts, void* stream) {
  LRX_CHECK_ARG(K >= 1 && K <= GRAPH_MAX_K, "graph_detour_counts: K=%d out of range (1 .. %d)", K, GRAPH_MAX_K);
  LRX_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31), "graph_detour_counts: n_rows=%lld out of range (0 .. 2^31 - 1)", (long long)n_rows);
  if (n_rows == 0) return LRX_OK;
  LRX_CHECK_ARG(knn != nullptr && counts != nullptr, "graph_detour_counts: null pointer");
  hipLaunchKernelGGL(k_graph_detours, dim3((unsigned int)n_rows), dim3((K + 63) / 64 * 64), 0, (hipStream_t)stream, knn, n_rows, (int)K, counts);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}
