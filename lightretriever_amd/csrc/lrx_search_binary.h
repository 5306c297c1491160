// liblrx search, part 7 -- BINARY flat index (faiss IndexBinaryFlat + the reference's float rerank), map: section H.
// Part of the ONE translation unit lrx_search.hip (included at its end: it reuses bitonic_sort_desc, sel_pack / f2key and lrx_cu_count).  Not a
// stand-alone header.  Contract and code layout: include/lrx.h (lrx_binary_ip_search), DESIGN.md §5.4.4.
//
//     k_bin_pack         bit j = x[j] > threshold[j] (strict; NaN -> 0), np.packbits byte order; fp32 rows -> blocked codes, queries -> the scan's query tiles
//     k_bin_store        rows that arrive packed (uint8 [n, d / 8]) -> blocked codes
//     k_bin_scan<QT, M>  THE HOT PATH: one row per lane, h(q, r) = popcount(q ^ r) for a tile of QT queries whose words are wave-uniform (scalar
//                        loads), the row's 16-byte groups loaded once per query tile.  Three epilogues over the same scan (h is recomputed,
//                        never stored): M = 0 per-query histogram of h (LDS partials, integer atomics), M = 1 rows under the cutoff appended
//                        to the query's key list + ties counted per 1024-row tile, M = 2 the lowest ties placed by their rank in row order
//     k_bin_cut          cutoff t_q = the smallest h whose cumulative count reaches kk, need_eq = kk - count(h < t_q)
//     k_bin_tie_prefix   exclusive prefix of a query's per-tile tie counts, in row order
//     k_bin_sort         Hamming output: the <= 2048 (h, row) keys of a query sorted in LDS -> (D int32, I)
//     k_bin_rerank_score one wave per (query, candidate): (float) of the fp64 sum of +-q over the candidate's bits, the query row in LDS
//     k_bin_rerank_sort  (score desc, row asc) of a query's candidates in LDS -> (D fp32, I)
//     k_bin_decode       blocked codes -> row-major packed bytes (reconstruct_n, save)
#pragma once

#define BIN_BLK 128             // rows per code block (the PQ code layout with M = d / 8 bytes per row)
#define BIN_TILE 1024           // rows per scan tile: one row per lane
#define BIN_MAXK SEL_MAXK       // binary_k <= 2048: one LDS-resident sort per query
#define BIN_MAX_BITS 16384
#define BIN_HIST_FLUSH 63       // tiles between two flushes of the LDS histogram: its bins are 16 bits wide, 63 x 1024 < 65536
#define BIN_RR_CAND 16          // candidates per workgroup of the rerank (4 waves x 4)
#define BIN_RR_QMAX 65535       // queries per launch of the rerank scoring (grid.y)

static __host__ __device__ __forceinline__ int bin_groups(int d) { return (d + 127) / 128; }      // 16-byte groups per row
static __host__ __device__ __forceinline__ int64_t bin_code_off(int64_t r, int byte, int G) {
  return (r / BIN_BLK) * BIN_BLK * 16 * G + (int64_t)(byte >> 4) * (BIN_BLK * 16) + (r % BIN_BLK) * 16 + (byte & 15);
}

// One thread per (row, byte of the padded row): 8 compares.  qt == 0: out = blocked codes, row row0 + i; qt > 0 (queries): out = the scan's
// query tiles of qt queries, [tile][G][qt][16 bytes].
// Padding bytes (byte >= d / 8) are written as zero, so the scan may run over whole 16-byte groups.
__global__ void __launch_bounds__(256)
k_bin_pack(const float* __restrict__ X, int64_t n_rows, int64_t ldx, int d, float thr, const float* __restrict__ thr_vec, uint8_t* __restrict__ out,
           int64_t row0, int G, int qt) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Mp = 16 * G;
  if (t >= n_rows * Mp) return;
  const int64_t i = t / Mp;
  const int byte = (int)(t - i * Mp);
  uint32_t v = 0;
  if (byte * 8 < d) {
    const float* x = X + i * ldx + byte * 8;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const float th = thr_vec != nullptr ? thr_vec[byte * 8 + b] : thr;
      v |= (x[b] > th ? 1u : 0u) << (7 - b);          // strict; NaN compares false
    }
  }
  out[qt == 0 ? bin_code_off(row0 + i, byte, G) : (((i / qt) * G + (byte >> 4)) * qt + i % qt) * 16 + (byte & 15)] = (uint8_t)v;
}

__global__ void __launch_bounds__(256)
k_bin_store(const uint8_t* __restrict__ B, int64_t n_rows, int64_t ldb, int d, uint8_t* __restrict__ codes, int64_t row0, int G) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Mp = 16 * G;
  if (t >= n_rows * Mp) return;
  const int64_t i = t / Mp;
  const int byte = (int)(t - i * Mp);
  codes[bin_code_off(row0 + i, byte, G)] = byte * 8 < d ? B[i * ldb + byte] : (uint8_t)0;
}

__global__ void __launch_bounds__(256)
k_bin_decode(const uint8_t* __restrict__ codes, int64_t row0, int64_t n_rows, int d, int G, uint8_t* __restrict__ out, int64_t ldo) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nb = d / 8;
  if (t >= n_rows * nb) return;
  const int64_t i = t / nb;
  const int byte = (int)(t - i * nb);
  out[i * ldo + byte] = codes[bin_code_off(row0 + i, byte, G)];
}

// cut[q] = {t_q, need_eq, n_lt, kk}
#define BIN_CUT_W 4

// The scan.  Grid (gx, query tiles): workgroup (x, y) walks the 1024-row tiles x, x + gx, ... for queries QT y .. QT y + QT - 1; lane t holds row
// 1024 tile + t.  The row comes in 16-byte groups (64 lanes: 1 KiB contiguous, the next group prefetched); the query words of a group are the same
// for every lane (kernel-argument pointer, uniform index: scalar loads), so a 32-bit word costs two vector operations per (query, row): the XOR and
// the accumulating population count.  qw holds whole query tiles, group major: [query tile][G][QT][16 bytes], so that the words a tile needs for
// one group are contiguous (queries >= nq of the last tile are scanned and dropped).
template <int QT, int MODE>
__global__ void __launch_bounds__(BIN_TILE)
k_bin_scan(const uint8_t* __restrict__ codes, int64_t n_rows, int G, const uint32_t* __restrict__ qw, int nq, int nbins, unsigned int* __restrict__ hist,
           const int* __restrict__ cut, unsigned int* __restrict__ fill, unsigned int* __restrict__ tiecnt, const unsigned int* __restrict__ tiebase,
           unsigned long long* __restrict__ keys, int64_t ntiles) {
  extern __shared__ __attribute__((aligned(16))) uint32_t bin_hist_s[];   // MODE 0: [QT][HW] words, two 16-bit bins per word
  __shared__ unsigned int wc[QT][BIN_TILE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * QT;
  const int nqt = nq - q0 < QT ? nq - q0 : QT;
  constexpr int QB = QT < 8 ? QT : 8;
  const uint4* qt = (const uint4*)qw + (int64_t)blockIdx.y * G * QT;   // [G][QT] 16-byte pieces of this query tile
  const int HW = (nbins + 1) >> 1;
  if (MODE == 0) {
    for (int e = tid; e < QT * HW; e += BIN_TILE) bin_hist_s[e] = 0;
    __syncthreads();
  }
  int since_flush = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (MODE == 2) {                                   // (uniform) nothing to place here for any query of the tile: skip the scan
      bool any = false;
#pragma unroll
      for (int t = 0; t < QT; ++t)
        if (t < nqt) {
          const int64_t o = (int64_t)(q0 + t) * ntiles + tile;
          any = any || (tiecnt[o] != 0 && tiebase[o] < (unsigned int)cut[(q0 + t) * BIN_CUT_W + 1]);
        }
      if (!any) continue;
    }
    const int64_t r = tile * BIN_TILE + tid;
    const bool valid = r < n_rows;
    const uint8_t* rc = codes + (r / BIN_BLK) * BIN_BLK * 16 * G + (r % BIN_BLK) * 16;
    uint32_t h[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) h[t] = 0;
    uint4 cur = make_uint4(0, 0, 0, 0);
    if (valid) cur = *(const uint4*)rc;                // (rows past n_rows may lie past the allocation: never loaded)
    // the query words go through the scalar registers QB queries at a time; the next batch is requested before the current one is used, so
    // its latency hides under the QB x 8 vector operations of the current batch
    uint4 nxq[QB];
#pragma unroll
    for (int u = 0; u < QB; ++u) nxq[u] = qt[u];
    for (int g = 0; g < G; ++g) {
      uint4 nxt = cur;
      if (valid && g + 1 < G) nxt = *(const uint4*)(rc + (int64_t)(g + 1) * (BIN_BLK * 16));
#pragma unroll
      for (int tb = 0; tb < QT / QB; ++tb) {
        uint4 cq[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) cq[u] = nxq[u];
        const int gn = tb + 1 < QT / QB ? g : (g + 1 < G ? g + 1 : g);         // (the last step loads its own batch again: in bounds, unused)
        const uint4* qn = qt + (int64_t)gn * QT + (tb + 1 < QT / QB ? tb + 1 : 0) * QB;
#pragma unroll
        for (int u = 0; u < QB; ++u) nxq[u] = qn[u];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
          h[tb * QB + u] += __popc(cur.x ^ cq[u].x);
          h[tb * QB + u] += __popc(cur.y ^ cq[u].y);
          h[tb * QB + u] += __popc(cur.z ^ cq[u].z);
          h[tb * QB + u] += __popc(cur.w ^ cq[u].w);
        }
      }
      cur = nxt;
    }
    if (MODE == 0) {
      if (valid) {
#pragma unroll
        for (int t = 0; t < QT; ++t)
          if (t < nqt) atomicAdd(&bin_hist_s[t * HW + (h[t] >> 1)], 1u << ((h[t] & 1u) * 16));
      }
      if (++since_flush == BIN_HIST_FLUSH || tile + gridDim.x >= ntiles) {
        since_flush = 0;
        __syncthreads();
        for (int e = tid; e < QT * HW; e += BIN_TILE) {
          const uint32_t w = bin_hist_s[e];
          if (w != 0) {
            const int t = e / HW, b = (e - t * HW) * 2;
            unsigned int* hq = hist + (int64_t)(q0 + t) * nbins;
            if (w & 0xFFFFu) atomicAdd(hq + b, w & 0xFFFFu);
            if (w >> 16) atomicAdd(hq + b + 1, w >> 16);     // (b + 1 < nbins: a count there means some h == b + 1 <= d)
            bin_hist_s[e] = 0;
          }
        }
        __syncthreads();
      }
    } else {
#pragma unroll
      for (int t = 0; t < QT; ++t)
        if (t < nqt) {
          const int q = q0 + t;
          const uint32_t T = (uint32_t)cut[q * BIN_CUT_W];
          const bool eq = valid && h[t] == T;
          if (MODE == 1 && valid && h[t] < T) {
            const unsigned int slot = atomicAdd(&fill[q], 1u);       // (the order of the slots does not matter: the keys are sorted)
            if (slot < BIN_MAXK) keys[(int64_t)q * BIN_MAXK + slot] = ((unsigned long long)h[t] << 32) | (unsigned long long)r;
          }
          const unsigned long long bal = __ballot(eq);
          if (lane == 0) wc[t][wave] = (unsigned int)__popcll(bal);
          if (MODE == 2) h[t] = eq ? (unsigned int)__popcll(bal & ((1ull << lane) - 1ull)) : 0xFFFFFFFFu;   // rank inside the wave
        }
      __syncthreads();
      if (MODE == 1) {
        if (tid < nqt) {
          unsigned int s = 0;
          for (int w = 0; w < BIN_TILE / 64; ++w) s += wc[tid][w];
          tiecnt[(int64_t)(q0 + tid) * ntiles + tile] = s;
        }
      } else {
#pragma unroll
        for (int t = 0; t < QT; ++t)
          if (t < nqt && h[t] != 0xFFFFFFFFu) {
            const int q = q0 + t;
            unsigned int rank = tiebase[(int64_t)q * ntiles + tile] + h[t];
            for (int w = 0; w < wave; ++w) rank += wc[t][w];
            const unsigned int need = (unsigned int)cut[q * BIN_CUT_W + 1], n_lt = (unsigned int)cut[q * BIN_CUT_W + 2];
            if (rank < need && n_lt + rank < BIN_MAXK)
              keys[(int64_t)q * BIN_MAXK + n_lt + rank] = ((unsigned long long)(uint32_t)cut[q * BIN_CUT_W] << 32) | (unsigned long long)r;
          }
      }
      __syncthreads();
    }
  }
}

// One workgroup per query: every thread sums a contiguous run of bins, thread 0 walks the 256 partial sums to the run in which the cumulative
// count reaches kk and then that run bin by bin.
__global__ void __launch_bounds__(256)
k_bin_cut(const unsigned int* __restrict__ hist, int nbins, int kk, int* __restrict__ cut) {
  __shared__ unsigned long long part[256];
  const int q = blockIdx.x, tid = threadIdx.x;
  const unsigned int* hq = hist + (int64_t)q * nbins;
  const int per = (nbins + 255) / 256;
  unsigned long long s = 0;
  for (int b = tid * per; b < (tid + 1) * per && b < nbins; ++b) s += hq[b];
  part[tid] = s;
  __syncthreads();
  if (tid != 0) return;
  int t = 0;
  unsigned long long below = 0;
  if (kk > 0) {
    int c = 0;
    while (c < 255 && below + part[c] < (unsigned long long)kk) below += part[c++];
    t = c * per;
    while (t < nbins - 1 && below + hq[t] < (unsigned long long)kk) below += hq[t++];
  }
  cut[q * BIN_CUT_W + 0] = t;
  cut[q * BIN_CUT_W + 1] = kk - (int)below;
  cut[q * BIN_CUT_W + 2] = (int)below;
  cut[q * BIN_CUT_W + 3] = kk;
}

__global__ void __launch_bounds__(BIN_TILE)
k_bin_tie_prefix(const unsigned int* __restrict__ cnt, unsigned int* __restrict__ base, int64_t ntiles) {
  __shared__ unsigned int ws[BIN_TILE / 64];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned int carry = 0;
  for (int64_t c0 = 0; c0 < ntiles; c0 += BIN_TILE) {
    const int64_t i = c0 + tid;
    const unsigned int v = i < ntiles ? cnt[(int64_t)q * ntiles + i] : 0u;
    unsigned int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) ws[wave] = x;
    __syncthreads();
    unsigned int woff = 0, tot = 0;
    for (int w = 0; w < BIN_TILE / 64; ++w) {
      const unsigned int s = ws[w];
      if (w < wave) woff += s;
      tot += s;
    }
    if (i < ntiles) base[(int64_t)q * ntiles + i] = carry + woff + x - v;
    carry += tot;
    __syncthreads();
  }
}

__device__ __forceinline__ int64_t bin_map_id(int64_t row, int64_t id_base, const int64_t* __restrict__ row_map) {
  return row_map != nullptr ? row_map[row] : id_base + row;
}

// Hamming output of one query: ascending (h, row) = descending ~key.  Padding keys are 0 (below every ~key of a real entry).
__global__ void __launch_bounds__(SEL_THREADS)
k_bin_sort(const unsigned long long* __restrict__ keys, int kk, int k, int64_t id_base, const int64_t* __restrict__ row_map, int32_t* __restrict__ out_d,
           int64_t* __restrict__ out_i) {
  __shared__ unsigned long long buf[BIN_MAXK];
  const int q = blockIdx.x;
  int P = 2;
  while (P < kk) P <<= 1;
  for (int i = threadIdx.x; i < P; i += blockDim.x) buf[i] = i < kk ? ~keys[(int64_t)q * BIN_MAXK + i] : 0ull;
  bitonic_sort_desc(buf, P);
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const unsigned long long key = ~buf[i < P ? i : 0];
    const bool real = i < kk;
    out_d[(int64_t)q * k + i] = real ? (int32_t)(key >> 32) : 0x7FFFFFFF;
    out_i[(int64_t)q * k + i] = real ? bin_map_id((int64_t)(key & 0xFFFFFFFFull), id_base, row_map) : -1;
  }
}

// Grid (ceil(kk / 16), queries), 256 threads: the query row sits in LDS, wave w scores candidates 16 x + 4 w .. + 3.  Lane l takes the 32-bit
// words l, l + 64, ... of the candidate's row; inside a word it walks the 32 dimensions starting at its own lane number (LDS reads of one
// instruction then fall into 32 different banks).  Every term is +-q[j] as an fp64, the sum is fp64, rounded once.
__global__ void __launch_bounds__(256)
k_bin_rerank_score(const uint8_t* __restrict__ codes, int d, int G, const float* __restrict__ Q, const unsigned long long* __restrict__ keys, int kk,
                   float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) float bin_q_s[];   // [ceil(d / 32) * 32], zero-padded
  const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = (d + 31) / 32;
  for (int e = tid; e < W * 32; e += 256) bin_q_s[e] = e < d ? Q[(int64_t)q * d + e] : 0.f;
  __syncthreads();
  for (int j = 0; j < BIN_RR_CAND / 4; ++j) {
    const int c = blockIdx.x * BIN_RR_CAND + wave * (BIN_RR_CAND / 4) + j;
    if (c >= kk) break;                                                    // (uniform per wave)
    const int64_t r = (int64_t)(keys[(int64_t)q * BIN_MAXK + c] & 0xFFFFFFFFull);
    double acc = 0.0;
    for (int w = lane; w < W; w += 64) {
      const uint32_t bits = *(const uint32_t*)(codes + bin_code_off(r, 4 * w, G));
#pragma unroll 8
      for (int s = 0; s < 32; ++s) {
        const int e = (s + lane) & 31;                                     // dimension 32 w + e: byte e / 8 of the word, bit 7 - e % 8
        const double v = (double)bin_q_s[32 * w + e];
        acc += ((bits >> (8 * (e >> 3) + 7 - (e & 7))) & 1u) ? v : -v;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) scores[(int64_t)q * BIN_MAXK + c] = (float)acc;
  }
}

__global__ void __launch_bounds__(SEL_THREADS)
k_bin_rerank_sort(const unsigned long long* __restrict__ keys, const float* __restrict__ scores, int kk, int k, int64_t id_base,
                  const int64_t* __restrict__ row_map, float* __restrict__ out_d, int64_t* __restrict__ out_i) {
  __shared__ unsigned long long buf[BIN_MAXK];
  const int q = blockIdx.x;
  int P = 2;
  while (P < kk) P <<= 1;
  for (int i = threadIdx.x; i < P; i += blockDim.x)
    buf[i] = i < kk ? sel_pack(f2key(scores[(int64_t)q * BIN_MAXK + i]), (int64_t)(keys[(int64_t)q * BIN_MAXK + i] & 0xFFFFFFFFull)) : 0ull;
  bitonic_sort_desc(buf, P);
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const unsigned long long c = buf[i < P ? i : 0];
    const bool real = i < kk;
    out_d[(int64_t)q * k + i] = real ? key2f((uint32_t)(c >> 32)) : -FLT_MAX;
    out_i[(int64_t)q * k + i] = real ? bin_map_id(sel_row(c), id_base, row_map) : -1;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
struct BinPlan {
  int G, nbins, qt, nqpad;
  int64_t ntiles;
  size_t qw_off, hist_off, fill_off, cut_off, cnt_off, base_off, keys_off, sc_off, total;
};

static int bin_query_tile(int32_t dim, int32_t n_queries) {
  if (n_queries <= 4 || dim > 4096) return 4;
  return dim > 2048 ? 16 : 32;       // the LDS histogram of a tile: QT x (d / 2 + 1) words -- at most 128 KiB + 128 B (32 x 2048 bits; 4 x 16384 =
}                                    // BIN_MAX_BITS: 128 KiB + 16 B), of the 160 KiB a gfx950 workgroup may hold

static BinPlan bin_plan(int64_t n_rows, int32_t dim, int32_t n_queries) {
  BinPlan p;
  const size_t nq = (size_t)(n_queries > 0 ? n_queries : 1);
  p.G = bin_groups(dim);
  p.nbins = dim + 1;
  p.qt = bin_query_tile(dim, n_queries);
  p.nqpad = (int)lrx_cdiv((int64_t)nq, p.qt) * p.qt;
  p.ntiles = lrx_cdiv(n_rows > 0 ? n_rows : 1, BIN_TILE);
  p.qw_off = 0;
  p.hist_off = align256((size_t)p.nqpad * 16 * p.G);
  p.fill_off = p.hist_off + align256(nq * p.nbins * 4);           // (hist and fill are zeroed together)
  p.cut_off = p.fill_off + align256(nq * 4);
  p.cnt_off = p.cut_off + align256(nq * BIN_CUT_W * 4);
  p.base_off = p.cnt_off + align256(nq * (size_t)p.ntiles * 4);
  p.keys_off = p.base_off + align256(nq * (size_t)p.ntiles * 4);
  p.sc_off = p.keys_off + align256(nq * BIN_MAXK * 8);
  p.total = p.sc_off + align256(nq * BIN_MAXK * 4);
  return p;
}

extern "C" size_t lrx_binary_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t binary_k) {
  (void)binary_k;
  if (dim <= 0 || dim % 8 != 0 || dim > BIN_MAX_BITS) return 0;
  return bin_plan(n_rows, dim, n_queries).total;
}

#define LRX_BIN_CHECK_DIM(who, dim) \
  LRX_CHECK_ARG((dim) > 0 && (dim) % 8 == 0 && (dim) <= BIN_MAX_BITS, who ": dim=%d must be a positive multiple of 8, at most %d", (int)(dim), BIN_MAX_BITS)

extern "C" int lrx_binary_pack_rows(const float* x, int64_t n_rows, int64_t ldx, int32_t dim, float threshold, const float* threshold_vec, void* codes,
                                    int64_t row0, void* stream) {
  LRX_BIN_CHECK_DIM("binary_pack_rows", dim);
  LRX_CHECK_ARG(n_rows >= 0 && row0 >= 0 && ldx >= dim, "binary_pack_rows: bad rows (n_rows=%lld, row0=%lld, ldx=%lld)", (long long)n_rows, (long long)row0,
                (long long)ldx);
  if (n_rows == 0) return LRX_OK;
  LRX_CHECK_ARG(x != nullptr && codes != nullptr, "binary_pack_rows: null pointer");
  const int G = bin_groups(dim);
  hipLaunchKernelGGL(k_bin_pack, dim3((unsigned)lrx_cdiv(n_rows * 16 * G, 256)), dim3(256), 0, (hipStream_t)stream, x, n_rows, ldx, dim, threshold,
                     threshold_vec, (uint8_t*)codes, row0, G, 0);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_binary_store_rows(const void* bytes, int64_t n_rows, int64_t ld_bytes, int32_t dim, void* codes, int64_t row0, void* stream) {
  LRX_BIN_CHECK_DIM("binary_store_rows", dim);
  LRX_CHECK_ARG(n_rows >= 0 && row0 >= 0 && ld_bytes >= dim / 8, "binary_store_rows: bad rows (n_rows=%lld, row0=%lld, ld_bytes=%lld)", (long long)n_rows,
                (long long)row0, (long long)ld_bytes);
  if (n_rows == 0) return LRX_OK;
  LRX_CHECK_ARG(bytes != nullptr && codes != nullptr, "binary_store_rows: null pointer");
  const int G = bin_groups(dim);
  hipLaunchKernelGGL(k_bin_store, dim3((unsigned)lrx_cdiv(n_rows * 16 * G, 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)bytes, n_rows, ld_bytes,
                     dim, (uint8_t*)codes, row0, G);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_binary_decode_rows(const void* codes, int64_t row0, int64_t n_rows, int32_t dim, void* out_bytes, int64_t ldo, void* stream) {
  LRX_BIN_CHECK_DIM("binary_decode_rows", dim);
  LRX_CHECK_ARG(row0 >= 0 && n_rows >= 0 && ldo >= dim / 8, "binary_decode_rows: row0=%lld n_rows=%lld ldo=%lld", (long long)row0, (long long)n_rows,
                (long long)ldo);
  if (n_rows == 0) return LRX_OK;
  LRX_CHECK_ARG(codes != nullptr && out_bytes != nullptr, "binary_decode_rows: null pointer");
  hipLaunchKernelGGL(k_bin_decode, dim3((unsigned)lrx_cdiv(n_rows * (dim / 8), 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, row0, n_rows,
                     dim, bin_groups(dim), (uint8_t*)out_bytes, ldo);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

template <int QT, int MODE>
static int bin_scan_launch(const BinPlan& p, const void* codes, int64_t n_rows, int nq, char* ws, hipStream_t s) {
  const int nqt = (int)lrx_cdiv(nq, QT);
  size_t smem = 0;
  int64_t gx = lrx_cdiv(2 * (int64_t)lrx_cu_count(), nqt);
  if (MODE == 0) {                                    // a histogram over 64 KiB leaves room for one workgroup per CU
    smem = (size_t)QT * ((p.nbins + 1) / 2) * 4;
    if (smem > 65536) gx = lrx_cdiv(lrx_cu_count(), nqt);
    LRX_HIP(hipFuncSetAttribute((const void*)k_bin_scan<QT, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  }
  gx = gx > p.ntiles ? p.ntiles : gx;
  hipLaunchKernelGGL((k_bin_scan<QT, MODE>), dim3((unsigned)gx, (unsigned)nqt), dim3(BIN_TILE), smem, s, (const uint8_t*)codes, n_rows, p.G,
                     (const uint32_t*)(ws + p.qw_off), nq, p.nbins, (unsigned int*)(ws + p.hist_off), (const int*)(ws + p.cut_off),
                     (unsigned int*)(ws + p.fill_off), (unsigned int*)(ws + p.cnt_off), (const unsigned int*)(ws + p.base_off),
                     (unsigned long long*)(ws + p.keys_off), p.ntiles);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

template <int MODE>
static int bin_scan(const BinPlan& p, const void* codes, int64_t n_rows, int nq, char* ws, hipStream_t s) {
  switch (p.qt) {
    case 4: return bin_scan_launch<4, MODE>(p, codes, n_rows, nq, ws, s);
    case 16: return bin_scan_launch<16, MODE>(p, codes, n_rows, nq, ws, s);
    default: return bin_scan_launch<32, MODE>(p, codes, n_rows, nq, ws, s);
  }
}

// The Hamming candidates of every query: keys[q][0 .. kk) of the workspace, kk = min(n_cand, n_rows), in no particular order.
static int bin_candidates(const BinPlan& p, const void* codes, int64_t n_rows, int32_t dim, const float* q, int32_t nq, float threshold,
                          const float* threshold_vec, int kk, char* ws, hipStream_t s) {
  hipLaunchKernelGGL(k_bin_pack, dim3((unsigned)lrx_cdiv((int64_t)nq * 16 * p.G, 256)), dim3(256), 0, s, q, (int64_t)nq, (int64_t)dim, dim, threshold,
                     threshold_vec, (uint8_t*)(ws + p.qw_off), (int64_t)0, p.G, p.qt);
  LRX_LAUNCH_CHECK();
  LRX_HIP(hipMemsetAsync(ws + p.hist_off, 0, p.cut_off - p.hist_off, s));
  int rc = LRX_OK;
  if (n_rows > 0 && (rc = bin_scan<0>(p, codes, n_rows, nq, ws, s)) != LRX_OK) return rc;
  hipLaunchKernelGGL(k_bin_cut, dim3((unsigned)nq), dim3(256), 0, s, (const unsigned int*)(ws + p.hist_off), p.nbins, kk, (int*)(ws + p.cut_off));
  LRX_LAUNCH_CHECK();
  if (n_rows == 0) return LRX_OK;
  if ((rc = bin_scan<1>(p, codes, n_rows, nq, ws, s)) != LRX_OK) return rc;
  hipLaunchKernelGGL(k_bin_tie_prefix, dim3((unsigned)nq), dim3(BIN_TILE), 0, s, (const unsigned int*)(ws + p.cnt_off), (unsigned int*)(ws + p.base_off),
                     p.ntiles);
  LRX_LAUNCH_CHECK();
  return bin_scan<2>(p, codes, n_rows, nq, ws, s);
}

static int bin_check_search(const char* who, const void* codes, int64_t n_rows, int32_t dim, const float* q, int32_t n_queries, int32_t k, int32_t binary_k,
                            const void* out_d, const void* out_i, const void* ws, size_t ws_bytes, int32_t flags) {
  LRX_CHECK_ARG(dim > 0 && dim % 8 == 0 && dim <= BIN_MAX_BITS, "%s: dim=%d must be a positive multiple of 8, at most %d", who, dim, BIN_MAX_BITS);
  LRX_CHECK_ARG(k >= 1 && k <= binary_k && binary_k <= BIN_MAXK, "%s: need 1 <= k <= binary_k <= %d (k=%d, binary_k=%d)", who, BIN_MAXK, k, binary_k);
  if (codes_check_rows(who, n_rows) != LRX_OK) return LRX_ERR_INVALID;
  LRX_CHECK_ARG((flags & ~LRX_BINARY_SELECT_ONLY) == 0, "%s: unknown flags 0x%x", who, flags);
  if (n_queries <= 0) return LRX_OK;
  LRX_CHECK_ARG((codes != nullptr || n_rows == 0) && q != nullptr && ((out_d != nullptr && out_i != nullptr) || (flags & LRX_BINARY_SELECT_ONLY)) && ws != nullptr,
                "%s: null pointer", who);
  return codes_check_workspace(who, ws_bytes, bin_plan(n_rows, dim, n_queries).total);
}

extern "C" int lrx_binary_hamming_search(const void* codes, int64_t n_rows, int32_t dim, const float* q, int32_t n_queries, float threshold,
                                         const float* threshold_vec, int32_t k, int64_t id_base, int32_t* out_dist, int64_t* out_ids, const int64_t* row_map,
                                         void* workspace, size_t workspace_bytes, int32_t flags, void* stream) {
  int rc = bin_check_search("binary_hamming_search", codes, n_rows, dim, q, n_queries, k, k, out_dist, out_ids, workspace, workspace_bytes, flags);
  if (rc != LRX_OK || n_queries <= 0) return rc;
  const BinPlan p = bin_plan(n_rows, dim, n_queries);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int kk = (int)(n_rows < k ? n_rows : k);
  if ((rc = bin_candidates(p, codes, n_rows, dim, q, n_queries, threshold, threshold_vec, kk, ws, s)) != LRX_OK) return rc;
  if (flags & LRX_BINARY_SELECT_ONLY) return LRX_OK;
  hipLaunchKernelGGL(k_bin_sort, dim3((unsigned)n_queries), dim3(SEL_THREADS), 0, s, (const unsigned long long*)(ws + p.keys_off), kk, k, id_base, row_map,
                     out_dist, out_ids);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_binary_ip_search(const void* codes, int64_t n_rows, int32_t dim, const float* q, int32_t n_queries, float threshold,
                                    const float* threshold_vec, int32_t k, int32_t binary_k, int64_t id_base, float* out_scores, int64_t* out_ids,
                                    const int64_t* row_map, void* workspace, size_t workspace_bytes, int32_t flags, void* stream) {
  int rc = bin_check_search("binary_ip_search", codes, n_rows, dim, q, n_queries, k, binary_k, out_scores, out_ids, workspace, workspace_bytes, flags);
  if (rc != LRX_OK || n_queries <= 0) return rc;
  const BinPlan p = bin_plan(n_rows, dim, n_queries);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int kk = (int)(n_rows < binary_k ? n_rows : binary_k);
  if ((rc = bin_candidates(p, codes, n_rows, dim, q, n_queries, threshold, threshold_vec, kk, ws, s)) != LRX_OK) return rc;
  if (flags & LRX_BINARY_SELECT_ONLY) return LRX_OK;
  for (int32_t q0 = 0; kk > 0 && q0 < n_queries; q0 += BIN_RR_QMAX) {          // (keys and scores are strided per query: a launch takes its slice)
    const int nq = n_queries - q0 < BIN_RR_QMAX ? n_queries - q0 : BIN_RR_QMAX;
    hipLaunchKernelGGL(k_bin_rerank_score, dim3((unsigned)lrx_cdiv(kk, BIN_RR_CAND), (unsigned)nq), dim3(256), (size_t)((dim + 31) / 32) * 32 * 4, s,
                       (const uint8_t*)codes, dim, p.G, q + (int64_t)q0 * dim, (const unsigned long long*)(ws + p.keys_off) + (int64_t)q0 * BIN_MAXK, kk,
                       (float*)(ws + p.sc_off) + (int64_t)q0 * BIN_MAXK);
    LRX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_bin_rerank_sort, dim3((unsigned)n_queries), dim3(SEL_THREADS), 0, s, (const unsigned long long*)(ws + p.keys_off),
                     (const float*)(ws + p.sc_off), kk, k, id_base, row_map, out_scores, out_ids);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}
