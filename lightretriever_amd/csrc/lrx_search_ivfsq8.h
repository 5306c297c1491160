// liblrx search, part O -- INVERTED FILE over 8-BIT SCALAR-QUANTISED codes (faiss IndexIVFScalarQuantizer, QT_8bit | QT_8bit_uniform, inner
// product): the exact top k under the 8-bit store's score over the rows of the cells a query probes.  k_ivf_sq8_scan, k_ivf_sq8_encode,
// k_ivf_sq8_decode, lrx_ivf_sq8_ip_search, lrx_ivf_sq8_encode_rows, lrx_ivf_sq8_decode_rows (contract: include/lrx.h).
// Part of the ONE translation unit lrx_search.hip (included at its end, after lrx_search_ivfsq.h: it reuses the whole cell-major chain of
// lrx_search_ivf.h -- ivf_cell_major_search: clear, plan, items, scatter, select, the chunking, the workspace and the error counter -- and the
// quantiser of lrx_search_sq8.h: sq8_dec's arithmetic, k_sq8_encode's rule, the qtype numbers).  Not a stand-alone header.
//
// The only kernel of the chain that is this file's is the scan: k_ivf_scan's item walk over codes of 1 byte per element, row-major [n_rows, dim]
// by stored position (NOT the tiled layout of the flat 8-bit index: a cell's rows are consecutive, so a group is one contiguous run of bytes).
// Unlike the fp16 scan, which converts a code once per (query, row) pair, the group is DECODED ONCE per item, to fp32 in LDS, and every pair is
// then scored by exact_dot_lds, the dot of the fp32 scan: k_ivf_scan's per-pair work over a quarter of its HBM bytes.
#pragma once

extern "C" int32_t lrx_ivf_sq8_group_rows(int32_t dim) { return dim >= 1 ? ivf_group_rows(dim) : 0; }   // (the fp32 scan's: the group is staged as fp32)

// sq8_dec from its first rounding on: t = fl32((code + 0.5) / 255) comes from the scan's table
__device__ __forceinline__ float sq8_dec_t(float t, float vmin, float vdiff) {
#pragma clang fp contract(off)
  const float m = t * vdiff;
  return vmin + m;
}

// exact_dot_lds over a row of the scan's SWIZZLED LDS image (k_ivf_sq8_scan: the 16-byte slot s of the 64-byte chunk c lies at slot
// s ^ (c / 2) % 4; `swz` is that xor for this lane's chunks of this row, the same for all of them since a lane's chunks are 8 apart): lane
// sub still multiplies elements 4 sub + 128 u + 0..3 of each 2048-element block, read from where the swizzle put them.
__device__ __forceinline__ float exact_dot_lds_row_base(const float* x_lds, const float* __restrict__ qglob, int D, int lane, int swz, double base) {
  const int sub = lane & 31;
  const int x0 = 4 * ((sub & ~3) | ((sub & 3) ^ swz)) - 4 * sub;   // where this lane's elements lie, relative to their logical place
  return exact_dot_lds<true>([=](int i) { return *(const f32x4*)(x_lds + i + x0); }, qglob, D, lane, base);
}

// The scan: ivf_scan_items (lrx_search_ivf.h) over 8-bit codes.  A group's code rows -- one contiguous run of nrows * D bytes, 16-byte aligned
// since D % 32 == 0, nrows * D <= ROWGRP_LDS_FLOATS -- are loaded with coalesced non-temporal 16-byte loads
// (16 codes per lane) and decoded ONCE into LDS as fp32 (64 KiB): y = vmin_i + t[code] * vdiff_i, t from a 256-entry LDS table of
// fl32((c + 0.5) / 255) (IEEE division, built by the workgroup), vmin / vdiff per dimension from `trained` (two scalars for the uniform type: UNIFORM).
// A lane's 16 floats -- one 64-byte chunk c = i / 16 of the image -- are four 16-byte LDS stores; slot s goes to slot s ^ (c / 2) % 4, so the
// eight lanes that one store cycle serves (banks (a / 4) % 32, 64 B per lane: unswizzled they would hit two slots four times over) hit eight
// distinct 16-byte slots; the half-wave that reads a row undoes it per lane (exact_dot_lds_row_base).  A pair's score is the dot over the
// fp32 rows plus its base term (ivf_probe_base).  SEL: the walk under a row selector (ivf_scan_items).
template <bool UNIFORM, bool SEL>
__global__ void __launch_bounds__(ROWGRP_THREADS, 4)          // (4 waves per SIMD = two workgroups per CU, as k_ivf_scan has: at most 128 VGPRs)
k_ivf_sq8_scan(const uint8_t* __restrict__ C, int64_t N, int D, int G, const float* __restrict__ trained,
               const int64_t* __restrict__ list_off, const int64_t* __restrict__ row_ids, int nlist, const float* __restrict__ q,
               const float* __restrict__ probe_scores, int nprobe, int64_t ld_probe, const unsigned long long* __restrict__ sorted,
               const unsigned int* __restrict__ cell_off, const unsigned int* __restrict__ item_off, unsigned int item_cap,
               const unsigned int* __restrict__ seg_off, int64_t max_scan, unsigned long long* __restrict__ words, const uint32_t* __restrict__ sel) {
  __shared__ __attribute__((aligned(16))) float s_x[ROWGRP_LDS_FLOATS];
  __shared__ float s_t[256];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 256) s_t[tid] = __fdiv_rn((float)tid + 0.5f, 255.f);   // (read after the walk's barrier in front of the first item's staging)
  const int col0 = (tid * 16) % D, col_step = (ROWGRP_THREADS * 16) % D;   // the dimension of a lane's first code, pass by pass (no division per item)
  ivf_scan_items<SEL>(N, G, list_off, row_ids, nlist, nprobe, sorted, cell_off, item_off, item_cap, seg_off, max_scan, words, sel,
    [&](int64_t ra, int nrows) {
      int col = col0;                                        // (D % 32 == 0: a lane's 16 codes are 16 consecutive dimensions of one row)
      const uint8_t* src = C + ra * D;
      for (int i = tid * 16; i < nrows * D; i += ROWGRP_THREADS * 16, col += col_step, col -= col >= D ? D : 0) {
        const sq8_i32x4 cw = __builtin_nontemporal_load((const sq8_i32x4*)(src + i));
        const int swz = (i >> 5) & 3;                        // the chunk's slot xor
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t w = (uint32_t)cw[g];
          f32x4 mn, df;
          if (UNIFORM) {
            mn = f32x4{trained[0], trained[0], trained[0], trained[0]};
            df = f32x4{trained[1], trained[1], trained[1], trained[1]};
          } else {
            mn = *(const f32x4*)(trained + col + 4 * g);
            df = *(const f32x4*)(trained + D + col + 4 * g);
          }
          f32x4 y;
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = sq8_dec_t(s_t[(w >> (8 * e)) & 255u], mn[e], df[e]);
          *(f32x4*)(s_x + i + 4 * (g ^ swz)) = y;
        }
      }
    },
    [&](int rr, unsigned int qi, unsigned int slot) {
      return exact_dot_lds_row_base(s_x + rr * D, q + (int64_t)qi * D, D, lane, (rr * (D >> 5) + ((lane & 31) >> 3)) & 3,
                                    ivf_probe_base(probe_scores, ld_probe, nprobe, qi, slot));
    });
}

// The codes of n rows, one thread per 16-column piece of a row (64 B of fp32 in, ONE 16-byte store out, row-major): v = x - centroid[cell]
// (one fp32 subtraction; cent == NULL: v = x), then k_sq8_encode's rule -- u = (v - vmin) / vdiff (IEEE division; 0 where vdiff == 0, below the
// range and for NaN; clamped to 1), code = (int)(255 u) -- into code row row0 + i.  A cell outside [0, nlist) is never dereferenced: the row's
// codes are zeros and it is counted (once, by the thread of its first piece).
__global__ void __launch_bounds__(256)
k_ivf_sq8_encode(const float* __restrict__ x, int64_t ldx, int64_t n, int D, const float* __restrict__ cent, const int64_t* __restrict__ cells, int nlist,
                 const float* __restrict__ trained, int uniform, uint8_t* __restrict__ codes, int64_t row0) {
#pragma clang fp contract(off)
  const int pieces = D >> 4;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * pieces; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / pieces;
    const int i0 = (int)(t - r * pieces) * 16;
    const int64_t c = cells != nullptr ? cells[r] : 0;
    const bool ok = cells == nullptr || (c >= 0 && c < (int64_t)nlist);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (ok) {
      const float* xr = x + r * ldx + i0;
      const float* cr = cent != nullptr ? cent + c * D + i0 : nullptr;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 xv = *(const f32x4*)(xr + 4 * g);
        const f32x4 cv = cr != nullptr ? *(const f32x4*)(cr + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
        uint32_t word = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = i0 + 4 * g + e;
          const float vmin = trained[uniform ? 0 : i], vdiff = trained[uniform ? 1 : D + i];
          const float v = cr != nullptr ? xv[e] - cv[e] : xv[e];
          float u = vdiff != 0.f ? __fdiv_rn(v - vmin, vdiff) : 0.f;
          if (!(u >= 0.f)) u = 0.f;                          // below the range, and NaN
          if (u > 1.f) u = 1.f;
          word |= (uint32_t)(int)(255.f * u) << (8 * e);
        }
        w[g] = word;
      }
    } else if (i0 == 0) {
      atomicAdd(&g_ivf_bad, 1u);
    }
    *(uint4*)(codes + (row0 + r) * D + i0) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// Code rows [row0, row0 + n) decoded to fp32, one thread per 4 elements: sq8_dec, plus centroid[cells[i]] (one fp32 add) when cent is given.
// A cell outside [0, nlist) is never dereferenced: the decoded row is zeros and it is counted (once).
__global__ void __launch_bounds__(256)
k_ivf_sq8_decode(const uint8_t* __restrict__ codes, int64_t row0, int64_t n, int D, const float* __restrict__ trained, int uniform,
                 const float* __restrict__ cent, const int64_t* __restrict__ cells, int nlist, float* __restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
  const int pieces = D >> 2;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * pieces; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / pieces;
    const int i0 = (int)(t - r * pieces) * 4;
    const int64_t c = cells != nullptr ? cells[r] : 0;
    const bool ok = cells == nullptr || (c >= 0 && c < (int64_t)nlist);
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
      const uint32_t w = *(const uint32_t*)(codes + (row0 + r) * D + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e;
        const float v = sq8_dec((w >> (8 * e)) & 255u, trained[uniform ? 0 : i], trained[uniform ? 1 : D + i]);
        y[e] = cent != nullptr ? v + cent[c * D + i] : v;
      }
    } else if (i0 == 0) {
      atomicAdd(&g_ivf_bad, 1u);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) out[r * ldo + i0 + e] = y[e];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
extern "C" size_t lrx_ivf_sq8_ip_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int32_t k,
                                                 int64_t max_scan_rows) {
  return lrx_ivf_flat_ip_workspace_bytes(n_rows, nlist, dim, n_queries, nprobe, k, max_scan_rows);
}

// lrx_ivf_sq8_ip_search and lrx_ivf_sq8_ip_range_search: the driver over k_ivf_sq8_scan
static int ivf_sq8_run(const char* who, const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                       const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores,
                       int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, const IvfOut& out, const IvfSel& sel, void* workspace,
                       size_t workspace_bytes, void* stream) {
  LRX_CHECK_ARG(sq8_qtype_ok(qtype), "%s: qtype=%d (0: QT_8bit, 2: QT_8bit_uniform)", who, qtype);
  LRX_CHECK_ARG(by_residual == 0 || probe_scores != nullptr, "%s: by_residual=%d needs probe_scores", who, by_residual);
  LRX_CHECK_ARG(trained != nullptr && (uintptr_t)trained % 16 == 0, "%s: trained (vmin ++ vdiff) must be a 16-byte aligned pointer", who);
  const int uniform = qtype == SQ8_QT_8BIT_UNIFORM ? 1 : 0;
  return ivf_cell_major_search(who, codes, (uintptr_t)codes % 16 == 0, "codes must be 16-byte aligned", dim > 0 ? ivf_group_rows(dim) : 1, n_rows, dim,
                               list_off, nlist, q, n_queries, probes, nprobe, ld_probe, max_scan_rows, out, sel, workspace, workspace_bytes, stream,
                               [&](const IvfScanArgs& a) {
    const float* ps = by_residual ? probe_scores + (int64_t)a.q0 * ld_probe : (const float*)nullptr;
    auto* kern = uniform ? (a.sel != nullptr ? k_ivf_sq8_scan<true, true> : k_ivf_sq8_scan<true, false>)
                         : (a.sel != nullptr ? k_ivf_sq8_scan<false, true> : k_ivf_sq8_scan<false, false>);
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(ROWGRP_THREADS), 0, a.stream, (const uint8_t*)codes, n_rows, (int)dim, a.G, trained, list_off, row_ids,
                       (int)nlist, a.q, ps, (int)nprobe, ld_probe, a.sorted, a.cell_off, a.item_off, a.item_cap, a.seg_off, max_scan_rows, a.words, a.sel);
  });
}

extern "C" int lrx_ivf_sq8_ip_search(const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                                     const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                     const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k,
                                     int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return ivf_sq8_run("ivf_sq8_ip_search", codes, n_rows, dim, trained, qtype, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe, ld_probe,
                     by_residual, max_scan_rows, ivf_out_topk(k, id_base, out_scores, out_ids, row_map), IVF_NO_SEL, workspace, workspace_bytes, stream);
}

// The search under a row selector (lrx_search_selector.h): sel_bits == NULL is lrx_ivf_sq8_ip_search.
extern "C" int lrx_ivf_sq8_ip_search_sel(const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                                         const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                         const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k,
                                         int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, const uint32_t* sel_bits,
                                         int64_t sel_rows, void* workspace, size_t workspace_bytes, void* stream) {
  return ivf_sq8_run("ivf_sq8_ip_search_sel", codes, n_rows, dim, trained, qtype, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe,
                     ld_probe, by_residual, max_scan_rows, ivf_out_topk(k, id_base, out_scores, out_ids, row_map), IvfSel{sel_bits, sel_rows}, workspace,
                     workspace_bytes, stream);
}

extern "C" size_t lrx_ivf_sq8_ip_range_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int64_t max_scan_rows) {
  return lrx_ivf_flat_ip_range_workspace_bytes(n_rows, nlist, dim, n_queries, nprobe, max_scan_rows);
}

extern "C" int lrx_ivf_sq8_ip_range_search(const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                                           const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                           const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows,
                                           float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity,
                                           const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream) {
  return ivf_sq8_run("ivf_sq8_ip_range_search", codes, n_rows, dim, trained, qtype, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe,
                     ld_probe, by_residual, max_scan_rows, ivf_out_range(radius, id_base, lims, out_scores, out_ids, capacity, row_map), IVF_NO_SEL, workspace,
                     workspace_bytes, stream);
}

extern "C" int lrx_ivf_sq8_ip_range_search_sel(const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                                               const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                               const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows,
                                               float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity,
                                               const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace, size_t workspace_bytes,
                                               void* stream) {
  return ivf_sq8_run("ivf_sq8_ip_range_search_sel", codes, n_rows, dim, trained, qtype, list_off, row_ids, nlist, q, n_queries, probes, probe_scores, nprobe,
                     ld_probe, by_residual, max_scan_rows, ivf_out_range(radius, id_base, lims, out_scores, out_ids, capacity, row_map),
                     IvfSel{sel_bits, sel_rows}, workspace, workspace_bytes, stream);
}

// the argument checks the encode and decode entries share
#define IVFSQ8_CHECK_ROWS(name, dim, qtype, n, row0, nlist, centroids, cells)                                                                       \
  LRX_CHECK_ARG(dim >= 32 && dim <= 8192 && dim % 32 == 0, name ": dim=%d must be a multiple of 32 in 32..8192", dim);                              \
  LRX_CHECK_ARG(sq8_qtype_ok(qtype), name ": qtype=%d (0: QT_8bit, 2: QT_8bit_uniform)", qtype);                                                    \
  LRX_CHECK_ARG(n >= 0 && row0 >= 0 && row0 + n < (1ll << 32), name ": rows [%lld, %lld + %lld) out of range", (long long)row0, (long long)row0,    \
                (long long)n);                                                                                                                      \
  LRX_CHECK_ARG(nlist >= 1, name ": nlist=%d must be >= 1", nlist);                                                                                 \
  LRX_CHECK_ARG(centroids == nullptr || cells != nullptr, name ": centroids need cells")

extern "C" int lrx_ivf_sq8_encode_rows(const float* x, int64_t ldx, int64_t n, int32_t dim, const float* centroids, const int64_t* cells, int32_t nlist,
                                       const float* trained, int32_t qtype, void* codes, int64_t row0, void* stream) {
  IVFSQ8_CHECK_ROWS("ivf_sq8_encode_rows", dim, qtype, n, row0, nlist, centroids, cells);
  if (n == 0) return LRX_OK;
  LRX_CHECK_ARG(x != nullptr && codes != nullptr && trained != nullptr, "ivf_sq8_encode_rows: null pointer");
  LRX_CHECK_ARG(ldx >= dim && ldx % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)centroids % 16 == 0 && (uintptr_t)codes % 16 == 0,
                "ivf_sq8_encode_rows: x, centroids and codes must be 16-byte aligned (ldx=%lld >= dim=%d, ldx %% 4 == 0)", (long long)ldx, dim);
  const int64_t blocks = lrx_cdiv(n * (dim / 16), 256), cap = 64 * (int64_t)lrx_cu_count();
  hipLaunchKernelGGL(k_ivf_sq8_encode, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, (hipStream_t)stream, x, ldx, n, (int)dim, centroids,
                     cells, (int)nlist, trained, qtype == SQ8_QT_8BIT_UNIFORM ? 1 : 0, (uint8_t*)codes, row0);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}

extern "C" int lrx_ivf_sq8_decode_rows(const void* codes, int64_t row0, int64_t n, int32_t dim, const float* trained, int32_t qtype, const float* centroids,
                                       const int64_t* cells, int32_t nlist, float* out, int64_t ldo, void* stream) {
  IVFSQ8_CHECK_ROWS("ivf_sq8_decode_rows", dim, qtype, n, row0, nlist, centroids, cells);
  LRX_CHECK_ARG(ldo >= dim, "ivf_sq8_decode_rows: ldo=%lld < dim=%d", (long long)ldo, dim);
  if (n == 0) return LRX_OK;
  LRX_CHECK_ARG(codes != nullptr && out != nullptr && trained != nullptr, "ivf_sq8_decode_rows: null pointer");
  LRX_CHECK_ARG((uintptr_t)codes % 4 == 0, "ivf_sq8_decode_rows: codes must be 4-byte aligned");
  const int64_t blocks = lrx_cdiv(n * (dim / 4), 256), cap = 64 * (int64_t)lrx_cu_count();
  hipLaunchKernelGGL(k_ivf_sq8_decode, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, row0, n,
                     (int)dim, trained, qtype == SQ8_QT_8BIT_UNIFORM ? 1 : 0, centroids, cells, (int)nlist, out, ldo);
  LRX_LAUNCH_CHECK();
  return LRX_OK;
}
