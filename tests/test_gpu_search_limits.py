"""GPU: the search kernels beyond their INTERNAL limits -- sizes at which the code changes shape (a pass count, a flush, a row that no longer
fits LDS, a grid extent) and that no other test reaches.  Each case is the smallest shape that crosses its limit; every comparison is bit
for bit (ids, and score bits through .view(int32)) against the existing yardsticks or an analytic / integer-exact expectation.

The census.  Every size constant of lightretriever_amd/csrc/lrx_search*.h and lrx_search.hip -- chunk, capacity, pass and flush constants, and
the tile geometry next to them -- with its value and the test that takes a shape across it (a short name without a file is a test of this
file; "=" marks a limit that is an argument bound: the test sits ON it and the first value beyond is refused).  A constant nothing crosses
has the reason in its line.  The lines about this file's tests were run; the lines about other files come from reading those tests'
parameters and docstrings, not from coverage data.  test_census_names_every_size_constant_with_its_value keeps the table in step with
the sources.

  binary (lrx_search_binary.h)
    BIN_BLK              128  test_gpu_binary_index.py::test_pack_equals_np_packbits (adds that start inside a block), every n % 128 != 0 there
    BIN_TILE            1024  test_gpu_binary_index.py::test_hamming_topk_and_rerank_equal_the_yardstick (thousands of tiles, ragged last tile)
    BIN_MAXK            2048  = test_gpu_binary_index.py::test_hamming_topk_and_rerank_equal_the_yardstick[300000-1544] (binary_k = 2048; 2049 refused)
    BIN_MAX_BITS       16384  = test_binary_widest_row_16384_bits, test_binary_widest_row_pack_and_decode_round_trip: SERVED (131 088 B histogram)
    BIN_HIST_FLUSH        63  test_binary_flush_is_taken_at_the_4_query_tile, test_binary_bin_that_would_wrap_without_the_flush (66 / 65 tiles per workgroup),
                              test_binary_bin_of_exactly_65536_rows_per_workgroup (64 tiles: the case a scan WITHOUT the flush fails)
    BIN_RR_CAND           16  test_gpu_binary_index.py::test_hamming_topk_and_rerank_equal_the_yardstick (binary_k = 300, 1000: many workgroups, a ragged last one)
    BIN_RR_QMAX        65535  test_binary_more_queries_than_grid_y
    BIN_CUT_W              4  (a record width, not a limit)
    -- dark: k_bin_scan's own grid.y is the number of QUERY TILES; it passes 65 535 only beyond 262 140 queries (4-query tile, d > 4096:
       4 GiB of query rows and as much histogram) or 2 097 120 (32-query tile): not cheap, not crossed.
  impact (lrx_search_impact.h)
    IMP_MAX_W          32768  = test_gpu_impact_index.py::test_window_edges[32768] (rows in three windows; larger windows refused)
    IMP_TCHUNK           256  test_impact_queries_of_more_than_256_terms, test_impact_range_search_with_more_than_256_terms (256, 257, 512, 513, 700 terms)
    IMP_ROW_CHUNK    4194304  test_gpu_impact_index.py::test_row_chunks_are_merged (4 Mi + 77 rows)
    IMP_MATRIX_BYTES 1073741824  test_impact_query_chunks_under_the_matrix_budget (1100 queries x 270 000 rows)
    IMP_QC_MAX         65535  test_impact_more_queries_than_grid_y
  product quantiser (lrx_search_pq.h, lrx_search_ivfpq.h)
    PQ_KSUB              256  (the code alphabet of 8-bit codes, not a limit)
    PQ_BLK               128  test_gpu_pq_index.py::test_two_pass_scan_with_a_padded_last_group_is_bit_identical_to_the_yardstick (n = 1029)
    PQ_GRP                16  the same test (M % 16 != 0: a padded last group)
    PQ_SCAN_THREADS     1024  the same test (more than one tile, ragged)
    PQ_SCAN_MC           128  the same test (M = 200: two passes over the tables), test_gpu_workspace_discipline.py "pq d=400 M=200"
    PQ_ENC_ROWS          256  test_gpu_pq_index.py::test_add_encodes_like_the_yardstick_and_reconstructs
    PQ_ENC_MAX_DSUB       64  = test_gpu_pq_index.py::test_codes_at_the_smallest_and_largest_sub_space_widths, ::test_sub_space_width_65_is_refused_by_the_library
    PQ_ROW_CHUNK     4194304  test_gpu_pq_index.py::test_row_chunks_are_merged
    PQ_MATRIX_BYTES 1073741824  test_gpu_pq_index.py::test_id_base_row_map_query_chunks_and_the_torch_op (894 queries per chunk)
    PQ_QC_MAX          65535  test_pq_more_queries_than_grid_y
    IVFPQ_TILE          1024  test_gpu_ivfpq_index.py (segments longer than a tile), test_gpu_ivf_plan_scale.py
  flat / fp16-SQ search (lrx_search.hip, lrx_search_filter.h, lrx_search_select.h, lrx_search_bounded.h, lrx_search_refine.h, lrx_search_range.h)
    ROWS_F32               0  (a row-source tag, not a limit)
    ROWS_F16T              1  (a row-source tag, not a limit)
    SPLIT_MIN_QT           3  test_gpu_search.py::test_two_pass_equals_six_product_path_and_oracle (Q = 5 and Q >= 33), test_flat_search_over_long_rows_is_the_integer_matmul
    XPF_S                  4  test_gpu_search_emit.py::test_score_free_filter_equals_score_matrix_filter_bitwise (D = 192, 256, 512: three slices, the ring depth, more)
    SAMPLE_SS_MAX         32  test_gpu_search_emit.py::test_baseline_index_shapes_properties (1M rows and more: the stride rule reaches its cap)
    ANY_FLAG_GROUPS        2  test_gpu_range_search.py::test_overflow_in_the_second_query_group_of_a_chunk (LRX_EMIT_MAX_QUERIES / 128)
    MERGE_MAX          16384  = test_gpu_search.py::test_merge_at_the_widest_supported_exchange (8 x 2048; 9 x 2048 refused)
    S_ROWS               256  test_gpu_search.py::test_random_vs_oracle (257 rows ... 70 000 rows)
    S_BK                  32  the same test (D = 32, 64, 96: one, two, three slices)
    S_XTILE            32768  (S_ROWS x S_BK x 4 bytes: derived)
    SP_ROWS              128  test_gpu_search.py::test_two_pass_equals_six_product_path_and_oracle (row counts that are no multiple of 128)
    SPF_RT                 2  test_gpu_search_emit.py::test_score_free_filter_equals_score_matrix_filter_bitwise (tile geometry of the split filter)
    SPF_NST                2  the same test
    SPF_WV                 8  the same test
    SEL_THREADS         1024  test_gpu_select_paths.py (rows shorter and longer than one pass of the workgroup)
    SEL_MAXK            2048  = test_gpu_select_paths.py (k = 2048), test_gpu_search.py::test_two_pass_equals_six_product_path_and_oracle[6000-64-5-2048]
    SEL_CAND            4096  test_gpu_select_paths.py::test_pq_case_with_id_base_and_row_map, ::test_flat_band_case (band rows beyond the list: the streaming form)
    SEL_EQCAP           2048  test_gpu_select_paths.py (more ties at the cut than the tie list holds)
    REF_CAND            4096  test_gpu_search.py::test_two_pass_band_overflow_falls_back_per_query, test_gpu_search_stages.py::test_stages_against_the_fp64_model
    REF_BLK             8192  test_gpu_search.py::test_two_pass_band_overflow_falls_back_per_query (20 000 near-copies: more qualifying blocks than a part lists)
    REF_SPLIT              4  (workgroups per query, fixed)
    REF_PCAND           1024  (REF_CAND / REF_SPLIT: derived, crossed with REF_CAND)
    REF_PBLK            2048  (REF_BLK / REF_SPLIT: derived, crossed with REF_BLK)
    REF_QLDS            8192  test_flat_search_over_long_rows_is_the_integer_matmul, test_sq_fp16_search_over_long_rows_is_the_integer_matmul,
                              test_range_search_over_long_rows_is_the_integer_matmul, test_rerank_over_long_rows_is_the_integer_matmul,
                              test_gaussian_long_rows_search_range_and_rerank (D = 8224, 12 288): SERVED by all six entries
    ROWGRP_LDS_FLOATS  16384  test_gpu_search_refine_rows.py::test_row_grouped_rescoring_equals_the_per_query_gather_bitwise (D = 256, 2048, 4096: groups of
                              32, 8 and 4 rows); four rows wider than 4096 floats do not fit, row_group_layout then keeps the per-query gather (REF_QLDS's cases)
    ROWGRP_THREADS       512  the same test
    RANGE_CAP          65536  test_gpu_range_codes.py::test_sq_list_overflow_falls_back_to_the_matrix_and_counts (70 000 hits)
    RERANK_MAX_CAND     2048  = test_gpu_refine_index.py::test_integer_probe_is_exact_over_fp32_rows[shape4] (2048 candidates; 2049 refused in test_refusals_and_graph_capture)
    RERANK_MAX_SPLIT      16  test_gpu_refine_index.py::test_integer_probe_is_exact_over_fp32_rows (1, 3 and 5 queries: 16 parts; 130 queries: 1 part)
  code-index driver (lrx_search_codes.h), 8-bit SQ (lrx_search_sq8.h)
    SR_THREADS           256  test_gpu_range_codes.py::test_pq_default_chunk (tiles of 256 rows, ragged)
    SR_SEG              4096  test_gpu_range_codes.py::test_pq_default_chunk, ::test_impact_every_hit (5000 / 3000 rows: two segments / one ragged)
    SQ8_BLK              128  test_gpu_sq8_index.py::test_search_is_exact_over_the_decoded_rows
    SQ8_QT_MAX             8  test_gpu_sq8_index.py::test_torch_op_and_ctypes_agree_with_the_class (1000 queries: chunks of 128)
    SQ8_QCHUNK           128  the same test
    SQ8_ROW_CHUNK    4194304  dark: 4 Mi + rows of 8-bit codes AND their training are not cheap; the chunk loop is scan_search's, crossed by PQ and impact
    SQ8_MATRIX_BYTES 1073741824  dark: binds only beyond 2 M rows (128 queries x rows x 4 B); the rule is scan_plan's, crossed by PQ and impact
    SQ8_NMAX           16319  test_gpu_sq8_stages.py::test_stages_against_the_fp64_model (digit planes at their extremes)
    SQ8_QT_8BIT            0  (faiss's quantiser type, not a limit)
    SQ8_QT_8BIT_UNIFORM    2  (faiss's quantiser type, not a limit)
    -- dark: lrx_sq8_train_minmax walks its rows 33.5 M at a time (grid.y <= 65 535 x 1024 rows): a 33.5 M-row training set is not cheap.
  inverted files (lrx_search_ivf.h, lrx_search_ivfsq.h)
    IVF_MAX_NPROBE      2048  = test_gpu_ivf_plan_scale.py::test_the_nprobe_ladder
    IVF_PLAN_THREADS     256  test_gpu_ivf_plan_scale.py::test_the_nprobe_ladder, ::test_the_item_scan_around_1024_cells
    IVF_MAX_GROUP_ROWS   128  test_gpu_ivf_index.py::test_hand_made_cells_against_the_yardstick_and_the_rerank (cells around the row group)
    IVF_WORDS_BYTES 805306368  test_gpu_ivf_plan_scale.py::test_one_row_over_the_scan_bound_at_1500_probes (the chunk rule under the words budget)
    IVF_MAX_CHUNK       1024  test_gpu_ivf_plan_scale.py::test_more_pairs_than_the_scatter_grid_has_threads
    IVF_SEL_SORT        2048  test_gpu_ivf_plan_scale.py::test_the_nprobe_ladder (segments shorter and longer than one sort)
    IVFSQ_LDS_HALVES   32768  test_gpu_ivfsq_index.py::test_hand_made_cells_against_the_yardstick (cells around the row group of the scan)
  graph (lrx_search_graph.h)
    GRAPH_THREADS        512  (workgroup size, fixed)
    GRAPH_MAX_BEAM      2048  = test_gpu_graph_index.py::test_search_where_one_step_brings_more_rows_than_the_beam_holds
    GRAPH_MAX_CAND      1024  test_gpu_graph_index.py::test_entry_list_longer_than_one_slice
    GRAPH_QLDS          4096  test_gpu_graph_index.py::test_query_rows_too_long_for_lds (D = 8192, the entry's maximum)
    GRAPH_HASH          4096  test_gpu_graph_index.py::test_search_after_the_visited_table_forgot
    GRAPH_HASH_FILL     3072  the same test
    GRAPH_ITEMS            6  ((GRAPH_MAX_BEAM + GRAPH_MAX_CAND) / GRAPH_THREADS: derived)
    GRAPH_MAX_K          256  = test_gpu_graph_index.py::test_detour_kernel_equals_the_yardstick
    DETOUR_SLOTS        1024  the same test (K = 256: the table a quarter full)
"""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binary_yardstick as BY  # noqa: E402
import impact_yardstick as IY  # noqa: E402
import range_codes_yardstick as RY  # noqa: E402
import refine_yardstick as FY  # noqa: E402
import ws_guard  # noqa: E402

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lightretriever_amd", "csrc")
FLT_MAX = float(np.finfo(np.float32).max)


@functools.lru_cache(maxsize=None)
def define(header, name):
    """The integer value of `#define name value` in a csrc file: the tests size their cases from the library's own constants."""
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"^#define\s+%s\s+\(?(\d+)(?:ll\s*<<\s*(\d+)\))?" % name, f.read(), re.M)
    assert m, (header, name)
    return int(m.group(1)) << int(m.group(2) or 0)


@pytest.fixture(scope="module", autouse=True)
def release_shared_cases():
    """The shared corpora and indexes (computed once, left unchanged) go when the module is done."""
    yield
    for f in (impact_case, integer_rows, flat_index, sq_index, gauss_rows):
        f.cache_clear()
    torch.cuda.empty_cache()


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cdiv(a, b):
    return -(-a // b)


def same_bits(got, want):
    (Dg, Ig), (Dw, Iw) = got, want
    Dw, Iw = (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t for t in (Dw, Iw))
    assert torch.equal(Ig.cpu(), Iw.cpu())
    assert Dg.dtype == Dw.dtype and torch.equal(Dg.cpu().view(torch.int32), Dw.cpu().view(torch.int32))


def same_range(got, want):
    want = tuple(torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t for t in want)
    assert torch.equal(got[0].cpu(), want[0].cpu()), (got[0][:8].tolist(), want[0][:8].tolist())
    assert torch.equal(got[2].cpu(), want[2].cpu())
    assert got[1].dtype == want[1].dtype == torch.float32 and torch.equal(got[1].cpu().view(torch.int32), want[1].cpu().view(torch.int32))


# =====================================================================================================================================
# A. binary scan: the mid-scan flush of the 16-bit LDS histogram, and the widest row
# =====================================================================================================================================
def bin_geometry(d, Q):
    """(query tile, workgroups along the rows before the clamp to the tile count) of k_bin_scan<QT, 0>: bin_query_tile and bin_scan_launch
    (lrx_search_binary.h) restated."""
    qt = 4 if (Q <= 4 or d > 4096) else (16 if d > 2048 else 32)
    lds = qt * ((d + 2) // 2) * 4
    return qt, cdiv(cu_count() if lds > 65536 else 2 * cu_count(), cdiv(Q, qt))


def bin_tiles_per_workgroup(n, d, Q):
    ntiles = cdiv(n, define("lrx_search_binary.h", "BIN_TILE"))
    return cdiv(ntiles, min(bin_geometry(d, Q)[1], ntiles))


def test_binary_flush_is_taken_at_the_4_query_tile():
    """d = 8192, Q = 1024: 256 query tiles of 4, a histogram of 65 552 B, one workgroup per CU -> every workgroup walks 65 or 66 tiles and
    flushes its LDS histogram once in mid-scan (after 63) and once at the end."""
    import test_gpu_binary_index as TB
    flush = define("lrx_search_binary.h", "BIN_HIST_FLUSH")
    d, Q = 8192, 1024
    qt, gx = bin_geometry(d, Q)
    assert qt == 4 and gx == cdiv(cu_count(), 256)
    n = (flush + 2) * gx * 1024 + 37
    assert bin_tiles_per_workgroup(n, d, Q) > flush
    xb = TB.random_packed(n, d, seed=21)
    idx = TB.build(xb, d)
    q = TB.grid_q(Q, d, seed=22)
    Dh, Ih = idx.search(q, 100, rerank=False)
    Dr, Ir = idx.search(q, 50, binary_k=300)
    for s in range(0, Q, 128):
        H = TB.hamming_t(TB.pack_t(q[s:s + 128]), xb)
        TB.assert_same((Dh[s:s + 128], Ih[s:s + 128]), TB.hamming_topk_t(H, 100))
        _, C = TB.hamming_topk_t(H, 300)
        TB.assert_same((Dr[s:s + 128], Ir[s:s + 128]), TB.rerank_t(q[s:s + 128], xb, C, 50))


def test_binary_bin_that_would_wrap_without_the_flush():
    """d = 64, Q = 1024 (32 query tiles of 32, 16 workgroups along the rows at 256 CUs), n = 65 x gx x 1024 rows that ALL carry one code, but
    for 20 planted rows: every row of a workgroup's 65 tiles lands in the same bin of a query, 64 512 between two flushes -- 66 560 without
    the flush, which carries into the neighbouring 16-bit half.  The expectation is analytic: per query the planted rows and the first rows
    at the common distance, by (distance, row)."""
    import test_gpu_binary_index as TB
    flush = define("lrx_search_binary.h", "BIN_HIST_FLUSH")
    d, Q = 64, 1024
    qt, gx = bin_geometry(d, Q)
    assert qt == 32 and gx == cdiv(2 * cu_count(), 32)
    n = (flush + 2) * gx * 1024
    assert bin_tiles_per_workgroup(n, d, Q) > flush and (flush + 2) * 1024 > 65535 >= flush * 1024
    rng = np.random.default_rng(31)
    c0 = rng.integers(0, 2, d).astype(np.uint8)                          # the common row, as bits
    b0 = c0.copy()
    b0[rng.choice(d, 10, replace=False)] ^= 1                            # query 0: 10 bits from the common row
    fixed = [3, 700, 1023, 1024, flush * gx * 1024 - 1, (flush - 1) * gx * 1024 + 5, flush * gx * 1024, flush * gx * 1024 + 1023, n - 1024, n - 1]
    rows = np.array(sorted(fixed + [r for r in rng.choice(n, 40, replace=False).tolist() if r not in fixed][:10]))
    assert np.unique(rows).size == 20
    planted = np.tile(b0, (20, 1))
    for i in range(20):
        planted[i, rng.choice(d, i % 10, replace=False)] ^= 1           # i % 10 bits from query 0: strictly closer than the common row
    qbits = rng.integers(0, 2, (Q, d)).astype(np.uint8)
    qbits[0] = b0
    q = torch.from_numpy(qbits.astype(np.float32) * 2 - 1).cuda()
    xb = torch.from_numpy(np.packbits(c0)).cuda().repeat(n, 1)
    xb[torch.from_numpy(rows).cuda()] = torch.from_numpy(np.packbits(planted, axis=1)).cuda()
    idx = TB.build(xb, d)
    assert torch.equal(idx.reconstruct_n(int(rows[4]) - 1, 3), xb[int(rows[4]) - 1:int(rows[4]) + 2])
    # distances on the host, from the packed bytes: column 0 the common row, columns 1 .. 20 the planted rows
    Hs = BY.hamming(BY.pack(q.cpu().numpy()), np.vstack([np.packbits(c0)[None, :], np.packbits(planted, axis=1)])).astype(np.int64)
    assert Hs[0, 0] == 10 and (Hs[0, 1:] < 10).all()
    for k in (1, 100, 2048):
        common = np.setdiff1d(np.arange(k + 20), rows)[:k]              # the first k rows that are not planted
        key = np.concatenate([(Hs[:, 1:] << 32) | rows[None, :], (Hs[:, :1] << 32) | common[None, :]], axis=1)
        key = np.sort(key, axis=1)[:, :k]
        want = ((key >> 32).astype(np.int32), key & 0xFFFFFFFF)
        if k >= 20:
            assert want[1][0, :20].tolist() == rows[np.lexsort((rows, Hs[0, 1:]))].tolist()
        same_bits(idx.search(q, k, rerank=False), want)


def test_binary_bin_of_exactly_65536_rows_per_workgroup():
    """The same tile and grid, n = 64 x gx x 1024 rows of ONE code and nothing planted: a workgroup puts exactly 65 536 rows into one bin of
    every query.  A 16-bit half that is not flushed after 63 tiles then reads 0 (the carry goes to the neighbouring bin or is lost): the bin
    vanishes from the histogram and every cutoff moves.  (With 65 tiles, above, the wrapped half still reads 1024 per workgroup -- more than
    any k -- so a scan that never flushed would pass there: a library built with BIN_HIST_FLUSH = 66 does, and fails here.)  The expectation
    is rows 0 .. k - 1 at the common distance."""
    import test_gpu_binary_index as TB
    flush = define("lrx_search_binary.h", "BIN_HIST_FLUSH")
    d, Q = 64, 1024
    qt, gx = bin_geometry(d, Q)
    n = (flush + 1) * gx * 1024
    assert bin_tiles_per_workgroup(n, d, Q) == flush + 1 and (flush + 1) * 1024 == 65536
    rng = np.random.default_rng(33)
    c0 = rng.integers(0, 2, d).astype(np.uint8)
    qbits = rng.integers(0, 2, (Q, d)).astype(np.uint8)
    qbits[0], qbits[1] = c0, 1 - c0                                      # distances 0 and d: the first and the last bin
    q = torch.from_numpy(qbits.astype(np.float32) * 2 - 1).cuda()
    idx = TB.build(torch.from_numpy(np.packbits(c0)).cuda().repeat(n, 1), d)
    h = BY.hamming(BY.pack(q.cpu().numpy()), np.packbits(c0)[None, :])[:, 0]
    assert h[0] == 0 and h[1] == d and (h % 2 == 0).any() and (h % 2 == 1).any()      # both halves of a histogram word
    for k in (1, 100, 2048):
        same_bits(idx.search(q, k, rerank=False), (np.repeat(h[:, None], k, axis=1).astype(np.int32), np.tile(np.arange(k, dtype=np.int64), (Q, 1))))


@pytest.mark.parametrize("Q", [5, 1])
def test_binary_widest_row_16384_bits(Q):
    """BIN_MAX_BITS: the 4-query tile's histogram is 4 x 8193 words = 131 088 B of LDS, the rerank's query row 64 KiB."""
    import test_gpu_binary_index as TB
    d = define("lrx_search_binary.h", "BIN_MAX_BITS")
    assert d == 16384
    n, k, binary_k = 3000, 10, 100
    xb = TB.random_packed(n, d, seed=41)
    idx = TB.build(xb, d)
    q = TB.grid_q(Q, d, seed=42)
    H = TB.hamming_t(TB.pack_t(q), xb)
    TB.assert_same(idx.search(q, binary_k, rerank=False), TB.hamming_topk_t(H, binary_k))
    TB.assert_same(idx.search(q, k, rerank=False), TB.hamming_topk_t(H, k))
    _, C = TB.hamming_topk_t(H, binary_k)
    TB.assert_same(idx.search(q, k, binary_k=binary_k), TB.rerank_t(q, xb, C, k))


def test_binary_widest_row_pack_and_decode_round_trip():
    import test_gpu_binary_index as TB
    from lightretriever_amd import BinaryFlatIndex
    d, n = 16384, 300
    x = TB.special_rows(n, d, 0.25, seed=43)
    with np.errstate(invalid="ignore"):
        want = np.packbits(x > 0.25, axis=1)
    assert want.shape == (n, d // 8) and np.array_equal(want, BY.pack(x, 0.25))
    idx = BinaryFlatIndex(d, threshold=0.25)
    idx.add(x[:130])
    idx.add(torch.from_numpy(x[130:]).cuda())                            # a start that is not a block boundary
    assert np.array_equal(idx.codes().cpu().numpy(), want)
    idx2 = BinaryFlatIndex(d)
    idx2.add(want)
    assert np.array_equal(idx2.reconstruct_n(120, 20).cpu().numpy(), want[120:140]) and np.array_equal(idx2.codes().cpu().numpy(), want)
    with pytest.raises(NotImplementedError, match="16384"):
        BinaryFlatIndex(d + 8)


# =====================================================================================================================================
# B. impact scan: queries of more than IMP_TCHUNK = 256 terms (2 and 3 passes over the term ranges in LDS)
# =====================================================================================================================================
VOCAB, OOD = 2000, (5000, 2000, 777_777)      # terms no document holds (2000 = the dictionary's size: the first id outside)


@functools.lru_cache(maxsize=None)
def impact_case():
    """3000 rows x 12 postings over a 2000-term vocabulary (term 0 in every row, every other term in some row) and the queries: 256, 257
    terms, an empty one, 512 terms, a 1-term one, 513 and 700 terms, and a 700-term query with one term at positions 255, 256 and 257 (a
    repeat across the pass boundary, also after the index's own query check has dropped the unknown term in front), an unknown term in
    each of the three passes and term 0 in the second pass only.  -> (docs, queries, yardstick, its integer scores [Q, n])."""
    chunk = define("lrx_search_impact.h", "IMP_TCHUNK")
    assert chunk == 256
    rng = np.random.default_rng(51)
    docs = [(np.concatenate([[0], 1 + rng.choice(VOCAB - 1, 11, replace=False)]), rng.integers(1, 300, 12)) for _ in range(3000)]
    assert np.unique(np.concatenate([t for t, _ in docs])).size == VOCAB
    queries = []
    for nt in (chunk, chunk + 1, 0, 2 * chunk, 1, 2 * chunk + 1, 700):
        queries.append((rng.choice(VOCAB, nt, replace=False), rng.integers(1, 4, nt)))
    t = 1 + rng.choice(VOCAB - 1, 700, replace=False)                    # (term 0 is not among them)
    t[chunk - 1] = t[chunk] = t[chunk + 1] = t[10]
    t[100], t[300], t[600] = OOD
    t[400] = 0
    assert np.flatnonzero(t == 0).tolist() == [400] and (t[[99, 101]] < VOCAB).all()
    queries.append((t, rng.integers(1, 4, 700)))
    yard = IY.Yardstick(*IY.csr_of(docs))
    S = RY.impact_scores(yard, queries)
    assert (S[7] >= 1).all() and not (S[2] >= 1).any()
    return docs, queries, yard, S


def impact_index(window_rows):
    from lightretriever_amd import ImpactIndex
    idx = ImpactIndex()
    idx.window_rows = window_rows
    idx.add(*IY.csr_of(impact_case()[0]))
    return idx


def raw_csr(queries):
    """The queries as they are -- unknown terms included -- as the int32 device arrays the torch ops take."""
    from lightretriever_amd.impact_index import query_csr
    return tuple(torch.from_numpy(a.astype(np.int32)).cuda() for a in query_csr(queries))


@pytest.mark.parametrize("window_rows", [128, 0, 32768])
def test_impact_queries_of_more_than_256_terms(window_rows):
    """Workgroups with 0, 1, 2 and 3 passes side by side, at 128-row windows (24 windows, 256 threads), the library's rule (2048 rows) and the
    one 32768-row window (1024 threads: the term rotation (tid + 64 j) & 1023 with j up to 255).  Through ImpactIndex.search (which drops
    the unknown terms on the host) and through the torch op (which hands the kernel the query as it is)."""
    from lightretriever_amd import torch_ops  # noqa: F401
    from lightretriever_amd.impact_index import query_csr
    docs, queries, yard, S = impact_case()
    idx = impact_index(window_rows)
    off, term, cnt = idx.check_queries(*query_csr(queries))
    assert np.diff(off).tolist() == [256, 257, 0, 512, 1, 513, 700, 697]
    assert term[off[7] + 255] == term[off[7] + 256] == queries[7][0][10]          # the repeat still straddles the boundary after the drop
    for k in (10, 2048):
        want = yard.search(queries, k)
        same_bits(idx.search(*query_csr(queries), k), want)
        same_bits(torch.ops.lrx.impact_topk(idx._postings, idx._term_off, idx.ntotal, *raw_csr(queries), k, 0, None, window_rows), want)


@pytest.mark.parametrize("window_rows", [128, 0])
def test_impact_range_search_with_more_than_256_terms(window_rows):
    from lightretriever_amd import torch_ops  # noqa: F401
    from lightretriever_amd.impact_index import query_csr
    docs, queries, yard, S = impact_case()
    idx = impact_index(window_rows)
    mid = float(np.quantile(S[S >= 1].astype(np.float32), 0.9, method="lower"))   # a score some row holds: strictly greater excludes it
    for radius in (-1.0, mid):
        want = RY.range_impact(S, radius)
        assert 0 < int(want[0][-1]) and (radius < 0 or int(want[0][-1]) < int((S >= 1).sum()))
        same_range(idx.range_search(*query_csr(queries), radius), want)
    same_range(torch.ops.lrx.impact_range_search(idx._postings, idx._term_off, idx.ntotal, *raw_csr(queries), mid, 0, window_rows, 0), RY.range_impact(S, mid))


# =====================================================================================================================================
# C. rows longer than REF_QLDS = 8192 floats: the refine / rerank kernels read the query row from global memory, exact_dot walks more
#    than four 2048-element blocks
# =====================================================================================================================================
LONG_DIMS = [8224, 12288]                     # 8192 + 32 (no fp16 shadow: not a multiple of 64), and a multiple of 64


@functools.lru_cache(maxsize=None)
def integer_rows(dim):
    """6000 rows and 40 queries of integers in [-8, 8] on the device, and their exact scores [40, 6000] as int64 (an fp64 matmul: every
    product and partial sum is an integer below 2^20, exact in fp32 and fp64 in any order)."""
    assert dim > define("lrx_search_bounded.h", "REF_QLDS") == 8192
    g = torch.Generator(device="cuda").manual_seed(dim)
    X = torch.randint(-8, 9, (6000, dim), generator=g, device="cuda").float()
    q = torch.randint(-8, 9, (40, dim), generator=g, device="cuda").float()
    X[4001] = X[17]                                                      # twins: equal scores for every query
    S = (q.double() @ X.double().T)
    assert float(S.abs().max()) < 2 ** 20 and torch.equal(S, S.round())
    return X, q, S.long()


def integer_topk(S, k, id_base=0):
    """S int64 [Q, n] -> (D fp32, I): score descending, ties to the lower row."""
    n = S.shape[1]
    key = torch.topk(-S * (1 << 32) + torch.arange(n, device=S.device)[None, :], k, dim=1, largest=False, sorted=True).values
    rows = key & 0xFFFFFFFF
    return torch.gather(S, 1, rows).float(), rows + id_base


@functools.lru_cache(maxsize=None)
def flat_index(dim, n, shadow=True):
    from lightretriever_amd import FlatIPIndex
    idx = FlatIPIndex(dim, capacity=n, id_base=100)
    idx.shadow_f16 = shadow
    idx.add(integer_rows(dim)[0][:n])
    assert (idx._xb is not None) == (shadow and dim % 64 == 0)
    return idx


@functools.lru_cache(maxsize=None)
def sq_index(dim, kind="int"):
    from lightretriever_amd import SQFp16Index
    idx = SQFp16Index(dim, capacity=6000, id_base=100)
    idx.add(integer_rows(dim)[0] if kind == "int" else gauss_rows(dim)[0])
    return idx


# (a width that is no multiple of 64 never has a shadow: its default state is the state without one)
FLAT_STATES = [(dim, n, state) for dim in LONG_DIMS for n in (3000, 6000) for state in ("default", "no_shadow", "six_product")
               if state != "no_shadow" or dim % 64 == 0]


@pytest.mark.parametrize("dim,n,state", FLAT_STATES)
def test_flat_search_over_long_rows_is_the_integer_matmul(dim, n, state):
    """n = 3000 (at most REF_CAND rows) and n = 6000; 5 queries (the exact-fp32 filter) and 40 (the split filter); k = 10 and 1000; with the
    fp16 shadow, without it and with two_pass off."""
    X, q, S = integer_rows(dim)
    idx = flat_index(dim, n, state != "no_shadow")
    idx.two_pass = state != "six_product"
    try:
        for Q in (5, 40):
            for k in (10, 1000):
                same_bits(idx.search(q[:Q], k), integer_topk(S[:Q, :n], k, id_base=100))
    finally:
        idx.two_pass = True


def test_sq_fp16_search_over_long_rows_is_the_integer_matmul():
    dim = 12288
    X, q, S = integer_rows(dim)
    idx = sq_index(dim)
    assert torch.equal(idx.reconstruct_n(5990, 10), X[5990:])            # small integers are fp16 numbers: the codes are the rows
    for Q in (5, 40):
        for k in (10, 1000):
            same_bits(idx.search(q[:Q], k), integer_topk(S[:Q], k, id_base=100))


def integer_range(S, radius, id_base=0):
    mask = S.float() > radius
    lims = torch.zeros(S.shape[0] + 1, dtype=torch.int64, device=S.device)
    lims[1:] = torch.cumsum(mask.sum(dim=1), 0)
    qi, rows = torch.nonzero(mask, as_tuple=True)
    return lims, S[qi, rows].float(), rows + id_base


@pytest.mark.parametrize("dim,kind", [(8224, "flat"), (12288, "flat"), (12288, "sq_fp16")])
def test_range_search_over_long_rows_is_the_integer_matmul(dim, kind):
    """The radius lies between two attained integer scores, about 50 and about 1500 rows per query above it (and one radius nothing reaches)."""
    X, q, S = integer_rows(dim)
    idx = flat_index(dim, 6000) if kind == "flat" else sq_index(dim)
    for Q, per_query in ((5, 50), (40, 1500)):
        v = torch.sort(S[:Q].reshape(-1), descending=True).values
        radius = float(v[per_query * Q]) + 0.5
        want = integer_range(S[:Q], radius, id_base=100)
        assert abs(int(want[0][-1]) - per_query * Q) <= 2 * Q
        same_range(idx.range_search(q[:Q], radius), want)
    assert idx.range_search(q[:5], float(S.max()))[0].tolist() == [0] * 6


@pytest.mark.parametrize("dim,kind", [(8224, "flat"), (12288, "flat"), (12288, "sq_fp16")])
def test_rerank_over_long_rows_is_the_integer_matmul(dim, kind):
    """lrx_flat_ip_rerank / lrx_sq_fp16_ip_rerank through ctypes: 600 candidates per query with a -1, a row >= n and a row named twice, k = 100."""
    import test_gpu_refine_index as TR
    n, Q, nc, k = 3000, 5, 600, 100
    X, q, S = integer_rows(dim)
    rng = np.random.default_rng(dim)
    cand = rng.integers(0, n, (Q, nc))
    cand[:, 7], cand[:, 300], cand[:, 599] = -1, n + 5, cand[:, 0]
    cand[0, 11], cand[0, 12] = 17, 4001 if n > 4001 else 17              # (row 17 twice in query 0)
    want = FY.rerank(q[:Q].cpu().numpy(), X[:n].cpu().numpy(), cand, k, id_base=9)
    Si = S.cpu().numpy()
    for i in range(Q):                                                   # the yardstick's scores are the integer matmul's
        assert np.array_equal(want[0][i], Si[i, want[1][i] - 9].astype(np.float32))
    from lightretriever_amd import _lib
    lib = _lib.lib()
    index = sq_index(dim) if kind != "flat" else None
    torch.cuda.synchronize()
    assert lib.lrx_device_error_count(1) >= 0 and lib.lrx_device_error_count(1) == 0
    if kind == "flat":
        got = TR.rerank_flat(q[:Q], X[:n], cand, k, id_base=9)
    else:
        got = TR.rerank_codes(q[:Q], index, cand, k, id_base=9, n_rows=n)
    # the candidates past the shard are skipped AND counted (the -1 is not): read here, so that the counter is left at zero for the next caller
    assert lib.lrx_device_error_count(1) == int((cand >= n).sum()) == Q and lib.lrx_device_error_count(1) == 0
    TR.assert_yardstick(got, want)


# ---- a corpus that is not made of integers: unit-norm Gaussian rows, checked as tests/test_gpu_search.py checks its cases ----------------
@functools.lru_cache(maxsize=None)
def gauss_rows(dim):
    rng = np.random.default_rng(dim + 1)
    X = rng.standard_normal((6000, dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    q = rng.standard_normal((40, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[:8] = X[np.arange(8) * 700] * np.float32(0.9) + np.float32(0.1) * q[:8]      # queries next to a stored row
    return torch.from_numpy(X).cuda(), torch.from_numpy(q).cuda()


@pytest.mark.parametrize("dim,kind", [(8224, "flat"), (12288, "flat"), (12288, "sq_fp16")])
def test_gaussian_long_rows_search_range_and_rerank(dim, kind):
    from lightretriever_amd import FlatIPIndex
    import test_gpu_range_search as TG
    import test_gpu_refine_index as TR
    from test_gpu_search import check_against_oracle
    X, q = gauss_rows(dim)
    if kind == "flat":
        idx = FlatIPIndex(dim, capacity=6000, id_base=100)
        idx.add(X)
        rows = X
    else:
        idx = sq_index(dim, "gauss")
        rows = X.half().float()                                          # the codes, decoded
        assert torch.equal(idx.reconstruct_n(0, 50), rows[:50])
    for Q, k in ((40, 100), (5, 10)):
        D, I = idx.search(q[:Q], k)
        check_against_oracle(D, I, q[:Q].cpu().numpy(), rows.cpu().numpy(), k, id_base=100)
    # the rerank of a search's own hits, shuffled, reports the search's list bit for bit (include/lrx.h)
    D, I = idx.search(q[:5], 100)
    cand = TR.shuffled(I - 100, seed=3)
    got = TR.rerank_flat(q[:5], X, cand, 100, id_base=100) if kind == "flat" else TR.rerank_codes(q[:5], idx, cand, 100, id_base=100)
    same_bits(got, (D, I))
    radius = float(D[:, 60].max())
    want = TG.range_fp64_gpu(q[:5], rows, radius, id_base=100)
    assert int(want[0][-1]) >= 60
    TG.assert_same(idx.range_search(q[:5], radius), want)


# =====================================================================================================================================
# D. more queries than a grid's y extent holds
# =====================================================================================================================================
MANY = 65_543


def test_pq_more_queries_than_grid_y():
    """65 543 queries over 300 rows: the plan cuts the queries at 65 535 per chunk (k_pq_scan's grid.y), two chunks, inside the declared
    workspace (guard bands on both sides)."""
    import test_gpu_pq_index as TP
    from lightretriever_amd import _lib
    d, M, n, k = 8, 1, 300, 5
    idx, C, codes = TP.make(d, M, n, seed=61)
    lib = _lib.lib()
    assert define("lrx_search_pq.h", "PQ_QC_MAX") == 65535 == int(lib.lrx_pq_ip_chunk_queries(n, d, M, MANY, k))
    need = int(lib.lrx_pq_ip_workspace_bytes(n, d, M, MANY, k))
    assert need == int(lib.lrx_pq_ip_workspace_bytes(n, d, M, 65535, k)) < 200 << 20
    q = torch.from_numpy(TP.queries(MANY, d, seed=62)).cuda()
    g = ws_guard.Guarded(need, "cuda").fill(0xFF).arm()
    ws_guard.plant(idx, g)
    got = idx.search(q, k)
    torch.cuda.synchronize()
    assert g.check().numel() == 0
    ws_guard.assert_planted(idx, g)
    TP.assert_same(got, TP.want_topk(q, C, codes, k))
    # the range search cuts at the same number
    S = TP.Y.scores_torch(TP.lut_torch(q, C), codes)
    radius = float(torch.sort(S.reshape(-1), descending=True).values[3 * MANY])
    TP.assert_same_range(idx.range_search(q, radius), TP.want_range(q, C, codes, radius))


def test_binary_more_queries_than_grid_y():
    """65 543 queries over 300 rows of 8 bits, k = 3 of binary_k = 8: k_bin_rerank_score takes its queries 65 535 per launch.  The yardstick's
    arithmetic without its per-query loops (the byte table of binary_yardstick; grid queries, so the fp64 matmul is exact in any order),
    checked against the loops on the first and the last 40 queries."""
    import test_gpu_binary_index as TB
    assert define("lrx_search_binary.h", "BIN_RR_QMAX") == 65535
    d, n, k, binary_k = 8, 300, 3, 8
    xb = TB.random_packed(n, d, seed=71)
    idx = TB.build(xb, d)
    q = TB.grid_q(MANY, d, seed=72)
    pop8 = torch.from_numpy(BY._POP8.astype(np.int32)).cuda()
    H = pop8[(TB.pack_t(q)[:, :1].long() ^ xb[:, 0].long()[None, :])]
    Dh, C = TB.hamming_topk_t(H, binary_k)
    sign = ((xb[:, :, None].int() >> torch.arange(7, -1, -1, device="cuda")) & 1).reshape(n, d).double() * 2 - 1
    c = torch.sort(C, dim=1).values
    s = torch.gather((q.double() @ sign.T).float(), 1, c)
    v, o = torch.sort(s, dim=1, descending=True, stable=True)
    want = (v[:, :k].contiguous(), torch.gather(c, 1, o[:, :k]))
    for sl in (slice(0, 40), slice(MANY - 40, MANY)):
        Hs = TB.hamming_t(TB.pack_t(q[sl]), xb)
        assert torch.equal(Hs, H[sl])
        TB.assert_same((want[0][sl], want[1][sl]), TB.rerank_t(q[sl], xb, TB.hamming_topk_t(Hs, binary_k)[1], k))
    TB.assert_same(idx.search(q, binary_k, rerank=False), (Dh, C))
    TB.assert_same(idx.search(q, k, binary_k=binary_k), want)


def cycled_impact_queries(n_distinct, Q, vocab, seed):
    """Q queries that walk through n_distinct different ones (the yardstick is asked once per different query)."""
    rng = np.random.default_rng(seed)
    distinct = [(rng.choice(vocab, 1 + i % 5, replace=False), rng.integers(1, 4, 1 + i % 5)) for i in range(n_distinct)]
    which = np.arange(Q) % n_distinct
    return distinct, which, [distinct[i] for i in which]


def test_impact_more_queries_than_grid_y():
    """IMP_QC_MAX: 65 543 queries over 300 rows are two chunks of k_impact_scan's grid.y (the second holds 8 queries; 61 different queries,
    so the chunk boundary falls inside a cycle)."""
    from lightretriever_amd import ImpactIndex, _lib
    from lightretriever_amd.impact_index import query_csr
    rng = np.random.default_rng(81)
    docs = [(rng.choice(50, 6, replace=False), rng.integers(1, 100, 6)) for _ in range(300)]
    distinct, which, queries = cycled_impact_queries(61, MANY, 50, seed=82)
    idx = ImpactIndex()
    idx.add(*IY.csr_of(docs))
    assert int(_lib.lib().lrx_impact_chunk_queries(300, MANY, 5)) == define("lrx_search_impact.h", "IMP_QC_MAX") == 65535
    D, I = IY.Yardstick(*IY.csr_of(docs)).search(distinct, 5)
    same_bits(idx.search(*query_csr(queries), 5), (D[which], I[which]))


def test_impact_query_chunks_under_the_matrix_budget():
    """IMP_MATRIX_BYTES: 1100 queries x 270 000 rows x 4 B is more than the 1 GiB a chunk's score matrix may take -- two query chunks, each
    with its own first query for the scan and its own slice of the outputs."""
    from lightretriever_amd import ImpactIndex, _lib
    from lightretriever_amd.impact_index import query_csr
    n, V, Q, k = 270_000, 400, 1100, 10
    assert Q * n * 4 > define("lrx_search_impact.h", "IMP_MATRIX_BYTES") and n < define("lrx_search_impact.h", "IMP_ROW_CHUNK")
    g = torch.Generator().manual_seed(91)
    terms = ((torch.randint(0, V, (n, 1), generator=g) + torch.arange(4) * 100) % V).reshape(-1).to(torch.int32)     # four distinct terms per row
    weights = torch.randint(1, 50, (n * 4,), generator=g).to(torch.int32)
    off = torch.arange(n + 1, dtype=torch.int64) * 4
    idx = ImpactIndex()
    idx.add(terms.cuda(), weights.cuda(), off.cuda())
    qc = int(_lib.lib().lrx_impact_chunk_queries(n, Q, k))
    assert Q / 2 < qc < Q
    distinct, which, queries = cycled_impact_queries(37, Q, V, seed=92)
    D, I = IY.Yardstick(terms.numpy(), weights.numpy(), off.numpy()).search(distinct, k)
    same_bits(idx.search(*query_csr(queries), k), (D[which], I[which]))


# =====================================================================================================================================
# E. the census is about the constants the library has today
# =====================================================================================================================================
def test_census_names_every_size_constant_with_its_value():
    """Every `#define NAME <integer>` of lrx_search*.h / lrx_search.hip appears in the table above with its value, so a constant that is
    added or changed has to be placed there (and given a crossing test, or a reason)."""
    table = dict(re.findall(r"^\s{4}([A-Z][A-Z0-9_]+)\s+([0-9][0-9_]*)\s", __doc__, re.M))
    for fn in sorted(os.listdir(CSRC)):
        if not fn.startswith("lrx_search"):
            continue
        with open(os.path.join(CSRC, fn)) as f:
            src = f.read()
        for name, val, sh in re.findall(r"^#define\s+([A-Z][A-Z0-9_]+)\s+\(?(\d+)(?:ll\s*<<\s*(\d+)\))?\s*(?://.*)?$", src, re.M):
            assert name in table, f"{fn}: {name} is not in the census"
            assert int(table[name].replace("_", "")) == int(val) << int(sh or 0), (name, table[name])
