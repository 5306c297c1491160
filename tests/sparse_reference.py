"""The reference of the sparse-hit path, written once: the sparsify and compaction kernels of lightretriever_amd/csrc/lrx_sparse.hip
(k_sparse_transform, k_topk_threshold, k_sparse_compact and its CSR form) and the hit-fusion kernels of lrx_fuse.hip (k_hit_contrib,
k_hit_union), each restated in numpy, and the inputs the GPU tests run -- generated here so that the host test that proves what the inputs
claim (tests/test_sparse_reference_host.py) sees the same arrays as tests/test_gpu_sparse_reference.py.  Plain numpy; nothing from
lightretriever_amd and no torch.

Everything but one library call is exactly reproducible, so the comparisons are bit-level:
  top-k threshold   a pure selection: the k-th largest value, everything strictly below it becomes the filter value, survivors keep their bits.
  quantisation      one fp32 product and round-half-even; numpy's fp32 product and np.rint are the same operations.
  fusion            IEEE double in a fixed order (division, one multiplication, sums in system order).
  log1pf            the one inexact ingredient.  The reference takes log1p in float64 and rounds ONCE to fp32.  LOG1PF_MEASURED_ULP is the
                    largest error of the device's log1pf against float64, in fp32 ulps of the float64 result, over every positive finite bf16
                    argument and 2^18 random fp32 arguments in [2^-30, 2^30] (test_gpu_sparse_reference.py::test_log1pf_alone measures it and
                    requires it to stay within the figure below).  No HIP math documentation ships with the compiler, so BUDGET_ULP, what a
                    test grants, is that figure doubled and rounded up to a whole ulp.
Why the bf16-rounded path needs no budget at all: in production the kernel's arguments are bf16 numbers (the max-aggregate output is bf16).
For none of the 32 639 positive finite bf16 arguments does fp32(log1p64(x)) lie within MIDPOINT_CLEAR_ULP = 4 fp32 ulps of a bf16 rounding
midpoint (the nearest, at x = 7.447e26, is 5.6 ulps away; proven on the host), so any log1pf good to 4 ulp rounds every one of them to the same bf16 number as the
reference: the rounded path is compared exhaustively, bit for bit, nothing excluded.  BUDGET_ULP must therefore not exceed 4.
The unrounded path quantises log1pf's fp32 result directly; there an element may be left out only when float64 log1p(x) * q lies within
BUDGET_ULP * ulp * q of a half-integer (near_half).  The doubling leaves at least half the budget spare, which covers the one further rounding
on the way, the fp32 product's (half an ulp of x * q, below ulp * q).  At most NEAR_HALF_CAP of a case's elements may be left out."""
import functools

import numpy as np

BF16_MIN = np.float32(-3.3895313892515355e38)        # torch.finfo(torch.bfloat16).min: the running-max start value of the aggregation
N_POSITIVE_BF16 = 32639                              # bit patterns 0x0001 .. 0x7f7f
MIDPOINT_CLEAR_ULP = 4.0
LOG1PF_MEASURED_ULP = 0.56                           # measured on an MI355X (gfx950, ROCm 7 hipcc -O3): 0.5577 ulp, at x = 0.37241006 (bf16 arguments alone: 0.5299)
BUDGET_ULP = 2.0                                     # ceil(2 * 0.56)
NEAR_HALF_CAP = 0.005
Q_PRODUCTION = 100


# ---------------------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits(a):
    """the uint32 bit patterns of an fp32 array"""
    return f32(a).view(np.uint32)


def bf16_rne(x):
    """fp32 -> the nearest bf16 number (ties to even on the bit pattern), as fp32 with zero low 16 bits"""
    u = bits(x).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def ulp32(y):
    """the fp32 unit in the last place at the float64 value y (2^-149 below the normal range)"""
    _, e = np.frexp(np.abs(np.asarray(y, np.float64)))
    return np.ldexp(1.0, np.maximum(e, -125) - 24)


def positive_bf16():
    """every positive finite bf16 number, ascending, as fp32 (bf16's subnormals included)"""
    return (np.arange(1, 0x7F80, dtype=np.uint32) << 16).view(np.float32)


def midpoint_distance_ulp(y):
    """distance of the float64 value y > 0 from the nearest bf16 rounding midpoint, in fp32 ulps of y"""
    y = np.asarray(y, np.float64)
    _, e = np.frexp(y)
    s = np.ldexp(y, 8 - np.maximum(e, -125))          # bf16 numbers are the integers on this scale, an fp32 ulp is 2^-16
    return np.abs(s - np.floor(s) - 0.5) * 65536.0


# ---------------------------------------------------------------------------------------------------------------
# k_topk_threshold: the key map, the radix trace, the selection
# ---------------------------------------------------------------------------------------------------------------
def f32_key(x):
    """the order-preserving uint32 key of k_topk_threshold: negative numbers have all bits flipped, the others the sign bit set"""
    b = bits(x)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_f32(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def radix_trace(row, k):
    """The bucket the 4-pass radix select settles on in each 8-bit pass, most significant digit first, for the k-th largest key of the row:
    -> (buckets [4], the selected value).  Restates the kernel's walk (histogram of the keys under the prefix, scan from bucket 255 down)."""
    keys = f32_key(row).astype(np.uint64)
    need, prefix, out = int(k), 0, []
    for p in range(4):
        shift = 24 - 8 * p
        sel = keys if p == 0 else keys[(keys >> (shift + 8)) == prefix]
        hist = np.bincount(((sel >> shift) & 255).astype(np.int64), minlength=256)
        b = 255
        while hist[b] < need and b > 0:
            need -= int(hist[b])
            b -= 1
        out.append(b)
        prefix = (prefix << 8) | b
    return out, key_f32(np.uint32(prefix))[()]


def effective_k(top_k, min_keep, cols):
    return min(max(int(top_k), int(min_keep)), int(cols))


def topk_threshold(x, k, filter_value=0.0):
    """Per row: the k-th largest value BY VALUE (np.partition), everything strictly below it becomes filter_value, ties with it survive
    (finetune/sparse_pooling.py:92-109).  Survivors keep their bits.  1 <= k <= cols."""
    x = np.atleast_2d(f32(x))
    cols = x.shape[1]
    kth = np.partition(x, cols - k, axis=1)[:, cols - k:cols - k + 1]
    return np.where(x < kth, np.float32(filter_value), x)


def sparsify(x, relu=True, log1p=True, round_bf16=False, top_k=0, min_keep=8):
    """-> (out fp32, y64).  relu, then log1p in float64 rounded once to fp32 (then RNE to bf16 if asked), then the top-k threshold with
    k = min(max(top_k, min_keep), cols) when top_k > 0.  y64: the float64 value before any rounding (where a test places its ulp budget)."""
    x = np.atleast_2d(f32(x))
    if relu:
        x = np.maximum(x, np.float32(0))
    y64 = x.astype(np.float64)
    if log1p:
        with np.errstate(invalid="ignore", divide="ignore"):
            y64 = np.log1p(y64)
        x = y64.astype(np.float32)
        if round_bf16:
            x = bf16_rne(x)
    if top_k > 0:
        x = topk_threshold(x, effective_k(top_k, min_keep, x.shape[1]))
    return x, y64


def quantise(x, q):
    """rint(max(x, 0) * q) with the product in fp32 (oracle.quantize_sparse, finetune/sparse_converter_mixin.py:129-133); a float64 product
    would differ at the halves.  max is fmaxf: a NaN gives 0.  int64, so that the largest product below 2^31 needs no care."""
    return np.rint(np.fmax(f32(x), np.float32(0)) * np.float32(q)).astype(np.int64)


def compact(x, q, capacity=None):
    """-> (ids, weights, counts): per row the columns with a non-zero quantised weight in ascending order and the weights, the first
    `capacity` of them; counts is the TRUE number, not the stored one."""
    w = quantise(np.atleast_2d(x), q)
    ids, weights, counts = [], [], []
    for row in w:
        nz = np.flatnonzero(row)
        counts.append(nz.size)
        nz = nz[:capacity]
        ids.append(nz.astype(np.int32))
        weights.append(row[nz].astype(np.int32))
    return ids, weights, np.asarray(counts, np.int32)


def near_half(y64, q, budget_ulp=None):
    """the elements a test of the unrounded path may leave out: float64 log1p(x) * q within budget * ulp * q of a half-integer"""
    budget_ulp = BUDGET_ULP if budget_ulp is None else budget_ulp
    p = np.asarray(y64, np.float64) * q
    return np.abs(p - np.floor(p) - 0.5) <= budget_ulp * ulp32(y64) * q


# ---------------------------------------------------------------------------------------------------------------
# k_hit_contrib / k_hit_union
# ---------------------------------------------------------------------------------------------------------------
def contributions(scores, ids, method, p0, p1=0.0):
    """float64 [Q, k].  Slots with id < 0 take no part and give 0.  method 'rrf': 1 / (p0 + rank), ranks from 1 by score descending,
    earlier position first among equals (a stable sort, like the oracle's).  'linear': (s - min) / (max - min + p1) * p0 in that order."""
    scores, ids = np.atleast_2d(np.asarray(scores, np.float64)), np.atleast_2d(np.asarray(ids, np.int64))
    out = np.zeros_like(scores)
    for q in range(scores.shape[0]):
        pos = np.flatnonzero(ids[q] >= 0)
        if pos.size == 0:
            continue
        s = scores[q, pos]
        if method == "rrf":
            order = np.argsort(-s, kind="stable")
            out[q, pos[order]] = 1.0 / (np.float64(p0) + np.arange(1, pos.size + 1, dtype=np.float64))
        else:
            out[q, pos] = (s - s.min()) / (s.max() - s.min() + np.float64(p1)) * np.float64(p0)
    return out


def union(ids_cat, contrib_cat):
    """-> (scores f64 [Q, n], ids i64 [Q, n], counts i32 [Q]).  A document's contributions are summed in list-position order (= system
    order), starting from 0.0; rows sorted by fused score descending, lower id first among equals; -inf / -1 padding."""
    ids_cat, contrib_cat = np.atleast_2d(np.asarray(ids_cat, np.int64)), np.atleast_2d(np.asarray(contrib_cat, np.float64))
    Q, n = ids_cat.shape
    sc, out_ids, counts = np.full((Q, n), -np.inf), np.full((Q, n), -1, np.int64), np.zeros(Q, np.int32)
    for q in range(Q):
        tot = {}
        for i, c in zip(ids_cat[q].tolist(), contrib_cat[q]):
            if i >= 0:
                tot[i] = tot.get(i, np.float64(0.0)) + c
        order = sorted(tot.items(), key=lambda kv: (-kv[1], kv[0]))
        counts[q] = len(order)
        out_ids[q, :len(order)] = [i for i, _ in order]
        sc[q, :len(order)] = [v for _, v in order]
    return sc, out_ids, counts


def fuse(systems, method, rrf_k=60, weights=None, eps=1e-8):
    """systems [(scores [Q, k_i], ids [Q, k_i])] -> (contributions per system, union(...))"""
    con = [contributions(s, i, method, *((rrf_k, 0.0) if method == "rrf" else (weights[j], eps))) for j, (s, i) in enumerate(systems)]
    return con, union(np.concatenate([i for _, i in systems], 1), np.concatenate(con, 1))


def systems_to_dicts(systems):
    """the dict-of-dicts form the oracle (and the reference project) fuses: per system {query: {doc: score}} over the valid slots, a query
    without any left out"""
    return [{str(q): {str(int(p)): float(v) for p, v in zip(i[q], s[q]) if p >= 0} for q in range(len(i)) if (i[q] >= 0).any()} for s, i in systems]


def dicts_to_systems(results_list):
    """score_fuse_utils._dicts_to_arrays in numpy: -> (query names, doc names, [(scores, ids)])"""
    qids, pids = {}, {}
    for res in results_list:
        for q, passages in res.items():
            qids.setdefault(str(q), len(qids))
            for p in passages:
                pids.setdefault(str(p), len(pids))
    systems = []
    for res in results_list:
        kmax = max([len(v) for v in res.values()] + [1])
        sc, ids = np.zeros((len(qids), kmax)), np.full((len(qids), kmax), -1, np.int64)
        for q, passages in res.items():
            r = qids[str(q)]
            sc[r, :len(passages)] = [float(v) for v in passages.values()]
            ids[r, :len(passages)] = [pids[str(p)] for p in passages]
        systems.append((sc, ids))
    return list(qids), list(pids), systems


def fused_to_dicts(sc, ids, counts, qnames=None, pnames=None):
    return {(qnames[q] if qnames else str(q)): {(pnames[int(i)] if pnames else str(int(i))): float(v) for i, v in zip(ids[q, :counts[q]], sc[q, :counts[q]])}
            for q in range(len(counts)) if qnames or counts[q] > 0}


# ---------------------------------------------------------------------------------------------------------------
# case tables: threshold select
# ---------------------------------------------------------------------------------------------------------------
THRESHOLD_COLS = (1, 7, 255, 256, 257, 1023, 1024, 1025, 3001, 4097)      # below, at and above one pass of the kernel's 1024 threads
THRESHOLD_ROWS = 5
PAD = 3                                                                    # the strided form: rows of cols + PAD floats
PAD_SENTINEL = np.float32(12345.0)
DENORM = np.float32(1.4e-45)
FLT_BIG = np.float32(3.4e38)
SPECIALS = f32([0.0, -0.0, DENORM, -DENORM, np.inf, -np.inf, FLT_BIG, -FLT_BIG, 1.0, -1.0, 1.1754944e-38, -1.1754944e-38, 2.0 * DENORM, -2.0 * DENORM])


def threshold_calls(cols):
    """(top_k, min_keep) of every launch on a matrix of this width: top_k in {1, 2, cols - 1, cols, cols + 5} and one with min_keep > top_k"""
    ks = sorted({k for k in (1, 2, cols - 1, cols, cols + 5) if k > 0})
    return [(k, 0) for k in ks] + [(1, 3)]


def _shuffled(rng, a):
    a = f32(a)
    return a[rng.permutation(a.size)]


def tie_row(cols, k, rng):
    """m ties T = 1.5 around the k-th place, j < m of them inside the top k where the row has room (all m survive): g = k - j greater values,
    the m ties, the rest lower.  -> (row, m, g)"""
    m = min(4, cols)
    j = max(min(max(1, min(2, m - 1)), k), k + m - cols)
    g = k - j
    hi = 2.0 + np.arange(g, dtype=np.float64) / 8.0
    lo = 1.0 - np.arange(cols - g - m, dtype=np.float64) / 8.0
    return _shuffled(rng, np.concatenate([hi, np.full(m, 1.5), lo])), m, g


def zero_threshold_row(cols, k, rng):
    """k - 1 positive values (the denormal among them), then +0.0 and -0.0 where there is room, then negatives starting with the negative
    denormal: the k-th largest is a zero, so -1.4e-45 lies below the threshold and is filtered -- a flush-to-zero compare would keep it"""
    g = k - 1
    z = min(2, cols - g)
    pos = np.resize(f32([DENORM, 1.0, np.inf, FLT_BIG, 2.0 * DENORM]), g)
    neg = np.resize(f32([-DENORM, -2.0 * DENORM, -1.0, -np.inf, -FLT_BIG]), cols - g - z)
    return _shuffled(rng, np.concatenate([pos, f32([0.0, -0.0])[:z], neg]))


RADIX_OTHER_BYTES = (0x00800000, 0xC0004020, 0xC0400020, 0xC0402000)   # digit 0: -FLT_MAX (bucket 0) .. +inf (bucket 255), no NaN in between


def radix_row(cols, k, digit, bucket, rng):
    """Keys that differ only in byte `digit` (0 = most significant), the k-th largest in `bucket` (0 or 255) of that digit.
    bucket 255: k + 1 keys there where the row has room (their ties straddle k), the others spread over buckets 0 .. 254.
    bucket 0: k - 1 keys spread over buckets 1 .. 255, all others in bucket 0."""
    shift = 24 - 8 * digit
    if bucket == 255:
        n_top = min(cols, k + 1)
        byte = np.concatenate([np.full(n_top, 255), np.arange(cols - n_top) % 255])
    else:
        byte = np.concatenate([1 + np.arange(k - 1) % 255, np.zeros(cols - (k - 1), np.int64)])
    keys = (np.uint32(RADIX_OTHER_BYTES[digit]) | (byte.astype(np.uint32) << np.uint32(shift))).astype(np.uint32)
    return _shuffled(rng, key_f32(keys))


def sign_row(cols, k, rng, negative_kth):
    """small normal numbers of both signs; the k-th largest is the largest negative one (negative_kth: pass 0 settles on bucket 0x7f) or the
    smallest positive one (0x80): the two sides of the key map's sign flip"""
    tiny = 1.1754944e-38
    n_pos = (k - 1) if negative_kth else min(cols, k)
    return _shuffled(rng, np.concatenate([tiny * (1 + np.arange(n_pos)), -tiny * (1 + np.arange(cols - n_pos))]))


@functools.lru_cache(maxsize=None)
def threshold_matrices(cols, k):
    """The matrices (5 rows each) a launch with effective k runs: {name: fp32 [5, cols]}.  'edge': all equal, all BF16_MIN, the tie group,
    the zero threshold, the specials; 'radix0' / 'radix255': one row per key byte with the k-th in that bucket, and a side of the sign
    flip; 'random': bf16-valued normals (plenty of exact ties)."""
    rng = np.random.default_rng(cols * 10007 + k)
    edge = np.stack([np.full(cols, -1.0, np.float32), np.full(cols, BF16_MIN, np.float32), tie_row(cols, k, rng)[0], zero_threshold_row(cols, k, rng),
                     _shuffled(rng, np.resize(SPECIALS, cols))])
    r0 = np.stack([radix_row(cols, k, d, 0, rng) for d in range(4)] + [sign_row(cols, k, rng, True)])
    r255 = np.stack([radix_row(cols, k, d, 255, rng) for d in range(4)] + [sign_row(cols, k, rng, False)])
    rnd = bf16_rne(rng.standard_normal((THRESHOLD_ROWS, cols)).astype(np.float32) * 2)
    out = {"edge": edge, "radix0": r0, "radix255": r255, "random": rnd}
    for m in out.values():
        m.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------
# case tables: transform
# ---------------------------------------------------------------------------------------------------------------
EXHAUSTIVE_SHAPE = (7, 4663)          # 32 641 = the 32 639 positive bf16 numbers, 0.0 and BF16_MIN; 4663 = 4 x 1024 + 567


@functools.lru_cache(maxsize=None)
def exhaustive_bf16():
    """every positive finite bf16 number once, 0.0 and BF16_MIN, in a fixed random order (so that every row mixes all magnitudes)"""
    v = np.concatenate([positive_bf16(), f32([0.0, BF16_MIN])])
    x = v[np.random.default_rng(32639).permutation(v.size)].reshape(EXHAUSTIVE_SHAPE)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def log1pf_arguments():
    """what LOG1PF_MEASURED_ULP is measured over: every positive finite bf16 number, then 2^18 log-uniform fp32 numbers in [2^-30, 2^30]"""
    x = np.concatenate([positive_bf16(), (2.0 ** np.random.default_rng(18).uniform(-30, 30, 1 << 18)).astype(np.float32)])
    x.setflags(write=False)
    return x


def log1pf_error_ulp(got, x):
    """error of fp32 results against float64 log1p, in fp32 ulps of the float64 result"""
    y = np.log1p(np.asarray(x, np.float64))
    return np.abs(np.asarray(got, np.float64) - y) / ulp32(y)


def near_half_cases():
    """(name, near mask, q) of every unrounded-path input the GPU tests quantise: what the host test caps at NEAR_HALF_CAP"""
    x = exhaustive_bf16()
    yield "exhaustive bf16, q=100", near_half(sparsify(x, True, True, False)[1], Q_PRODUCTION), Q_PRODUCTION


# ---------------------------------------------------------------------------------------------------------------
# case tables: capacity compaction
# ---------------------------------------------------------------------------------------------------------------
COMPACT_COLS = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
OUT_SENTINEL = -7                                                          # prefill of ids / weights: no id and no weight is negative
COMPACT_PAD_VALUE = np.float32(7.0)                                        # row padding: would be an entry if it were read


@functools.lru_cache(maxsize=None)
def compact_rows(cols):
    """fp32 [4, cols]: every entry non-zero, none (zeros and negatives), the first and the last column only, about 3 % random (a few negative)"""
    rng = np.random.default_rng(cols * 31 + 5)
    x = np.zeros((4, cols), np.float32)
    x[0] = rng.random(cols, dtype=np.float32) + 0.02
    x[1] = np.where(rng.random(cols) < 0.5, 0.0, -rng.random(cols) - 0.01)
    x[2, 0], x[2, cols - 1] = 0.37, 2.5
    x[3] = np.where(rng.random(cols) < 0.03, rng.random(cols) * 3, 0) * np.where(rng.random(cols) < 0.1, -1, 1)
    x[3, cols // 2] = 1.25                                                 # never empty
    x.setflags(write=False)
    return x


def compact_capacities(cols, q=Q_PRODUCTION):
    """capacities that cut inside a wave (37), exactly at a wave end (64), at the end of a 1024-column chunk, and at each row's count and
    count +- 1"""
    counts = compact(compact_rows(cols), q)[2]
    return sorted({c for c in [37, 64, 1024] + [int(n) + d for n in counts for d in (-1, 0, 1)] if c >= 1})


Q_EXACT = 64                                                               # a power of two: x = v / 64 and x * 64 are exact
MAX_PRODUCT = 2147483520.0                                                 # the largest fp32 number below 2^31


def exact_rows():
    """fp32 [2, 70] at q = 64.  Row 0: the halves (n + 0.5) / 64 for n = 0 .. 63 (products exact: round half to even), then 0.49999997 / 64, a
    NaN, a negative, the largest product below 2^31, 1e-9 and 1.0.  Row 1: NaN only (no entry at all)."""
    x = np.zeros((2, 70), np.float32)
    x[0, :64] = (np.arange(64) + 0.5) / 64.0
    x[0, 64:] = [0.49999997 / 64.0, np.nan, -3.0, MAX_PRODUCT / 64.0, 1e-9, 1.0]
    x[1] = np.nan
    assert (x[0, :64] * np.float32(64) == np.arange(64) + 0.5).all() and float(x[0, 67]) * 64.0 == MAX_PRODUCT
    return x


# ---------------------------------------------------------------------------------------------------------------
# case tables: fusion
# ---------------------------------------------------------------------------------------------------------------
SCORE_PAD_SENTINEL = 777.0
ID_PAD_SENTINEL = 5                   # a valid-looking id: reading it as an entry would change the result
OUT_F64_SENTINEL = -123.25
OUT_I64_SENTINEL = -99
FUSE_PAD = 3


def _system(rng, Q, k, pool, flavour, id_offset):
    ids = np.stack([rng.choice(pool, size=k, replace=False) for _ in range(Q)]).astype(np.int64) + id_offset
    if flavour == "gauss":
        sc = np.sort(rng.standard_normal((Q, k)), axis=1)[:, ::-1].copy()
    elif flavour == "impact":                                              # integer scores, sorted as a search returns them: long tie runs
        sc = np.sort(rng.integers(1, max(3, k // 40 + 3), size=(Q, k)).astype(np.float64), axis=1)[:, ::-1].copy()
    elif flavour == "impact_unsorted":
        sc = rng.integers(-3, 4, size=(Q, k)).astype(np.float64)
    else:
        raise ValueError(flavour)
    return sc, ids


def _fusion_case(name, ks, Q, flavour, holes, id_offset=0, seed=0):
    rng = np.random.default_rng(seed + 1000 * len(ks) + sum(ks))
    pool = max(ks) + max(ks) // 2 + 3
    systems = []
    for s, k in enumerate(ks):
        sc, ids = _system(rng, Q, k, pool, flavour, id_offset)
        if holes:
            ids[rng.random((Q, k)) < 0.15] = -1                            # holes in the interior of the lists, not only at the tail
            if s == len(ks) - 1 and Q > 1:
                ids[Q - 1, :] = -1                                         # a list with no valid slot
            if s == 0 and k > 2:
                ids[0, k // 2:] = -1                                       # a short list
        systems.append((sc, ids))
    return dict(name=name, systems=systems, weights=[0.7, 0.3, 0.2, 0.1][:len(ks)], eps=1e-8, rrf_k=60)


def _linear_edges(eps):
    """Q = 3, four systems.  System 0: all scores equal (den = eps, contributions 0) / one valid slot / no valid slot.  System 1: negative
    scores with ties and a hole.  System 2: scores from 1e-30 to 1e30.  System 3 carries a zero weight."""
    s0 = (np.full((3, 5), 4.25), np.array([[1, 2, 3, 4, 5], [-1, -1, 9, -1, -1], [-1, -1, -1, -1, -1]], np.int64))
    s1 = (np.array([[-1.5, -7.0, -1.5, -1e3, -0.25], [-2.0, -2.0, -2.0, -2.0, -3.0], [-9.0, -8.0, -7.0, -6.0, -5.0]]),
          np.array([[3, 2, 11, -1, 12], [9, 1, 2, 3, 4], [7, 6, 5, 4, 3]], np.int64))
    s2 = (np.array([[1e-30, 1e30, 1.0, 3e-10, 5e12, 1e-30, 2.5]] * 3) * np.array([[1.0], [-1.0], [1.0]]),
          np.array([[1, 2, 3, 11, 20, 21, 22], [9, 8, 7, 6, 5, 4, 3], [3, 4, -1, 5, 6, -1, 7]], np.int64))
    s3 = (np.array([[3.0, 2.0, 1.0]] * 3), np.array([[1, 2, 3], [9, 3, 1], [5, 6, 7]], np.int64))
    return dict(name=f"linear edges eps={eps:g}", systems=[s0, s1, s2, s3], weights=[0.5, 0.3, 0.2, 0.0], eps=eps, rrf_k=60)


@functools.lru_cache(maxsize=None)
def fusion_cases():
    """Per-system k in {1, 2, 3, 63, 64, 65, 1000, 1024, 2048} and 4096 alone; totals 1, 2, 5, 4095, 4096; one to four systems (4 x 1024
    among them); Q in {1, 3}.  Ids are unique within a list (the dict form the oracle fuses cannot say anything else)."""
    return [
        _fusion_case("1 entry", (1,), 1, "gauss", False),
        _fusion_case("2 entries, 2 systems", (1, 1), 3, "impact", False),
        _fusion_case("5 entries", (2, 3), 3, "impact_unsorted", False, id_offset=2 ** 32 + 5),
        _fusion_case("63 + 64 + 65, holes", (63, 64, 65), 3, "impact_unsorted", True, id_offset=2 ** 62 - 10000),
        _fusion_case("63 + 64 + 65, gauss", (63, 64, 65), 1, "gauss", True),
        _fusion_case("4095 entries, 4 systems", (2048, 1024, 1000, 23), 3, "impact", True),
        _fusion_case("4 x 1024, gauss", (1024,) * 4, 3, "gauss", False),
        _fusion_case("4 x 1024, impact, holes", (1024,) * 4, 1, "impact", True, id_offset=2 ** 32 + 5),
        _fusion_case("4096 alone", (4096,), 1, "impact", True),
        _fusion_case("2 x 2048", (2048, 2048), 1, "impact_unsorted", True, seed=3),
        _fusion_case("3 x 1000", (1000,) * 3, 3, "impact", True, seed=4),
        _linear_edges(1e-8),
        _linear_edges(1e-6),
    ]


ORDER_CONTRIB = (1e16, 1.0, -1e16, 1.0)          # summed in this order: ((1e16 + 1) - 1e16) + 1 = 1; as 1e16 - 1e16 + 1 + 1 it is 2


@functools.lru_cache(maxsize=None)
def union_cases():
    """Hand-made (name, ids_cat [Q, n], contrib_cat [Q, n]) for lrx_hit_union alone.  'order': 40 documents present in each of four systems of
    64 slots with ORDER_CONTRIB (the sum in system order differs from the sum in another order), ids above 2^32 and near 2^62, holes.
    'equal': equal fused scores, to be ordered by id; a row without any valid entry."""
    rng = np.random.default_rng(11)
    k, docs = 64, 40
    ids = np.full((3, 4 * k), -1, np.int64)
    con = rng.random((3, 4 * k))
    base = [0, 2 ** 32 + 1, 2 ** 62 - 5000]
    for q in range(3):
        for s in range(4):
            slots = rng.permutation(k)
            ids[q, s * k + slots[:docs]] = base[q] + np.arange(docs) * 3
            con[q, s * k + slots[:docs]] = ORDER_CONTRIB[s]
            ids[q, s * k + slots[docs:docs + 10]] = base[q] + 1000 + 50 * s + np.arange(10)      # documents of one system only
    eq_ids = np.array([[8, 3, 2 ** 40, 5, -1, 3, 8, 1], [-1] * 8, [4, 4, 4, 4, 2, 2, 2, 2]], np.int64)
    eq_con = np.array([[0.5, 0.25, 0.5, 0.5, 9.0, 0.25, 0.0, 0.5], [1.0] * 8, [0.25, 0.25, 0.25, 0.25, 0.5, 0.5, 0.0, 0.0]])
    one = (np.array([[2 ** 62 - 1]], np.int64), np.array([[0.125]]))
    return [("order", ids, con), ("equal", eq_ids, eq_con), ("one entry", *one)]
