"""Host model of the shared top-k selection (lrx_search_select.h: select_topk_sorted, rescore_band) and the crafted score rows that put it
on every one of its data-dependent branches.  numpy only.

  order       key(s) is f2key (lrx_common.h); topk(s, k) is an np.lexsort over (row, -key): key descending, ties to the lower row,
              (-FLT_MAX, -1) padding.  It restates the contract, not the kernel.
  predictors  select_path(s, k) says which branch of select_topk_sorted a score row takes and the counts that decided it; band_form(s, k,
              gap) says which form of rescore_band the band `s >= kth - gap` takes.  Both read nothing but the row.
  harnesses   three ways of making an EXISTING index report an intended integer score row exactly, so that the selection is the only step
              that can go wrong:
                PQ    PQIndex(16, 16), dsub = 1, tables A (sub-space 0) and B (sub-space 1), zero centroids elsewhere, queries a e0 + b e1
                      with a, b in {0, 1, -1}: with A[j] = 256 j, B[j] = j the fp32 sum ((0 + a A[c0]) + b B[c1]) + 0 ... is the integer
                      +-(256 c0 + c1), exact.  The "special" tables put infinities, +-FLT_MAX, +-FLT_MIN, denormals and 0 into A (B = 0).
                flat  FlatIPIndex(32), two_pass = False, rows (level, 0, ..., 0), queries +-e0: matrix score = exact score = +-level.
                SQ8   SQ8Index(64, "QT_8bit_uniform"), trained = (0, 255), code column 0 = level, queries +-e0: the contract's score is a
                      strictly increasing function of the level (about level + 0.5), taken from sq8_yardstick, never from the level itself.
  CASES       the PQ cases (-> k_topk_select) and BAND_CASES (-> k_topk_select_rescore<ROWS_F32> and k_sq8_select_rescore), each with the
              label it must land on.  test_select_reference_host.py proves the labels on the CPU; test_gpu_select_paths.py runs the cases."""
import numpy as np

# ---- the caps of lrx_search_select.h / lrx_search_filter.h (test_select_reference_host.py greps them out of the headers) ----------------------
SEL_CAND = 4096       # candidate buffer: whole rows up to it, the fast path's gather, the band's list
SEL_EQCAP = 2048      # ties with the k-th key sorted in LDS up to it; the block lists hold 2 * SEL_EQCAP entries
SEL_MAXK = 2048
SP_ROWS = 128         # rows per block maximum
SQ8_NMAX = 16319      # lrx_search_sq8.h: the two-digit weights of the 8-bit filter

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
FLT_MIN = F32(np.finfo(np.float32).tiny)
DENORM = F32(np.finfo(np.float32).smallest_subnormal) * F32(3)

SELECT_LABELS = ("direct", "fast", "fast>cand>exact/sorted", "fast>cand>exact/scan", "fast>blocks>exact/scan", "exact/sorted", "exact/scan")
BAND_LABELS = ("in-list", "stream/rows", "stream/blocks")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# order
# ---------------------------------------------------------------------------------------------------------------------------------------------
def key(s) -> np.ndarray:
    """f2key: a uint32 that orders like the float (negative: all bits flipped; otherwise: the sign bit set)."""
    u = np.ascontiguousarray(s, dtype=F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def topk(s, k: int, id_base: int = 0, row_map=None):
    """One score row -> (D fp32 [k], I int64 [k])."""
    s = np.ascontiguousarray(s, dtype=F32).reshape(-1)
    n = s.shape[0]
    kk = min(k, n)
    order = np.lexsort((np.arange(n, dtype=np.int64), -key(s).astype(np.int64)))[:kk]
    D = np.full(k, -FLT_MAX, F32)
    I = np.full(k, -1, np.int64)
    D[:kk] = s[order]
    I[:kk] = np.asarray(row_map, dtype=np.int64)[order] if row_map is not None else order + id_base
    return D, I


def topk_rows(S, k: int, id_base: int = 0, row_map=None):
    """topk of every row of S [Q, n] -> (D [Q, k], I [Q, k])."""
    pairs = [topk(s, k, id_base, row_map) for s in S]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# predictors
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _kth_largest(a: np.ndarray, kk: int):
    return np.partition(a, a.shape[0] - kk)[a.shape[0] - kk]


def block_max_keys(ky: np.ndarray, pad_blocks: int = 0) -> np.ndarray:
    """Keys of the 128-row block maxima over the valid rows; pad_blocks further blocks without a valid row hold -FLT_MAX (the flat score
    kernels cover whole 256-row tiles)."""
    bm = np.maximum.reduceat(ky, np.arange(0, ky.shape[0], SP_ROWS))
    return np.concatenate([bm, np.full(pad_blocks, key(-FLT_MAX), np.uint32)]) if pad_blocks else bm


def select_path(s, k: int, pad_blocks: int = 0):
    """-> (label, counts): which branch of select_topk_sorted the row takes.  counts: nb (blocks whose maximum reaches the block threshold),
    cand (rows at or above it), neq (rows carrying the k-th key), need_eq (how many of them belong to the top-k); None where the kernel
    never computes the figure."""
    ky = key(np.asarray(s).reshape(-1))
    N = ky.shape[0]
    keff = min(k, N)
    c = dict(nb=None, cand=None, neq=None, need_eq=None)
    if N <= SEL_CAND:
        return "direct", c
    prefix = ""
    bm = block_max_keys(ky, pad_blocks)
    if bm.shape[0] >= keff:
        thr = _kth_largest(bm, keff)
        c["nb"] = int((bm >= thr).sum())
        if c["nb"] > 2 * SEL_EQCAP:
            prefix = "fast>blocks>"
        else:
            c["cand"] = int((ky >= thr).sum())       # (a row at or above the threshold lies in a block whose maximum is)
            if c["cand"] <= SEL_CAND:
                return "fast", c
            prefix = "fast>cand>"
    kth = _kth_largest(ky, keff)
    c["neq"] = int((ky == kth).sum())
    c["need_eq"] = keff - int((ky > kth).sum())
    return prefix + ("exact/sorted" if c["neq"] <= SEL_EQCAP else "exact/scan"), c


def band_counts(s, k: int, thr_gap: float):
    """(rows, blocks) of the band: rows with s >= kth - thr_gap and the 128-row blocks that hold one."""
    s = np.asarray(s, dtype=F32).reshape(-1)
    kth = float(_kth_largest(s, min(k, s.shape[0])))
    hit = s.astype(np.float64) >= kth - thr_gap
    return int(hit.sum()), int(np.logical_or.reduceat(hit, np.arange(0, s.shape[0], SP_ROWS)).sum())


def band_form(s, k: int, thr_gap: float) -> str:
    """Which form of rescore_band the band takes (block maxima present, finite threshold)."""
    if np.asarray(s).size <= SEL_CAND:
        return "in-list"
    rows, blocks = band_counts(s, k, thr_gap)
    if blocks > 2 * SEL_EQCAP:
        return "stream/blocks"
    return "stream/rows" if rows > SEL_CAND else "in-list"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# PQ harness
# ---------------------------------------------------------------------------------------------------------------------------------------------
PQ_D = PQ_M = 16
SPECIALS = np.array([-np.inf, -FLT_MAX, -1.0, -FLT_MIN, -DENORM, 0.0, DENORM, FLT_MIN, 1.0, FLT_MAX, np.inf], dtype=F32)
PQ_QUERIES = ((1, 1), (1, 0), (0, 1), (-1, -1))      # rows: 256 c0 + c1, 256 c0 (256 levels full of ties), c1, the reversed order
SPECIAL_QUERIES = ((1, 0), (-1, 0))                  # a = +-1 only: 0 * inf would put NaN into the table


def pq_tables(special: bool = False) -> np.ndarray:
    """Centroids fp32 [16, 256, 1]."""
    C = np.zeros((PQ_M, 256, 1), F32)
    j = np.arange(256)
    if special:
        C[0, :, 0] = SPECIALS[j % SPECIALS.shape[0]]
    else:
        C[0, :, 0] = 256 * j
        C[1, :, 0] = j
    return C


def pq_codes(v, special: bool = False) -> np.ndarray:
    """Intended values -> uint8 [n, 16].  Integer tables: v in [0, 65535], c0 = v >> 8, c1 = v & 255.  Special tables: v indexes SPECIALS."""
    v = np.asarray(v, dtype=np.int64)
    assert v.min(initial=0) >= 0 and v.max(initial=0) < (SPECIALS.shape[0] if special else 65536)
    codes = np.zeros((v.shape[0], PQ_M), np.uint8)
    codes[:, 0] = v if special else v >> 8
    if not special:
        codes[:, 1] = v & 255
    return codes


def pq_queries(pairs) -> np.ndarray:
    q = np.zeros((len(pairs), PQ_D), F32)
    for i, (a, b) in enumerate(pairs):
        q[i, 0], q[i, 1] = a, b
    return q


def pq_intended(v, pairs, special: bool = False) -> np.ndarray:
    """The score rows the harness is built to report, fp32 [Q, n]: +-(256 c0 + c1) and its parts, or +-SPECIALS[v] (with -0 read as +0: the
    contract's sum starts from +0)."""
    v = np.asarray(v, dtype=np.int64)
    if special:
        with np.errstate(all="ignore"):
            return np.stack([F32(0) + F32(a) * SPECIALS[v] for a, _ in pairs]).astype(F32)
    return np.stack([(a * 256 * (v >> 8) + b * (v & 255)).astype(F32) + F32(0) for a, b in pairs])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# flat and SQ8 harnesses (the band cases run on both)
# ---------------------------------------------------------------------------------------------------------------------------------------------
FLAT_D, SQ8_D = 32, 64
SQ8_TRAINED = np.array([0.0, 255.0], F32)            # QT_8bit_uniform: vmin, vdiff


def signs(nq: int) -> np.ndarray:
    """Alternating +e0, -e0."""
    return np.where(np.arange(nq) % 2 == 0, 1.0, -1.0).astype(F32)


def e0_queries(nq: int, d: int) -> np.ndarray:
    q = np.zeros((nq, d), F32)
    q[:, 0] = signs(nq)
    return q


def flat_rows(level) -> np.ndarray:
    x = np.zeros((len(level), FLAT_D), F32)
    x[:, 0] = level
    return x


def flat_intended(level, nq: int) -> np.ndarray:
    """fp32 [nq, n]: +-level (+0 where the level is 0: the exact score is an fp64 sum that starts from +0)."""
    return signs(nq)[:, None] * np.asarray(level, dtype=F32)[None, :] + F32(0)


def flat_pad_blocks(n: int) -> int:
    """Block maxima the flat score kernels write beyond the last valid row (they cover whole 256-row tiles)."""
    return -(-n // 256) * 2 - -(-n // SP_ROWS)


def sq8_codes(level) -> np.ndarray:
    c = np.zeros((len(level), SQ8_D), np.uint8)
    c[:, 0] = level
    return c


def sq8_expected_scores(level, nq: int) -> np.ndarray:
    """The contract's scores fp32 [nq, n] from sq8_yardstick.scores over the 256 possible code rows, gathered by level (rows with equal
    codes have equal scores)."""
    import sq8_yardstick as Y
    per_level = Y.scores(e0_queries(nq, SQ8_D), sq8_codes(np.arange(256)), SQ8_TRAINED)
    return np.ascontiguousarray(per_level[:, np.asarray(level, dtype=np.int64)])


def flat_eps(max_level: float = 255.0) -> float:
    """eps6 of select_rescore_query for a query +-e0 over rows of norm <= max_level, in fp64."""
    return (6 * FLAT_D + 8) * 2.0 ** -23 * 1.0 * max_level * 1.01


def sq8_eps() -> float:
    """eps(q) of k_sq8_prep for a query +-e0 under SQ8_TRAINED, its three terms evaluated in fp64 in the kernel's order."""
    q = np.zeros(SQ8_D, np.float64)
    q[0] = 1.0
    vmin, vdiff = float(SQ8_TRAINED[0]), float(SQ8_TRAINED[1])
    w = q * vdiff / 255.0
    wmax = float(np.max(np.abs(w).astype(F32) * F32(1.0000002)))
    scale = wmax / SQ8_NMAX
    n = np.clip(np.rint(w / scale), -SQ8_NMAX, SQ8_NMAX)
    err = np.abs(w - scale * n).sum()
    st = (np.abs(q) * (abs(vmin) + abs(vdiff))).sum()
    sa = np.abs(q).sum()
    return float(F32((128.0 * err + st * 2.0 ** -21 + sa * 3 * 2.0 ** -149) * 1.01) * F32(1.0000002))


BAND_EPS = {"flat": flat_eps, "sq8": sq8_eps}
LEVEL_GAP = 1.0          # adjacent levels are 1.0 apart in both harnesses
BAND_GAP = 0.5           # what band_form is given: any gap in (0, 1) selects the k-th level and everything above it


def band_gap_ok(harness: str) -> bool:
    """The band kth - 2 eps, taken at matrix scores that are themselves within eps of their level, stays inside the k-th level: the rows
    it rescores are exactly the rows at or above that level."""
    return 2.0 * BAND_EPS[harness]() * 1.01 < 0.5 * LEVEL_GAP


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _seed(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))      # (hash() of a str changes from process to process)


def _spread(rng, n: int, lo: int, hi: int) -> np.ndarray:
    """n values lo .. hi, each as often as any other (+-1), in random order."""
    return rng.permutation(lo + np.arange(n) % (hi - lo + 1))


def _tiny(N):
    def make():
        rng = np.random.default_rng(_seed("tiny") + N)
        return rng.permutation(np.arange(N) % SPECIALS.shape[0])
    return make


def _permutation(N):
    return lambda: np.random.default_rng(_seed("perm") + N).permutation(N)


def _top_level_on(N, n_top):
    """Value 60000 on n_top rows with every block holding at least one, distinct lower values elsewhere."""
    def make():
        rng = np.random.default_rng(_seed("cand-cap") + n_top)
        v = rng.permutation(N)
        nblk = -(-N // SP_ROWS)
        first = np.arange(nblk) * SP_ROWS + rng.integers(0, N - (nblk - 1) * SP_ROWS, nblk)       # one per block (the last block is partial)
        rest = rng.permutation(np.setdiff1d(np.arange(N), first))[:n_top - nblk]
        v[first] = 60000
        v[rest] = 60000
        return v
    return make


def _cand_overflow_distinct(N=20000, blocks=100, per_block=50):
    """`blocks` blocks hold `per_block` rows each above everything else, all distinct; one of the blocks holds the lowest of them, so its
    maximum -- the block threshold -- lies below all but per_block - 1 of the high rows."""
    def make():
        rng = np.random.default_rng(_seed("cand-overflow-distinct"))
        v = rng.permutation(N)
        which = rng.permutation(-(-N // SP_ROWS) - 1)[:blocks]                                    # (whole blocks only)
        high = 30000 + np.arange(blocks * per_block)
        high = np.concatenate([high[:per_block], rng.permutation(high[per_block:])])
        for j, b in enumerate(which):
            v[b * SP_ROWS + rng.permutation(SP_ROWS)[:per_block]] = high[j * per_block:(j + 1) * per_block]
        return v
    return make


def _tie_caps(g, neq, N=8192):
    """g distinct rows above, neq rows on one level, distinct lower rows elsewhere, all scattered."""
    def make():
        rng = np.random.default_rng(_seed("tie-caps") + 10000 * g + neq)
        v = rng.permutation(N)
        rows = rng.permutation(N)
        v[rows[:g]] = 40000 + rng.permutation(g)
        v[rows[g:g + neq]] = 30000
        return v
    return make


def _one_top_per_block(N, top, lo, hi):
    """`top` on one row of every block at a random offset, values lo .. hi elsewhere."""
    def make():
        rng = np.random.default_rng(_seed("block-cap") + N)
        v = _spread(rng, N, lo, hi)
        nblk = -(-N // SP_ROWS)
        off = rng.integers(0, SP_ROWS, nblk)
        off[-1] = rng.integers(0, N - (nblk - 1) * SP_ROWS)
        v[np.arange(nblk) * SP_ROWS + off] = top
        return v
    return make


def _special_order(N=5000):
    return lambda: np.random.default_rng(_seed("special-order")).integers(0, SPECIALS.shape[0], N)


def _case(name, make, ks, labels, special=False, id_base=0, counts=None):
    """labels: per k, the label of the FIRST query's row (256 c0 + c1, or +SPECIALS), None = whatever the model says.  counts: per k, the
    counts that must come with it."""
    return dict(name=name, make=make, ks=tuple(ks), labels=tuple(labels), special=special, id_base=id_base,
                queries=SPECIAL_QUERIES if special else PQ_QUERIES, counts=counts or {})


EX_S, EX_C = "exact/sorted", "exact/scan"
CASES = (
    [_case(f"tiny-{N}", _tiny(N), (1, 5, 400), ("direct",) * 3, special=True, id_base=7000) for N in (1, 127, 128, 129, 300)]
    + [_case("direct-cap-4096", _permutation(4096), (1, 100, 2048), ("direct",) * 3),
       _case("direct-cap-4097", _permutation(4097), (1, 100, 2048), ("fast", EX_S, EX_S)),          # 33 blocks < k
       _case("fast-20000", _permutation(20000), (1, 10, 157, 158), ("fast", "fast", "fast", EX_S),  # 157 blocks
             counts={157: dict(nb=157)}),
       _case("cand-cap-4096", _top_level_on(20000, 4096), (10,), ("fast",), counts={10: dict(nb=157, cand=4096)}),
       _case("cand-cap-4097", _top_level_on(20000, 4097), (10,), ("fast>cand>" + EX_C,), counts={10: dict(nb=157, cand=4097, neq=4097, need_eq=10)}),
       _case("cand-overflow-distinct", _cand_overflow_distinct(), (100,), ("fast>cand>" + EX_S,), counts={100: dict(nb=100, cand=4951, neq=1, need_eq=1)})]
    + [_case(f"tie-caps-{g}-{neq}", _tie_caps(g, neq), (1000,), (EX_S if neq <= 2048 else EX_C,), counts={1000: dict(neq=neq, need_eq=1000 - g)})
       for g, neq in ((500, 2047), (500, 2048), (500, 2049), (999, 2049), (0, 2049))]
    + [_case("block-cap-4096", _one_top_per_block(4096 * 128, 65535, 0, 59999), (10,), ("fast",), counts={10: dict(nb=4096, cand=4096)}),
       _case("block-cap-4097", _one_top_per_block(4097 * 128, 65535, 0, 59999), (10,), ("fast>blocks>" + EX_C,), counts={10: dict(nb=4097, neq=4097, need_eq=10)}),
       _case("block-cap-4097-partial", _one_top_per_block(4097 * 128 - 100, 65535, 0, 59999), (10,), ("fast>blocks>" + EX_C,),
             counts={10: dict(nb=4097, neq=4097, need_eq=10)}),
       _case("special-order", _special_order(), (2048,), (None,), special=True)]
)
CASE_BY_NAME = {c["name"]: c for c in CASES}


def case_rows(case):
    """-> (v, intended fp32 [Q, n]) of a PQ case."""
    v = case["make"]()
    return v, pq_intended(v, case["queries"], case["special"])


# ---- band cases: integer levels 1 .. 255, run on the flat and the SQ8 harness; forms[i] is the band form of query +e0 (i = 0) and -e0 (i = 1)
def _band_top_on(N, n_top):
    """Level 250 on n_top rows, levels 1 .. 200 elsewhere (so the band of -e0 is the few rows of level 1)."""
    def make():
        rng = np.random.default_rng(_seed("band-cap") + n_top)
        lv = _spread(rng, N, 1, 200)
        lv[rng.permutation(N)[:n_top]] = 250
        return lv
    return make


def _band_merge(N=20000, n_tie=5000):
    """Levels 201 .. 250 on one row each, five of them in each of ten different 2048-row windows; n_tie rows on level 200; 1 .. 199 elsewhere."""
    def make():
        rng = np.random.default_rng(_seed("band-merge"))
        lv = _spread(rng, N, 1, 199)
        windows = rng.permutation(-(-N // SEL_MAXK))[:10]
        rows = np.concatenate([w * SEL_MAXK + rng.permutation(min(SEL_MAXK, N - w * SEL_MAXK))[:5] for w in windows])
        lv[rng.permutation(np.setdiff1d(np.arange(N), rows))[:n_tie]] = 200
        lv[rows] = 201 + rng.permutation(50)
        return lv
    return make


def _band_maxk(N=20000, above=1000, n_tie=3500):
    def make():
        rng = np.random.default_rng(_seed("band-maxk"))
        lv = _spread(rng, N, 1, 199)
        rows = rng.permutation(N)
        lv[rows[:above]] = _spread(rng, above, 201, 250)
        lv[rows[above:above + n_tie]] = 200
        return lv
    return make


def _band_case(name, make, k, forms):
    return dict(name=name, make=make, k=k, forms=tuple(forms))


BAND_CASES = [
    _band_case("band-cap-4096", _band_top_on(20000, 4096), 10, ("in-list", "in-list")),
    _band_case("band-cap-4097", _band_top_on(20000, 4097), 10, ("stream/rows", "in-list")),
    _band_case("band-direct", lambda: np.full(4097, 7, np.int64), 10, ("stream/rows", "stream/rows")),       # 33 blocks listed, 4097 rows in the band
    _band_case("band-merge", _band_merge(), 100, ("stream/rows", "in-list")),
    _band_case("band-maxk", _band_maxk(), 2048, ("stream/rows", "in-list")),
    _band_case("band-blocks-4096", _one_top_per_block(4096 * 128, 250, 1, 200), 10, ("in-list", "in-list")),
    _band_case("band-blocks-4097", _one_top_per_block(4097 * 128, 250, 1, 200), 10, ("stream/blocks", "in-list")),
]
BAND_BY_NAME = {c["name"]: c for c in BAND_CASES}
FLAT_BATCHES = (2, 40)       # the score matrix comes from another kernel above 32 queries
SQ8_BATCH = 2


def band_forms(level, k: int, nq: int):
    """The band form of each of nq alternating queries over the levels."""
    lv = np.asarray(level, dtype=F32)
    two = [band_form(lv, k, BAND_GAP), band_form(-lv, k, BAND_GAP)]
    return [two[i % 2] for i in range(nq)]
