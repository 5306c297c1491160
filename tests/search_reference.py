"""A plain fp64 model of the filter stages of the bounded inner-product search (lrx_search_bounded.h), and the cases the stage tests
run.  numpy only: no GPU, no library call, no oracle binary.  test_search_reference_host.py checks the model and the preconditions of every
case on the CPU; test_gpu_search_stages.py compares what each stage left in the workspace (FlatIPIndex.last_chunk_state) with it.

Notation (q one query, x_r one row, D the width; q~ = fp16(q), x~ = fp16(x), round-to-nearest-even, saturating at +-65504):
  s64   = q . x_r in fp64                      the exact score (for the fp16-SQ index the codes ARE the rows: x := x~)
  st64  = q~ . x~_r in fp64                    what the filter would compute without accumulation error
  acc   = (D + 32) 2^-23 |q~| |x~_r|           the design's accumulation term: |s~_gpu - st64| <= acc
  eps   = |q - q~| R + |q~| E + (D + 32) 2^-23 |q~| R          (ROWS_F16T: |q - q~| R16 + (D + 32) 2^-23 |q~| R16, R16 = R + E)
Every slack below is one of these terms or the rounding of an fp32 number; none is fitted to what the library returns."""
import math

import numpy as np

REF_CAND = 4096          # band capacity of a query over all parts of the refine step (lrx_search_bounded.h)
SEL_CAND = 4096
FILTER_SCORE_FREE, FUSED_ALWAYS, FUSED_NEVER = 2, 4, 8


def f16_sat(a):
    """fp16(a), round-to-nearest-even, saturating at +-65504 (f2h_sat), as fp64."""
    return np.clip(np.asarray(a, np.float32), np.float32(-65504), np.float32(65504)).astype(np.float16).astype(np.float64)


def host_bounds(X):
    """{R, E} = {max |x_row|, max |x_row - fp16(x_row)|} in fp64, rounded UP to fp32: what an index maintains, to the last bits (the host
    tests' stand-in for FlatIPIndex._bounds; the GPU tests read the index's own pair)."""
    X64 = np.asarray(X, np.float64)
    R = np.sqrt((X64 * X64).sum(1)).max()
    d = X64 - f16_sat(X)
    E = np.sqrt((d * d).sum(1)).max()
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf))) if float(np.float32(v)) < v else float(np.float32(v))
    return up(R), up(E)


def expected_plan(N, D, Q, k, shadow, flags, cus=256):
    """plan_chunk (lrx_search.hip) for one chunk of Q queries on a device of `cus` compute units, for the shapes the stage tests use (rows < 2^31,
    no dev-build knobs): the facts last_chunk_state() reports.  The GPU tests assert that the library's plan equals this one, so the host
    tests' preconditions are the preconditions of what runs."""
    mode = flags & 3
    fused_pref = 0 if flags & FUSED_NEVER else (1 if flags & FUSED_ALWAYS else -1)
    shadow = bool(shadow) and D % 64 == 0
    gemm = shadow and Q > 128 and D >= 1024 and mode != 3
    rb = 256 if gemm else (128 if shadow else 256)
    cap = 65536
    while cap < 64 * k:
        cap *= 2
    nwg = -(-N // rb)
    bpc = nwg // cus
    ss_fill = 2 if bpc < 6 else (4 if bpc < 12 else (8 if bpc < 24 else 32))
    ss_hits = int(0.25 * 1.41 * math.sqrt(N / k))
    ss_list = cap // (3 * k)
    ss_lim = min(ss_hits, ss_list, ss_fill)
    ss = 2
    while ss * 2 <= ss_lim:
        ss *= 2
    ss = min(ss, 32)
    fused_rule = Q <= 16 and D >= 512 and k <= 256 and nwg <= 8 * cus
    fused_ok = fused_pref != 0 and (fused_rule or fused_pref == 1) and shadow and not gemm and Q <= 128 and D % 256 == 0
    if fused_ok:
        lim = max(2, min(64, min(ss_hits, ss_list)))
        one_round = -(-nwg // cus)
        ss = 2 if one_round < 2 else min(one_round, lim)
    while ss > 2 and (-(-nwg // ss) - 1) * rb < 2 * k:
        ss = ss - 1 if fused_ok else ss >> 1
    nsamp = -(-nwg // ss)
    if nsamp * (rb // 16) < k:
        fused_ok = False
    feasible = (nsamp - 1) * rb >= 2 * k and nwg - nsamp >= 1 and D % 4 == 0 and (shadow or Q > 32)
    if not feasible:
        gemm = False
    emit = feasible and mode != 1 and (mode >= 2 or N >= 16384)
    nsplit = 4 if Q * 4 <= cus else (2 if Q * 2 <= cus else 1)
    return dict(emit=emit, fused=emit and fused_ok and not gemm, gemm=emit and gemm, ss=ss, rb=rb, cap=cap, nsplit=nsplit if emit else 4,
                group_rows=16 if shadow else 128, nsamp=nsamp)


def eps_upper_factor(D, codes_are_rows=False):
    """How far above eps_ref the library's fp32 eps may lie -- from the safety factors written in query_eps_block, nothing measured:
         eps_gpu = fl[(sqrt(B) R + sqrt(A) (E + accum R 1.01)) 1.0001] + 1e-30,   A = fl(sum fp16(q_i)^2), B = fl(sum (q_i - fp16(q_i))^2)
      * 1.01 multiplies the accumulation term only; as a factor on the whole sum it is an upper bound (all terms are >= 0);
      * 1.0001 multiplies everything; ROWS_F16T has another 1.0001 on R16;
      * A and B are fp32 sums of D fp32 squares (q_i - fp16(q_i) is exact in fp32): each square and each of the D - 1 additions, in whatever
        order the waves reduce them, rounds by at most 2^-24 relative, all terms >= 0, so fl(A) = A (1 + t), |t| <= D 2^-24 (to first order);
        the square root halves that and adds its own rounding: sqrt factor <= 1 + D 2^-25 + 2^-24;
      * at most 8 further fp32 operations (products, sums, the (D + 32) 2^-23 constant) of 2^-24 each.
    The same D 2^-25 + 9 2^-24 can act downwards: the LOWER check eps_ref <= eps_gpu holds through the 1.0001 as long as that is below 1e-4
    (D <= 3300; the stage tests stop at D = 1024)."""
    f = 1.01 * 1.0001 * (1.0001 if codes_are_rows else 1.0)
    return f * (1.0 + D * 2.0 ** -25 + 9 * 2.0 ** -24)


class StageModel:
    """The fp64 model of one chunk: q [Q, D] fp32, X [N, D] fp32 rows as added to the index, bounds = (R, E) as the index holds them, k, and
    the plan facts (ss, rb, cap, group_rows) of last_chunk_state() / expected_plan().  codes_are_rows: the fp16-SQ index (ROWS_F16T)."""

    def __init__(self, q, X, bounds, k, plan, codes_are_rows=False):
        q = np.asarray(q, np.float32)
        X = np.asarray(X, np.float32)
        self.Q, self.D = q.shape
        self.N = X.shape[0]
        self.k, self.plan, self.codes_are_rows = k, plan, codes_are_rows
        qt, xt = f16_sat(q), f16_sat(X)
        q64 = q.astype(np.float64)
        self.s64 = q64 @ (xt if codes_are_rows else X.astype(np.float64)).T
        self.st64 = qt @ xt.T
        self.qn = np.sqrt((qt * qt).sum(1))
        dq = q64 - qt
        self.dqn = np.sqrt((dq * dq).sum(1))
        self.xn = np.sqrt((xt * xt).sum(1))
        self.c_acc = (self.D + 32) * 2.0 ** -23
        self.acc = self.c_acc * self.qn[:, None] * self.xn[None, :]
        R, E = float(bounds[0]), float(bounds[1])
        if not E > 0.0:                                  # "not measured": query_eps_block's own bound of E from R
            E = R * 2.0 ** -11 + math.sqrt(self.D) * 2.0 ** -25 if R <= 65504.0 else R
        if codes_are_rows:
            R16 = R + E
            self.eps_ref = self.dqn * R16 + self.c_acc * self.qn * R16
        else:
            self.eps_ref = self.dqn * R + self.qn * E + self.c_acc * self.qn * R
        self.eps_factor = eps_upper_factor(self.D, codes_are_rows)
        self.eps_hi = self.eps_ref * self.eps_factor + 1e-30
        # sample rows: unit t of rb rows for every t % ss == 0
        rows = np.arange(self.N)
        self.in_sample = (rows // plan["rb"]) % plan["ss"] == 0
        self.sample_rows = rows[self.in_sample]
        self._thr_bounds = None

    # -- T' ------------------------------------------------------------------------------------------------------------------------------
    def threshold_grouping(self):
        """Rows per group of the maxima whose k-th largest is T' (sample_threshold_query): 128-row blocks when the sample has >= 8 k of them
        (and at most 2 SEL_CAND), 16-row groups when there are >= k, else 1 = the scores themselves; without a shadow (128-row block maxima
        only prune the exact selection) always 1."""
        nblk_s = self.plan["nsamp"] * self.plan["rb"] // 128
        if self.plan["group_rows"] != 16:
            return 1
        if nblk_s >= 8 * self.k and nblk_s <= 2 * SEL_CAND:
            return 128
        return 16 if nblk_s * 8 >= self.k else 1

    def _kth_largest(self, a, k):
        return np.partition(a, a.shape[1] - k, axis=1)[:, a.shape[1] - k]

    def threshold_bounds(self):
        """(lo, hi) [Q] for T' = thr + 2 eps.  hi: the k-th largest sample score (k sample rows reach T' whatever the grouping; the row-exact
        branch of clumpy samples raises T' to exactly that).  lo: the k-th largest group maximum.  Both from st64, widened by the largest acc of
        the query over the sample rows.  (The caller adds the rounding of the stored fp32 thr.)"""
        if self._thr_bounds is None:
            sr = self.sample_rows
            st = self.st64[:, sr]
            slack = self.acc[:, sr].max(1)
            hi = self._kth_largest(st, self.k)
            g = self.threshold_grouping()
            if g == 1:
                lo = hi.copy()
            else:
                gid = sr // g                              # sample units are whole, aligned groups of rows: a group never mixes units
                starts = np.flatnonzero(np.r_[True, gid[1:] != gid[:-1]])
                gmax = np.maximum.reduceat(st, starts, axis=1)
                assert gmax.shape[1] >= self.k
                lo = self._kth_largest(gmax, self.k)
            self._thr_bounds = (lo - slack, hi + slack)
        return self._thr_bounds

    # -- lists ---------------------------------------------------------------------------------------------------------------------------
    def list_must(self, thr):
        """(must be listed, must not be listed) [Q, N] for the stored thr [Q]: st64 >= thr + acc / st64 < thr - acc."""
        thr = np.asarray(thr, np.float64)[:, None]
        return self.st64 >= thr + self.acc, self.st64 < thr - self.acc

    def list_count_bounds(self, thr_lo, thr_hi, thr_sample_lo=None):
        """(lower, upper) [Q] list counts for a stored thr anywhere in [thr_lo, thr_hi]; sample rows may have entered at the (lower) group
        threshold thr_sample_lo (the row-exact branch keeps them)."""
        lo = (self.st64 - self.acc >= np.asarray(thr_hi)[:, None]).sum(1)
        t = np.repeat(np.asarray(thr_lo, np.float64)[:, None], self.N, axis=1)
        if thr_sample_lo is not None:
            t[:, self.in_sample] = np.minimum(t[:, self.in_sample], np.asarray(thr_sample_lo, np.float64)[:, None])
        hi = (self.st64 + self.acc >= t).sum(1)
        return lo, hi

    # -- band ----------------------------------------------------------------------------------------------------------------------------
    def band_count_bounds(self, eps_lo, eps_hi):
        """(lower, upper) [Q] counts of the band {s~ >= kth~ - 2 eps}, kth~ = k-th largest s~ of the shard, for an eps in [eps_lo, eps_hi]:
        s~ lies within acc of st64, so kth~ lies between the k-th largest of st64 - acc and of st64 + acc."""
        kth_lo = self._kth_largest(self.st64 - self.acc, self.k)
        kth_hi = self._kth_largest(self.st64 + self.acc, self.k)
        lower = (self.st64 - self.acc >= (kth_hi - 2.0 * np.asarray(eps_lo))[:, None]).sum(1)
        upper = (self.st64 + self.acc >= (kth_lo - 2.0 * np.asarray(eps_hi))[:, None]).sum(1)
        return lower, upper

    # -- what the host tests check before any GPU run ----------------------------------------------------------------------------------------
    def predictions(self, band_safe=REF_CAND // 4):
        """Without any GPU value: eps in [eps_ref, eps_hi], T' in threshold_bounds() -> ranges of the list and band counts per query, and the
        verdict per query: 'benign' (upper band <= band_safe = 1024: the refine step deals the list entries round-robin to nsplit parts of
        4096 / nsplit band slots each, so in the worst case one part gets the whole band -- 1024 is safe for nsplit = 1, 2 and 4; upper list
        <= cap / 2), 'overflow' (lower band > 4096: some part overflows whatever the split; or lower list > cap), or 'undecided'."""
        t_lo, t_hi = self.threshold_bounds()
        # (the stored thr = fl(T' - 2 eps): half an ulp of rounding, 2^-24 relative)
        thr_lo = t_lo - 2.0 * self.eps_hi
        thr_hi = t_hi - 2.0 * self.eps_ref
        thr_lo -= np.abs(thr_lo) * 2.0 ** -24
        thr_hi += np.abs(thr_hi) * 2.0 ** -24
        list_lo, list_hi = self.list_count_bounds(thr_lo, thr_hi)
        band_lo, band_hi = self.band_count_bounds(self.eps_ref, self.eps_hi)
        cap = self.plan["cap"]
        benign = (band_hi <= band_safe) & (list_hi <= cap // 2)
        overflow = (band_lo > REF_CAND) | (list_lo > cap)
        verdict = np.where(benign, "benign", np.where(overflow, "overflow", "undecided"))
        return dict(list_lo=list_lo, list_hi=list_hi, band_lo=band_lo, band_hi=band_hi, verdict=verdict)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _unit(a):
    a = np.asarray(a, np.float64)
    return (a / np.sqrt((a * a).sum(-1, keepdims=True))).astype(np.float32)


def _random_case(seed, N, D, Q, mixed):
    rng = np.random.default_rng(seed)
    X = _unit(rng.standard_normal((N, D)))
    if mixed:
        X = X * rng.uniform(0.05, 3.0, size=(N, 1)).astype(np.float32)
    q = _unit(rng.standard_normal((Q, D))) * np.float32(1.7)
    return X, q


def _band_overflow_case(seed, N, D, Q, ncopy=5000):
    """ncopy exact copies of one row, spread over the shard; the first half of the queries point at it (the copies fill the top-k and the band:
    more than 4096 band rows), the others are random (the copies score far below their top-k)."""
    X, q = _random_case(seed, N, D, Q, False)
    rng = np.random.default_rng(seed + 1)
    where = rng.permutation(N)[:ncopy]
    v = X[where[0]].copy()
    X[where] = v
    for j in range(Q // 2):
        q[j] = _unit(v.astype(np.float64) + 0.05 * rng.standard_normal(D)) * np.float32(1.7)
    return X, q


def _list_overflow_case(seed, N, D, Q, ncopy=68000):
    """ncopy near-copies of one row v (v + 1e-6 noise: alike within a fraction of eps) at random places among random rows; the first half of
    the queries point at v (more hits than the 64 Ki list holds), the others are orthogonal to v (the cluster scores ~0, far below their top-k)."""
    rng = np.random.default_rng(seed)
    X = _unit(rng.standard_normal((N, D)))
    v = X[0].astype(np.float64)
    where = rng.permutation(N)[:ncopy]
    X[where] = (v[None, :] + 1e-6 * rng.standard_normal((ncopy, D))).astype(np.float32)
    q = np.empty((Q, D), np.float32)
    for j in range(Q):
        r = rng.standard_normal(D)
        if j < Q // 2:
            q[j] = _unit(v + 0.05 * r) * np.float32(1.7)
        else:
            q[j] = _unit(r - (r @ v) * v / (v @ v)) * np.float32(1.7)
    return X, q


def _beyond_fp16_case(seed, N, D, Q):
    """Unit rows, one of them with an element of 1e5: its shadow saturates, E ~ 3.4e4, eps ~ 6e4 -- the band is useless, every query is
    flagged; every score stays finite."""
    X, q = _random_case(seed, N, D, Q, False)
    X[N // 3, 5] = np.float32(1e5)
    return X, q


def _clustered_case(seed, N, D, Q, csize=128):
    """Rows stored cluster by cluster (clusters of `csize` contiguous rows around a random centre), queries near cluster centres: the rows of a
    16-row group score alike; for a query whose cluster lies in the sample the k-th group maximum is far below the k-th sample score and the
    row-exact T' branch has to repair it."""
    rng = np.random.default_rng(seed)
    nc = N // csize
    C = _unit(rng.standard_normal((nc, D))).astype(np.float64)
    X = _unit(np.repeat(C, csize, axis=0) + 0.5 / math.sqrt(D) * rng.standard_normal((N, D)))
    perm = rng.permutation(nc // 2)                   # first half of the queries: clusters inside the sample (even 128-row units), the rest outside
    pick = np.r_[2 * perm[:Q // 2], 2 * perm[Q // 2:Q] + 1]
    q = _unit(C[pick] + 0.3 / math.sqrt(D) * rng.standard_normal((Q, D))) * np.float32(1.7)
    return X, q


_SF, _CHAIN, _FUSED = FILTER_SCORE_FREE, FILTER_SCORE_FREE | FUSED_NEVER, FILTER_SCORE_FREE | FUSED_ALWAYS
# name -> dict(N, D, Q, k, make, flags, shadow, index, kind); "benign": no query may overflow; "overflow": the listed queries must, the others must not
CASES = {
    "wg_per_block_3_slices_ragged":  dict(N=4301, D=192, Q=5, k=3, seed=101, mixed=True),
    "q_resident_block_max_thr":      dict(N=5000, D=256, Q=17, k=1, seed=102, mixed=False),
    "persistent_7_tiles_odd_blocks": dict(N=6017, D=512, Q=100, k=50, seed=103, mixed=True),
    "tiles_9_to_16_below_gemm":      dict(N=8000, D=256, Q=200, k=10, seed=104, mixed=False),
    "gemm_one_n_tile":               dict(N=8200, D=1024, Q=130, k=20, seed=105, mixed=True),
    "gemm_wide_ragged_n_tile":       dict(N=8200, D=1024, Q=300, k=5, seed=106, mixed=False),
    "fused_1_tile":                  dict(N=9000, D=512, Q=16, k=10, seed=107, mixed=True, flags=_FUSED),
    "fused_7_tiles":                 dict(N=9000, D=512, Q=100, k=10, seed=108, mixed=False, flags=_FUSED),
    "wave_lists_flushed":            dict(N=20000, D=256, Q=256, k=1000, seed=109, mixed=False),
    "no_shadow_dim_96":              dict(N=6000, D=96, Q=48, k=10, seed=110, mixed=True),
    "no_shadow_switched_off":        dict(N=6000, D=128, Q=48, k=10, seed=111, mixed=False, shadow=False),
    "sq_fp16_codes":                 dict(N=6000, D=128, Q=33, k=10, seed=112, mixed=True, index="sq"),
    "sorted_scores_thr":             dict(N=4200, D=64, Q=3, k=300, seed=113, mixed=False),
    "band_overflow_copies":          dict(N=12000, D=64, Q=4, k=10, seed=114, make=_band_overflow_case, overflow=(0, 1)),
    "list_overflow_near_copies":     dict(N=70000, D=64, Q=4, k=5, seed=115, make=_list_overflow_case, overflow=(0, 1)),
    "row_beyond_fp16":               dict(N=5000, D=128, Q=6, k=5, seed=116, make=_beyond_fp16_case, overflow=(0, 1, 2, 3, 4, 5)),
    "clustered_row_exact_thr":       dict(N=16384, D=256, Q=8, k=20, seed=117, make=_clustered_case),
}


def case_spec(name):
    c = dict(flags=_CHAIN, shadow=True, index="flat", overflow=(), make=None, mixed=False)
    c.update(CASES[name])
    c["has_shadow"] = c["index"] == "sq" or (c["shadow"] and c["D"] % 64 == 0)
    return c


_DATA = {}


def case_data(name):
    """(X, q) of a case: built once per process and shared (do not modify)."""
    if name not in _DATA:
        c = case_spec(name)
        X, q = c["make"](c["seed"], c["N"], c["D"], c["Q"]) if c["make"] else _random_case(c["seed"], c["N"], c["D"], c["Q"], c["mixed"])
        X.setflags(write=False)
        q.setflags(write=False)
        _DATA[name] = (X, q)
    return _DATA[name]


def adversarial_midpoint_case():
    """The rows and queries of test_gpu_search_emit.py::test_adversarial_fp16_rounding_midpoints: elements just below / above fp16 rounding
    midpoints, so that |s64 - st64| comes as close to the bound as rounding allows."""
    rng = np.random.default_rng(5)
    N, D, Q = 40000, 128, 48
    X = _unit32(rng.standard_normal((N, D)).astype(np.float32)) * np.float32(0.9)
    w = np.float32(1 + 2.0 ** -11 - 2.0 ** -15)
    a = np.float32(1 + 2.0 ** -11 + 2.0 ** -15)
    b = np.float32(1 - 2.0 ** -12 + 2.0 ** -15)
    q = np.abs(_unit32(rng.standard_normal((Q, D)).astype(np.float32)))
    q[:Q // 2] = w * np.float32(2.0) ** rng.integers(-3, 1, size=(Q // 2, D)).astype(np.float32)
    s = np.float32(0.9 / np.sqrt(D))
    half = np.arange(D) % 2 == 0
    for j in range(Q):
        for t in range(12):
            X[j * 40 + t] = s * w * np.float32(1 - 1.2e-5 * t) * np.float32(1 - 1e-3 * j)
        for t in range(12, 30):
            X[j * 40 + t] = s * np.where(half, a, b).astype(np.float32) * np.float32(1 - 6e-7 * t) * np.float32(1 - 1e-3 * j)
    return X, q


def _unit32(a):
    return a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-12)
