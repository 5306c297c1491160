"""fp64 model of the 8-bit scalar-quantised index's filter stages (lrx_sq8_ip_search: k_sq8_prep, k_sq8_scan) in numpy, on top of
sq8_yardstick.py, and the crafted cases of test_gpu_sq8_stages.py.  test_sq8_stage_reference_host.py checks every case's preconditions on
the model alone; the GPU test compares what each stage left in the workspace (SQ8Index.last_chunk_state) with it.

The model follows the kernel's operation order where the order decides a bit (w, wmax, scale, the digits) and sums in fp64 where it does
not (bias, the terms of eps): the GPU test allows those sums their fp64 rounding only."""
import numpy as np

import sq8_yardstick as Y

F32, F64 = np.float32, np.float64
NMAX = 16319                        # |128 hi + lo| <= 127 * 128 + 63
UP = F32(1.0000002)                 # the kernel's fp32 round-up factor (1 + 2^-22)
EPS_SAFETY = 1.01                   # the factor on the fp64 sum of eps's terms (k_sq8_prep's header comment)


def split(trained, d):
    return Y._split(trained, d)


def prep_w(q, trained):
    """w = q vdiff / 255 in fp64, the kernel's order: (q * vdiff) / 255."""
    q = np.asarray(q, F32)
    _, vdiff = split(trained, q.shape[1])
    return q.astype(F64) * vdiff.astype(F64) / 255.0


def prep_scale(w):
    """wmax = max_i fl32(|w_i|) * 1.0000002f (fp32, rounded up), scale = wmax / 16319 in fp64."""
    with np.errstate(all="ignore"):
        wmax = (np.abs(w).astype(F32) * UP).astype(F32).max(axis=1, initial=F32(0))
    return wmax.astype(F64) / float(NMAX)


def digits(w, scale):
    """n = clip(rint(w / scale), +-16319) (0 where scale = 0), hi = (n + 64) >> 7, lo = n - 128 hi."""
    sc = np.where(scale > 0, scale, 1.0)[:, None]
    n = np.where(scale[:, None] > 0, np.rint(w / sc), 0.0)
    n = np.clip(n, -NMAX, NMAX).astype(np.int64)
    hi = (n + 64) >> 7
    return n, hi, n - 128 * hi


def prep_bias(q, trained, w):
    vmin, _ = split(trained, q.shape[1])
    return (q.astype(F64) * vmin.astype(F64)).sum(1) + 128.5 * w.sum(1)


def bias_tolerance(q, trained, w):
    """d 2^-52 (sum |q vmin| + 128.5 sum |w|): what two fp64 sums of d terms in any order may differ by."""
    vmin, _ = split(trained, q.shape[1])
    return q.shape[1] * 2.0 ** -52 * (np.abs(q.astype(F64) * vmin.astype(F64)).sum(1) + 128.5 * np.abs(w).sum(1))


def eps_terms(q, trained, w, scale, n):
    """The three terms of the bound in k_sq8_prep's header comment, each [Q] fp64:
       128 sum |w - scale n|,   2^-21 sum |q| (|vmin| + |vdiff|),   3 2^-149 sum |q|."""
    vmin, vdiff = split(trained, q.shape[1])
    aq = np.abs(q.astype(F64))
    quant = 128.0 * np.abs(w - scale[:, None] * n).sum(1)
    decode = 2.0 ** -21 * (aq * (np.abs(vmin.astype(F64)) + np.abs(vdiff.astype(F64)))).sum(1)
    tiny = 3 * 2.0 ** -149 * aq.sum(1)
    return quant, decode, tiny


def eps_of(terms):
    """eps = fl32(1.01 (t1 + t2 + t3)) * 1.0000002f, as fp32."""
    total = (terms[0] + terms[1] + terms[2]) * EPS_SAFETY
    return (total.astype(F32) * UP).astype(F32)


def centred(codes):
    return np.asarray(codes).astype(F64) - 128.0


def filter_scores(scale, n, bias, cm):
    """v = scale sum_i n_i (c_i - 128) + bias, the integer sums exact (|sum| < 2^31, carried in fp64) -> (v, isum) [Q, rows]."""
    isum = n.astype(F64) @ cm.T
    return scale[:, None] * isum + bias[:, None], isum


def exact_scores(q, codes, trained):
    """s64 = q64 . decode(codes)64 [Q, rows]."""
    return q.astype(F64) @ Y.decode(codes, trained).astype(F64).T


class StageModel:
    """Everything the stages of one query chunk should hold, for queries q [Q, d] (fp32) over `codes` [rows, d] under `trained`."""

    def __init__(self, q, codes, trained):
        q = np.asarray(q, F32)
        self.q, self.codes, self.trained = q, codes, trained
        self.Q, self.d = q.shape
        self.rows = codes.shape[0]
        self.w = prep_w(q, trained)
        self.scale = prep_scale(self.w)
        self.n, self.hi, self.lo = digits(self.w, self.scale)
        self.rho = self.w - self.scale[:, None] * self.n
        self.bias = prep_bias(q, trained, self.w)
        self.terms = eps_terms(q, trained, self.w, self.scale, self.n)
        self.eps_ref = eps_of(self.terms)
        cm = centred(codes)
        self.v, self.isum = filter_scores(self.scale, self.n, self.bias, cm)
        self.s64 = exact_scores(q, codes, trained)
        self.s = self.s64.astype(F32)                    # (= sq8_yardstick.scores)

    def ratio(self):
        """|v - s64| / eps_ref per pair (0 where both vanish)."""
        err = np.abs(self.v - self.s64)
        e = self.eps_ref.astype(F64)[:, None]
        return np.where(err > 0, err / np.where(e > 0, e, np.finfo(F64).tiny), 0.0)

    def kth_filter(self, k):
        return np.sort(self.v, axis=1)[:, -min(k, self.rows)]


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
def _trained(rng, d, uniform, lo=0.5, hi=1.5):
    """Ranges as a training on rows of size ~1 leaves them: vmin < 0 < vmin + vdiff, both of the order of 3 / sqrt(d)."""
    m = 1 if uniform else d
    a, b = rng.uniform(lo, hi, m), rng.uniform(lo, hi, m)
    s = 3.0 / np.sqrt(d)
    return np.concatenate([-a * s, (a + b) * s]).astype(F32)


def _gauss(rng, Q, d, kind="gauss"):
    q = rng.standard_normal((Q, d))
    if kind == "unit":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    if kind == "spike":
        q[:, 3] = 200.0
    return q.astype(F32)


def _random_case(c, rng):
    d, n, Q = c["d"], c["n"], c["Q"]
    return _trained(rng, d, c["uniform"]), rng.integers(0, 256, (n, d), dtype=np.uint8), _gauss(rng, Q, d)


def aligned_rows(q, trained):
    """Rows A and B of every query -> uint8 [2 Q, d] (A_0, B_0, A_1, ...): A has code 255 where rho = w - scale n > 0 and 0 elsewhere, B is
    its complement, so v - s = -sum rho (c - 128) is -(127 sum_{rho > 0} |rho| + 128 sum_{rho <= 0} |rho|) for A and +(128 sum_{rho > 0} |rho|
    + 127 sum_{rho <= 0} |rho|) for B: the first term of eps, 128 sum |rho|, nearly whole."""
    w = prep_w(q, trained)
    scale = prep_scale(w)
    n, _, _ = digits(w, scale)
    a = np.where(w - scale[:, None] * n > 0, 255, 0).astype(np.uint8)
    out = np.empty((2 * q.shape[0], q.shape[1]), np.uint8)
    out[0::2], out[1::2] = a, 255 - a
    return out


def _aligned_case(c, rng):
    d, n, uniform = c["d"], c["n"], c["uniform"]
    trained = _trained(rng, d, uniform)
    q = np.concatenate([_gauss(rng, 2, d, "unit"), _gauss(rng, 2, d, "gauss") * F32(3), _gauss(rng, 2, d, "spike")])
    ab = aligned_rows(q, trained)
    return trained, np.concatenate([ab, rng.integers(0, 256, (n - ab.shape[0], d), dtype=np.uint8)]), q


def _offset_case(c, rng):
    d, n, Q = c["d"], c["n"], c["Q"]
    vmin = rng.choice([-1.0, 1.0], d) * rng.uniform(900, 1100, d)
    vdiff = rng.uniform(0.5e-3, 2e-3, d)
    return np.concatenate([vmin, vdiff]).astype(F32), rng.integers(0, 256, (n, d), dtype=np.uint8), _gauss(rng, Q, d)


def _subnormal_case(c, rng):
    """Three columns of four have a subnormal vdiff in [2^-140, 2^-128] and queries of the order of 2^110, every fourth a small normal one in
    [2^-126, 2^-120] and queries 2^-12 of that, vmin = -u vdiff: t * vdiff and vmin + m of the decode are subnormal or barely normal, the
    scores are normal (~2^-16), and 3 2^-149 sum |q| is several per cent of eps (the first term is 32 d max |w| / 16319: that share needs
    max |q vdiff| <= ~2^-128 mean |q|)."""
    d, n, Q = c["d"], c["n"], c["Q"]
    normal = np.arange(d) % 4 == 3
    vdiff = (2.0 ** np.where(normal, rng.uniform(-126, -120, d), rng.uniform(-140, -128, d))).astype(F32)
    vmin = (-rng.uniform(0, 1, d) * vdiff.astype(F64)).astype(F32)
    q = (rng.standard_normal((Q, d)) * np.where(normal, 2.0 ** 98, 2.0 ** 110)).astype(F32)
    return np.concatenate([vmin, vdiff]), rng.integers(0, 256, (n, d), dtype=np.uint8), q


def _const_cols_case(c, rng):
    trained, codes, q = _random_case(c, rng)
    trained[c["d"] + np.arange(0, c["d"], 3)] = 0            # vdiff = 0: the decoded value is vmin whatever the code (the codes stay random)
    return trained, codes, q


def _zero_query_case(c, rng):
    trained, codes, q = _random_case(c, rng)
    q[2] = 0
    return trained, codes, q


def _nonfinite_case(c, rng):
    trained, codes, q = _random_case(c, rng)
    q[1, 7] = np.nan
    q[4, 40] = np.inf
    return trained, codes, q


BAND_K = 10
BAND_SUPPORT = 64                    # dimensions per query: the queries of band_edge have disjoint supports, so each is a problem of its own


def _band_edge_case(c, rng):
    """Per query j (non-negative, on its own 64 dimensions; w > 0 there): row U_j = row A tuned so that its exact score lies just above those
    of k rows B_j,m = row B lowered by one code on a middling dimension each.  The filter sees U about eps too low and the others about eps
    too high, so U -- the exact top-1 -- lies almost 2 eps below the k-th filter score.  Every other row holds small codes on every dimension: far
    below for every query (rows crafted for another query hold 0 on this query's dimensions).
    Magnitudes n = w / scale per support: 8 large (3000 .. 16319), 32 middling (40 .. 300), 24 small (4 .. 30), so that a change of one code
    moves the exact score by 0.002 .. 8 eps."""
    d, n_rows, uniform = c["d"], c["n"], c["uniform"]
    Q = d // BAND_SUPPORT
    trained = _trained(rng, d, uniform)
    _, vdiff = split(trained, d)
    q = np.zeros((Q, d), F32)
    for j in range(Q):
        sup = np.arange(j * BAND_SUPPORT, (j + 1) * BAND_SUPPORT)
        mag = np.concatenate([[16319.0], np.exp(rng.uniform(np.log(3000), np.log(16000), 7)), np.exp(rng.uniform(np.log(40), np.log(300), 32)),
                              np.exp(rng.uniform(np.log(4), np.log(30), 24))])
        mag = np.rint(mag) + np.where(np.arange(BAND_SUPPORT) == 0, 0.0, rng.uniform(-0.45, 0.45, BAND_SUPPORT))
        q[j, sup] = (rng.permutation(mag) * 1e-6 * 255.0 / vdiff[sup].astype(F64)).astype(F32)
    w = prep_w(q, trained)
    scale = prep_scale(w)
    nn, _, _ = digits(w, scale)
    ab = aligned_rows(q, trained)
    crafted = []
    for j in range(Q):
        sup = np.arange(j * BAND_SUPPORT, (j + 1) * BAND_SUPPORT)
        one = lambda row: exact_scores(q[j:j + 1], row[None], trained)[0, 0]
        eps = float(eps_of(eps_terms(q[j:j + 1], trained, w[j:j + 1], scale[j:j + 1], nn[j:j + 1]))[0])
        a, b = np.zeros(d, np.uint8), np.zeros(d, np.uint8)
        a[sup], b[sup] = ab[2 * j, sup], ab[2 * j + 1, sup]
        mid = [i for i in sup if 40 <= nn[j, i] <= 300 and b[i] == 255]
        assert len(mid) >= BAND_K, "band_edge: too few middling dimensions on which row B can be lowered"
        others = []
        for i in sorted(mid, key=lambda i: nn[j, i])[:BAND_K]:
            r = b.copy()
            r[i] -= 1
            others.append(r)
        target = max(one(r) for r in others) + 0.1 * eps
        u = a.copy()
        for i in sorted(sup, key=lambda i: -w[j, i]):        # large |w| first: the coarse steps cost the least alignment per unit of score
            need = target - one(u)
            room = 255 - int(u[i]) if need > 0 else int(u[i])
            step = min(room, int(abs(need) / w[j, i]))
            if step:
                u[i] = int(u[i]) + (step if need > 0 else -step)
                if (target - one(u)) * need < 0:              # (the decode is not exactly linear in the code: never cross the target)
                    u[i] = int(u[i]) - (1 if need > 0 else -1)
        crafted += [u] + others
    crafted = np.stack(crafted)
    fill = rng.integers(0, 24, (n_rows - crafted.shape[0], d), dtype=np.uint8)
    codes = np.concatenate([fill[:50], crafted, fill[50:]])      # (the crafted rows of query j: 50 + 11 j .. 50 + 11 j + 10, U first)
    return trained, codes, q


def band_edge_rows(c):
    """-> (U rows [Q], the k other crafted rows [Q, k]) of a band_edge case."""
    Q = c["d"] // BAND_SUPPORT
    u = 50 + (BAND_K + 1) * np.arange(Q)
    return u, u[:, None] + 1 + np.arange(BAND_K)[None]


def padding_pattern(q, trained, rows):
    """Codes [rows, d] that maximise the filter score: row r serves query r % Q with 255 where its w > 0 and 0 elsewhere."""
    w = prep_w(q, trained)
    return np.where(w[np.arange(rows) % q.shape[0]] > 0, 255, 0).astype(np.uint8)


_R = dict(make=_random_case, k=10, uniform=False)
CASES = {
    "d64":                  dict(_R, d=64, n=300, Q=17, seed=201),
    "d64_uniform":          dict(_R, d=64, n=300, Q=17, seed=202, uniform=True),
    "d192":                 dict(_R, d=192, n=129, Q=33, seed=203),
    "d576_uniform":         dict(_R, d=576, n=257, Q=65, seed=204, uniform=True),
    "d1024":                dict(_R, d=1024, n=1000, Q=128, seed=205),
    "two_chunks":           dict(_R, d=256, n=500, Q=129, seed=206),
    "one_row":              dict(_R, d=64, n=1, Q=1, seed=207),
    "rows_127":             dict(_R, d=64, n=127, Q=16, seed=208),
    "rows_128":             dict(_R, d=64, n=128, Q=16, seed=209),
    "rows_129":             dict(_R, d=64, n=129, Q=16, seed=210),
    "grid_stride":          dict(_R, d=64, n=2 * 2048 * 128 + 77, Q=17, seed=211),
    "aligned_d64":          dict(_R, d=64, n=200, Q=6, seed=212, make=_aligned_case),
    "aligned_d64_uniform":  dict(_R, d=64, n=200, Q=6, seed=213, make=_aligned_case, uniform=True),
    "aligned_d256":         dict(_R, d=256, n=200, Q=6, seed=214, make=_aligned_case),
    "aligned_d256_uniform": dict(_R, d=256, n=200, Q=6, seed=215, make=_aligned_case, uniform=True),
    "band_edge":            dict(_R, d=256, n=300, Q=4, seed=216, make=_band_edge_case),
    "band_edge_uniform":    dict(_R, d=256, n=300, Q=4, seed=217, make=_band_edge_case, uniform=True),
    "offset":               dict(_R, d=128, n=300, Q=8, seed=218, make=_offset_case),
    "subnormal":            dict(_R, d=128, n=300, Q=8, seed=219, make=_subnormal_case),
    "const_cols":           dict(_R, d=192, n=300, Q=8, seed=220, make=_const_cols_case),
    "padding":              dict(_R, d=64, n=300, Q=8, seed=221),
    "zero_query":           dict(_R, d=64, n=5000, Q=5, seed=222, make=_zero_query_case, zero=(2,)),
    "nonfinite_query":      dict(_R, d=64, n=300, Q=6, seed=223, make=_nonfinite_case, bad=(1, 4)),
}
ALIGNED = [n for n in CASES if n.startswith("aligned")]
BAND_EDGE = [n for n in CASES if n.startswith("band_edge")]


def case_spec(name):
    c = dict(zero=(), bad=())
    c.update(CASES[name])
    c["qtype"] = "QT_8bit_uniform" if c["uniform"] else "QT_8bit"
    return c


_DATA, _MODELS = {}, {}


def case_data(name):
    """(trained, codes uint8 [n, d] row-major, q fp32 [Q, d]) of a case: built once per process and shared (do not modify)."""
    if name not in _DATA:
        c = case_spec(name)
        out = c["make"](c, np.random.default_rng(c["seed"]))
        for a in out:
            a.setflags(write=False)
        assert out[1].shape == (c["n"], c["d"]) and out[2].shape == (c["Q"], c["d"])
        _DATA[name] = out
    return _DATA[name]


def case_model(name, chunk=None):
    """StageModel of the case's good queries (all of them, or of the query chunk `chunk` = (q0, nq)): built once per process, shared."""
    key = (name, chunk)
    if key not in _MODELS:
        trained, codes, q = case_data(name)
        if chunk is not None:
            q = q[chunk[0]:chunk[0] + chunk[1]]
        with np.errstate(all="ignore"):
            _MODELS[key] = StageModel(q, codes, trained)
    return _MODELS[key]


def good_queries(name):
    c = case_spec(name)
    return np.array([i for i in range(c["Q"]) if i not in c["bad"]])
