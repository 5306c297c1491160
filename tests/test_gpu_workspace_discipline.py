"""GPU: every workspace-taking entry of the index classes and of the encoder, run in a workspace of EXACTLY the bytes its `lrx_*_workspace_bytes`
declared, planted between two guard bands (tests/ws_guard.py), under five fills of that block ("Workspace discipline"):

    1. 0x00     2. the leavings of a LARGER call of the same entry (more queries, a larger k or a lower radius) on the same index
    3. the leavings of the OTHER kind of call on that index (range after top-k, rerank=False after rerank=True, sel= after plain, ...)
    4. 0x7F (floats near FLT_MAX, large positive counters)     5. 0xFF (negative NaNs, -1 / UINT_MAX counters)

in this order for all calls of a case (the benign fills of every call come before the first hostile one: run the file with -x).  After every
call: (a) the result equals the expected one on bits, (b) no guard byte changed -- under fills 2 and 3 the bytes of the larger block behind
the planted one count as guard too, (c) the call ran in the planted block (a block that is too small is silently replaced by the wrappers,
and every check would pass vacuously), (d) the index's resident inputs are bit-unchanged, (e) the device error counter (and the search
fallback counter, for the 8-bit index) moved by exactly what the case's inputs predict: 0 unless the inputs hold an out-of-range entry.

The expected results are the families' yardsticks, built the way their own test_gpu_* files build them (helpers imported from there), on data
whose scores do not depend on the order of a summation (integers, or multiples of 2^-10).  The encoder has no bit-exact reference: its
expected result is its own run in a fresh block, tied to the goldens by the sibling tests' own checks (see encoder_case).  No comparison in
this file has a tolerance."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_selector_yardstick as YS  # noqa: E402
import range_codes_yardstick as RY  # noqa: E402
import refine_yardstick as YR  # noqa: E402
import pca_yardstick as YP  # noqa: E402
import sq8_stage_reference as R8  # noqa: E402
import sq8_yardstick as Y8  # noqa: E402
import impact_yardstick as YI  # noqa: E402
import test_gpu_binary_index as TB  # noqa: E402
import test_gpu_ivf_range as RG  # noqa: E402
import test_gpu_pq_index as TP  # noqa: E402
import test_gpu_range_search as TR  # noqa: E402
import test_gpu_sq8_index as T8  # noqa: E402
from test_gpu_ivf_range import dev, errors  # noqa: E402
from ws_guard import Guarded, assert_planted, plant  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
FILLS = ("0x00", "larger call", "other call", "0x7F", "0xFF")


# ---- the harness ----------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Call:
    """One entry under test.  run(big) makes the call (big: the larger call of fill 2, whose result is not compared) and returns a tuple of
    tensors; want: the expected tuple (tensors or arrays; None: the run in a fresh block -- the encoder only); other: the name of the call of the
    other kind (fill 3); errors: what lrx_device_error_count moves by per call; fallbacks: what lrx_search_fallback_count moves by (None: not
    read)."""
    name: str
    run: object
    want: object = None
    other: str = None
    errors: int = 0
    fallbacks: int = None


@dataclasses.dataclass
class Case:
    obj: object                 # what holds the workspace ...
    calls: list
    resident: object            # () -> {name: live tensor}: rows / codes / centroids / lists / selector words of the index
    attr: str = "_ws"           # ... and under which attribute


def bits_of(x):
    """A tensor or array -> a tensor (where it lives) whose equality is equality on bits (floats as integers: NaN == NaN, -0 != +0)."""
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.contiguous()
    if t.dtype in (torch.float32,):
        return t.view(torch.int32)
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def same(got, want):
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if g is None or w is None:
            if g is not w:
                return False
            continue
        g, w = bits_of(g), bits_of(w)
        w = w.to(g.device)
        if g.dtype != w.dtype or g.shape != w.shape or not torch.equal(g, w):
            return False
    return True


def fallbacks():
    from lightretriever_amd import _lib
    torch.cuda.synchronize()
    return int(_lib.lib().lrx_search_fallback_count(1))


def run_case(case: Case):
    obj, attr = case.obj, case.attr
    by_name = {c.name: c for c in case.calls}
    kept = {k: t.clone() for k, t in case.resident().items()}          # (d): clones taken before the first call

    def resident_changed():
        live = case.resident()
        return [k for k in kept if not torch.equal(bits_of(live[k]), bits_of(kept[k]))]

    # what each call needs: the first allocation of a call is exactly the library's figure, and its numel() is what the wrappers pass on
    errors()
    fallbacks()
    need = {}
    for c in case.calls:
        for big in (False, True):
            setattr(obj, attr, None)
            got = c.run(big)
            torch.cuda.synchronize()
            need[c.name, big] = int(getattr(obj, attr).numel())
            n_err, n_fb = errors(), fallbacks()
            if not big:
                if c.want is None:
                    c.want = tuple(None if t is None else t.clone() for t in got)
                assert same(got, c.want), f"{c.name}: a fresh block"
                assert n_err == c.errors, f"{c.name}: device error count in a fresh block"
                assert c.fallbacks is None or n_fb == c.fallbacks, f"{c.name}: fallback count in a fresh block"
        assert need[c.name, True] >= need[c.name, False], f"{c.name}: the larger call must need no less ({need[c.name, True]} < {need[c.name, False]})"
    assert not resident_changed()
    device = getattr(obj, attr).device
    setattr(obj, attr, None)

    def checked(c, g, n, where):
        """The small call in the first n bytes of g's inner block; the bytes behind them are guard too."""
        plant(obj, g, n, attr)
        tail = g.ws[n:].clone()
        g.arm()
        got = c.run(False)
        torch.cuda.synchronize()
        assert same(got, c.want), f"{where}: (a) the result depends on what the workspace held"
        bad = g.check()
        assert bad.numel() == 0, f"{where}: (b) {bad.numel()} guard bytes changed, the first at {int(bad[0]) - g.guard} from the start of the block of {n}"
        assert torch.equal(g.ws[n:], tail), f"{where}: (b) bytes behind the declared {n} changed"
        assert_planted(obj, g, attr)
        assert getattr(obj, attr).numel() == n, f"{where}: (c) the planted block was replaced"
        changed = resident_changed()
        assert not changed, f"{where}: (d) resident inputs changed: {changed}"
        assert errors() == c.errors, f"{where}: (e) device error count"
        assert c.fallbacks is None or fallbacks() == c.fallbacks, f"{where}: (e) fallback count"

    for fill in FILLS:
        for c in case.calls:
            where = f"{c.name} / {fill}"
            n = need[c.name, False]
            if fill == "larger call":
                nb = need[c.name, True]
                g = Guarded(nb, device)
                g.fill(0x00).arm()
                plant(obj, g, None, attr)
                c.run(True)
                torch.cuda.synchronize()
                assert g.check().numel() == 0, f"{where}: the larger call wrote outside its own {nb} bytes"
                assert_planted(obj, g, attr)
                errors()
                fallbacks()
                checked(c, g, n, where)
            elif fill == "other call":
                if c.other is None:
                    continue
                o = by_name[c.other]
                no = need[o.name, False]
                g = Guarded(max(no, n), device)
                g.fill(0x00).arm()
                plant(obj, g, no, attr)
                o.run(False)
                torch.cuda.synchronize()
                assert g.check().numel() == 0, f"{where}: {o.name} wrote outside its own {no} bytes"
                assert_planted(obj, g, attr)
                errors()
                fallbacks()
                checked(c, g, n, where)
            else:
                g = Guarded(n, device)
                g.fill(int(fill, 16))
                checked(c, g, n, where)
            setattr(obj, attr, None)
            del g


# ---- data whose scores do not depend on the order of the sum ------------------------------------------------------------------------------------------
def grid(shape, seed, step):
    """Gaussian values rounded to multiples of `step` inside (-4, 4).  step = 2^-10: a product of two is a multiple of 2^-20 below 16, a sum of
    d <= 1024 of them has 34 significant bits -- exact in fp64 in ANY order, so (float) of it is one well-defined number.  step = 2^-8: such a
    value is an fp16 number (10 significant bits), so fp16 codes hold it exactly."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(*shape, generator=g, device="cuda").clamp_(-3.9, 3.9)
    return (torch.round(x / step) * step).contiguous()


def radius_at(S, per_query):
    """A radius that IS a score of S (strictly greater excludes it), about per_query rows per query above it."""
    flat = torch.sort(S.reshape(-1), descending=True).values
    return float(flat[min(per_query * S.shape[0], flat.numel() - 1)])


def exact_scores(q, x):
    return (q.double() @ x.double().T).float()


# ---- FlatIPIndex: lrx_flat_ip_search_bounded_wire, lrx_flat_ip_search, lrx_flat_ip_range_search -------------------------------------------------------
def flat_case(d, n, queries, six_product=False, expect=None):
    """queries: {Q: k}.  The paths by the code (lrx_search.hip): n <= REF_CAND = 4096 rows: bounded_search hands the call to the plain path
    (lrx_flat_ip_search) and the range search takes its score-matrix path; n >= 16384: plan_chunk's score-free filter (emit) -- one persistent
    launch for sample, selection and main pass (fused) at <= 16 queries, d >= 512, d % 256 == 0, k <= 256; the main pass on the GEMM kernel
    at MORE than 128 queries and d >= 1024 (not at Q in {1, 7}: the code wins over the issue's guess); the range search takes its list path
    above 4096 rows.  n is no multiple of 128.  expect: {Q: plan facts last_chunk_state() must report}."""
    from lightretriever_amd import FlatIPIndex
    assert n % 128 != 0
    x = grid((n, d), 100 + d + n, 2.0 ** -10)
    x[n - 3] = x[5]                                                     # a twin: equal scores, the lower row first
    idx = TR.make_index(x, id_base=40)
    more = lambda Q: min(2 * Q + 3, 256)                                 # (one library chunk: a call of more queries forks over internal streams and lanes)
    q = grid((more(max(queries)), d), 7 + d, 2.0 ** -10)
    q[0] = x[5]
    S = exact_scores(q, x)
    calls = []

    def topk(Q, k, name, two_pass=True):
        def run(big):
            idx.two_pass = two_pass
            try:
                return idx.search(q[:more(Q)], 2 * k) if big else idx.search(q[:Q], k)
            finally:
                idx.two_pass = True
        D, I = T8.fp64_topk(q[:Q], x, k)
        return Call(name, run, (D, torch.where(I >= 0, I + 40, I)))

    for Q, k in queries.items():
        calls.append(topk(Q, k, f"search Q={Q}"))
        radius, low = radius_at(S[:Q], 30), radius_at(S[:more(Q)], 300)
        calls.append(Call(f"range_search Q={Q}", lambda big, Q=Q, radius=radius, low=low: idx.range_search(q[:more(Q)], low) if big else idx.range_search(q[:Q], radius),
                          TR.range_fp64_gpu(q[:Q], x, radius, id_base=40), other=f"search Q={Q}"))
        calls[-2].other = f"range_search Q={Q}"
    if six_product:                                                     # two_pass = False: the [Q, rows] score matrix of lrx_flat_ip_search
        Q, k = 7, queries[7]
        calls.append(topk(Q, k, "search two_pass=False", two_pass=False))
        calls[-1].other = "search Q=7"
    case = Case(idx, calls, lambda: {"rows": idx._x[:n], "shadow": idx._xb, "bounds": idx._bounds})
    if expect:
        for Q, facts in expect.items():
            idx.search(q[:Q], queries[Q])
            if facts == "plain":
                from lightretriever_amd import _lib
                with pytest.raises(_lib.LrxError, match="plain path"):
                    idx.last_chunk_state(0)
            else:
                st = idx.last_chunk_state(0)
                assert {f: st[f] for f in facts} == facts, (Q, {f: st[f] for f in facts})
        idx._ws = None
    return case


# ---- SQFp16Index: lrx_sq_fp16_ip_search, lrx_sq_fp16_ip_range_search -----------------------------------------------------------------------------------------
def sq_fp16_case():
    from lightretriever_amd import SQFp16Index
    n, d = 1029, 64
    x = grid((n, d), 3, 2.0 ** -8)                                       # fp16 numbers: the codes ARE the rows
    x[n - 1] = x[2]
    idx = SQFp16Index(d, id_base=9)
    idx.add(x)
    assert torch.equal(idx.codes().float(), x)
    q = grid((17, d), 4, 2.0 ** -10)
    S = exact_scores(q, x)
    D, I = T8.fp64_topk(q[:7], x, 10)
    radius, low = radius_at(S[:7], 20), radius_at(S, 200)
    calls = [Call("search", lambda big: idx.search(q, 100) if big else idx.search(q[:7], 10), (D, I + 9), other="range_search"),
             Call("range_search", lambda big: idx.range_search(q, low) if big else idx.range_search(q[:7], radius),
                  TR.range_fp64_gpu(q[:7], x, radius, id_base=9), other="search")]
    return Case(idx, calls, lambda: {"codes": idx._xb, "bounds": idx._bounds})


# ---- PQIndex: lrx_pq_ip_search, lrx_pq_ip_range_search (the shapes of test_gpu_pq_index's two-pass test) ---------------------------------------------
def pq_case(d, M):
    idx, C, codes = TP.make(d, M, 1029, seed=M)
    idx.id_base = 5
    q = torch.from_numpy(TP.queries(12, d, seed=d)).cuda()
    S = TP.Y.scores_torch(TP.lut_torch(q, C), codes)
    radius, low = radius_at(S[:5], 20), radius_at(S, 300)
    calls = [Call("search", lambda big: idx.search(q, 100) if big else idx.search(q[:5], 10), TP.want_topk(q[:5], C, codes, 10, id_base=5), other="range_search"),
             Call("range_search", lambda big: idx.range_search(q, low) if big else idx.range_search(q[:5], radius),
                  TP.want_range(q[:5], C, codes, radius, id_base=5), other="search")]
    return Case(idx, calls, lambda: {"codes": idx._codes, "centroids": idx.centroids})


# ---- SQ8Index: lrx_sq8_ip_search, on the cases of tests/sq8_stage_reference.py ---------------------------------------------------------------------------------
def sq8_case(name):
    """d64: a range per dimension; d64_uniform: one range; zero_query: query 2 is all zeros, every row ties, its band holds all 5000 rows and
    the selection takes the streaming fallback (sq8_stage_reference predicts one fallback per search: test_gpu_sq8_stages.test_results)."""
    from lightretriever_amd import SQ8Index
    c = R8.case_spec(name)
    trained, codes, q = R8.case_data(name)
    idx = SQ8Index(c["d"], c["qtype"], id_base=1000)
    idx.set_contents(torch.from_numpy(np.array(trained)), torch.from_numpy(np.array(codes)))
    qt = torch.from_numpy(np.array(q)).cuda()
    qbig = torch.cat([qt, qt.flip(0)])
    k = c["k"]
    Dw, Iw = Y8.topk(R8.case_model(name).s, k)
    Iw = np.where(Iw >= 0, Iw + 1000, -1)
    for z in c["zero"]:                                                  # rows 0 .. k - 1 at a score of +0 (test_gpu_sq8_stages.test_results)
        Dw[z], Iw[z] = 0.0, 1000 + np.arange(k)
    call = Call("search", lambda big: idx.search(qbig, 8 * k) if big else idx.search(qt, k), (Dw, Iw), fallbacks=len(c["zero"]))
    return Case(idx, [call], lambda: {"codes": idx._codes, "trained": idx.trained})


# ---- BinaryFlatIndex: lrx_binary_ip_search, lrx_binary_hamming_search ----------------------------------------------------------------------------------------------
def binary_case(d, n, Q):
    """d = 136: d % 128 != 0 (two 16-byte groups per row, the second mostly padding), Q = 7 on the 32-query tile, rows 100 .. 399 identical:
    the cutoff bin of a query near them holds 300 ties spread over the 1024-row tiles (tiecnt / tiebase).  d = 8192, Q = 5: bin_query_tile's
    4-query tile (d > 4096) with a histogram of 4 x 4097 words = 65 552 B, over 64 KiB; the second tile has one query and three padding ones."""
    xb = TB.random_packed(n, d, seed=d)
    xb[100:400] = xb[100]
    idx = TB.build(xb, d, id_base=3)
    q = TB.grid_q(2 * Q + 2, d, seed=2)
    q[1] = (((xb[100][:, None].int() >> torch.arange(7, -1, -1, device="cuda")) & 1).reshape(-1).float() * 2 - 1)   # the cluster at distance 0
    H = TB.hamming_t(TB.pack_t(q[:Q]), xb)
    shift = lambda DI: (DI[0], torch.where(DI[1] >= 0, DI[1] + 3, DI[1]))
    _, C = TB.hamming_topk_t(H, 200)
    calls = [Call("search rerank=True", lambda big: idx.search(q, 50, binary_k=1000) if big else idx.search(q[:Q], 10, binary_k=200),
                  shift(TB.rerank_t(q[:Q], xb, C, 10)), other="search rerank=False"),
             Call("search rerank=False", lambda big: idx.search(q, 600, rerank=False) if big else idx.search(q[:Q], 350, rerank=False),
                  shift(TB.hamming_topk_t(H, 350)), other="search rerank=True")]
    return Case(idx, calls, lambda: {"codes": idx._codes})


# ---- ImpactIndex: lrx_impact_search, lrx_range_impact_search ---------------------------------------------------------------------------------------------------------
def impact_case():
    """1000 documents over 200 terms; term 300 sits in three rows only, so the queries that name it alone have fewer hits than k; one query names no
    known term."""
    from lightretriever_amd import ImpactIndex
    from lightretriever_amd.impact_index import query_csr
    rng = np.random.default_rng(11)
    docs = [(rng.choice(200, 8, replace=False), rng.integers(1, 300, 8)) for _ in range(1000)]
    for r in (5, 400, 999):
        docs[r] = (np.append(docs[r][0], 300), np.append(docs[r][1], 9))
    csr = YI.csr_of(docs)
    idx = ImpactIndex(id_base=70)
    idx.add(*csr)
    yard = YI.Yardstick(*csr)
    queries = [([300], [2]), ([5000], [1]), ([300, 7], [1, 4])] + [(rng.choice(201, 3, replace=False), rng.integers(1, 5, 3)) for _ in range(4)]
    more = queries + [(rng.choice(201, 5, replace=False), rng.integers(1, 5, 5)) for _ in range(10)]
    k = 10
    Dw, Iw = yard.search(queries, k)
    assert (Iw[0] >= 0).sum() == 3 and (Iw[1] == -1).all()
    known = [(np.asarray(t)[np.asarray(t) < 301], np.asarray(c)[np.asarray(t) < 301]) for t, c in queries]
    S = RY.impact_scores(yard, known)
    radius = float(np.sort(S[S > 0])[::-1][40])
    calls = [Call("search", lambda big: idx.search(*query_csr(more), 100) if big else idx.search(*query_csr(queries), k),
                  (Dw, np.where(Iw >= 0, Iw + 70, -1)), other="range_search"),
             Call("range_search", lambda big: idx.range_search(*query_csr(more), -1.0) if big else idx.range_search(*query_csr(queries), radius),
                  RY.range_impact(S, radius, id_base=70), other="search")]
    idx.search(*query_csr(queries), k)                                   # (finalize(): the postings exist from here on)
    idx._ws = None
    return Case(idx, calls, lambda: {"postings": idx._postings, "term_off": idx._term_off})


# ---- RefineFlatIndex.search and refine.rerank(ws_slots=...): lrx_flat_ip_rerank, lrx_sq_fp16_ip_rerank -----------------------------------------------------------------
class Slots:
    """A holder whose vars() is the dict refine.rerank keeps its workspace in (key "_ws")."""
    _ws = None


def refine_case(store_kind):
    """A PQ base (600 x 128, M = 16, trained here) under a flat or an fp16 store; the rows are fp16 numbers, so both stores hold the same values.
    search(): the candidates are the base's own top k_base, taken once up front.  rerank(ws_slots=): hand-made candidates with padding (-1),
    a row named twice and rows at or past ntotal -- skipped, never read, and counted once each in lrx_device_error_count."""
    from lightretriever_amd import PQIndex, RefineFlatIndex, SQFp16Index
    from lightretriever_amd import refine as RF
    n, d, K = 600, 128, 20
    x = grid((n, d), 11, 2.0 ** -8)
    x[n - 10:] = x[:10]
    q = grid((17, d), 12, 2.0 ** -10)
    idx = RefineFlatIndex(PQIndex(d, 16), SQFp16Index(d) if store_kind == "fp16" else None, k_factor=2.0)
    idx.train(x)
    idx.add(x)
    idx.id_base = 30
    xn, qn = x.cpu().numpy(), q.cpu().numpy()
    cand = idx.base_index.search(q[:7], 2 * K)[1]
    calls = [Call("search", lambda big: idx.search(q, 2 * K, k_factor=4.0) if big else idx.search(q[:7], K), YR.rerank(qn[:7], xn, cand.cpu().numpy(), K, id_base=30),
                  other="search k_factor=1")]
    cand1 = idx.base_index.search(q[:7], K)[1]
    calls.append(Call("search k_factor=1", lambda big: idx.search(q, 2 * K, k_factor=3.0) if big else idx.search(q[:7], K, k_factor=1.0),
                      YR.rerank(qn[:7], xn, cand1.cpu().numpy(), K, id_base=30), other="search"))
    store = idx.refine_index
    rows = (lambda: {"store": store._xb, "bounds": store._bounds}) if store_kind == "fp16" else (lambda: {"store": store._x[:n]})
    base = idx.base_index
    resident = lambda: dict(rows(), base_codes=base._codes, base_centroids=base.centroids)
    # the function itself, its workspace in a caller's dict
    rng = np.random.default_rng(4)
    hand = rng.integers(0, n, (5, 48))
    hand[:, 3::4] = rng.integers(n, n + 500, hand[:, 3::4].shape)        # past ntotal
    hand[0, ::2] = -1
    hand[1, :6] = [17, 4, 17, 250, 4, -1]
    hand[4] = n + np.arange(48)                                          # a query with nothing valid
    n_bad = int((hand >= n).sum())
    hand_big = rng.integers(0, n, (12, 200))
    slots = Slots()
    hd, hb = dev(hand), dev(hand_big)
    fn = Call("rerank(ws_slots=)", lambda big: RF.rerank(q[:12], store, hb, 50, 0, None, vars(slots)) if big else RF.rerank(q[:5], store, hd, K, 0, None, vars(slots)),
              YR.rerank(qn[:5], xn, hand, K, n_rows=n), errors=n_bad)
    return Case(idx, calls, resident), Case(slots, [fn], resident)


# ---- PreTransformIndex(PCAMatrix, PQIndex): the base's workspace ------------------------------------------------------------------------------------------------------------
def pca_pq_case():
    """d 64 -> 32 with an integer matrix and integer queries: transform.apply(q) is exact (tests/pca_yardstick.apply gives the same integers), and
    the base is a PQIndex(32, 8) of fixed contents -- the expected result is pq_yardstick's over apply(q).  The planted block is the BASE's."""
    from lightretriever_amd import PCAMatrix, PreTransformIndex
    rng = np.random.default_rng(21)
    A = rng.integers(-2, 3, (32, 64)).astype(np.float32)
    b = rng.integers(-3, 4, 32).astype(np.float32)
    st = dict(d_in=64, d_out=32, eigen_power=0.0, random_rotation=False, is_trained=True, mean=np.zeros(64, np.float32), eigenvalues=np.ones(64, np.float32),
              PCAMat=np.zeros((64, 64), np.float32), A=A, b=b)
    base, C, codes = TP.make(32, 8, 1029, seed=3)
    idx = PreTransformIndex(PCAMatrix.from_state(st, device=base.device), base)
    q = rng.integers(-3, 4, (12, 64)).astype(np.float32)
    yq = YP.apply(q, A, b).astype(np.float32)
    qd = dev(q)
    assert torch.equal(idx.transform.apply(qd), dev(yq))
    call = Call("search", lambda big: idx.search(qd, 100) if big else idx.search(qd[:5], 10), TP.want_topk(dev(yq[:5]), C, codes, 10))
    return Case(base, [call], lambda: {"codes": base._codes, "centroids": base.centroids, "A": idx.transform.A, "b": idx.transform.b})


# ---- the four inverted-file indexes: search, range_search_probed, and the hooks they end in with hand-given probes, each with and without sel= ------------------------------------
# eight cells, 3000 rows: an empty cell, one of three rows, one of 2300 -- more than IVF_SEL_SORT = 2048 words on its own, so k_ivf_select takes its
# radix path for every query that probes it (all of them at nprobe = 8: a segment of 3000 words), while nprobe = 1 over the other cells is sorted whole
IVF_SIZES = [0, 3, 130, 2300, 200, 67, 250, 50]
# a repeat, a -1 and the empty cell | 2880 rows: one more than max_scan | padding | a repeat behind the large cell
IVF_HAND = np.array([[2, 2, -1, 0], [3, 4, 6, 2], [1, 5, -1, -1], [7, 3, 3, 4]], np.int64)
IVF_HAND_SCAN = 2300 + 200 + 250 + 130 - 1


def above(full, radius):
    """The yardstick's full result (every scanned pair, segment order) -> its hits above `radius`."""
    lims, D, I = full
    keep = D > np.float32(radius)
    return np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)[lims], D[keep], I[keep]


def ivf_case(fam):
    from lightretriever_amd import RowSelector
    S = RG.Store(fam, IVF_SIZES, d=64, Q=16, seed=5, by_residual=True)
    assert S.n == 3000 and S.nlist == 8
    idx = S.index(1)
    mask = np.random.default_rng(6).random(S.n) < 0.3
    sel = RowSelector.from_mask(mask)
    everything = np.ones(S.n, bool)
    host = lambda t: None if t is None else t.cpu().numpy()
    calls = []

    def add(name, run, full, k=None, radius=None, err=0):
        """The call without and with the selector; each is the other's `other kind`."""
        for tag, m, s in (("", everything, None), (" sel=", mask, sel)):
            want = YS.filter_topk(*YS.split(*full), m, k) if k is not None else YS.filter_range(*above(full, radius), m)
            calls.append(Call(name + tag, lambda big, s=s: run(big, s), want, errors=err))
        calls[-1].other, calls[-2].other = calls[-2].name, calls[-1].name

    # the public entries: the probes are the quantiser's own (taken once, up front, and handed to the yardstick)
    for nprobe, k in ((8, 50), (1, 10)):
        Q = 7
        q, qbig = dev(S.q[:Q]), dev(S.q)
        if nprobe == 1:                                                  # each query next to one centroid: all eight cells get probed, the empty one too
            qn = S.q.copy()
            qn[:8] += 4 * S.cent
            q, qbig = dev(qn[:Q]), dev(qn)
        ps, pr = idx.quantizer.search(q, nprobe)
        full = S.want(host(pr), host(ps) if S.by_residual else None, -INF, q=host(q))
        add(f"search nprobe={nprobe}", lambda big, s, q=q, qbig=qbig, k=k, nprobe=nprobe: idx.search(qbig, 4 * k, nprobe=nprobe, sel=s) if big else
            idx.search(q, k, nprobe=nprobe, sel=s), full, k=k)
        if nprobe == 8:
            radius = float(np.median(full[1]))
            add("range_search_probed", lambda big, s, q=q, qbig=qbig, radius=radius: idx.range_search_probed(qbig, -INF, 8, sel=s) if big else
                idx.range_search_probed(q, radius, 8, sel=s), full, radius=radius)
    # the hooks search() / range_search_probed() end in, with hand-given probes and a max_scan_rows one row short for query 1 (counted once per call)
    q4, q8 = dev(S.q[:4]), dev(S.q[:8])
    base = S.base(IVF_HAND.shape)
    pb, pb8 = dev(IVF_HAND), dev(np.concatenate([IVF_HAND, IVF_HAND[::-1]]))
    bs = None if base is None else dev(base)
    bs8 = None if base is None else dev(np.concatenate([base, base[::-1]]))
    full = S.want(IVF_HAND, base, -INF, q=S.q[:4], max_scan_rows=IVF_HAND_SCAN)
    assert np.diff(full[0]).tolist() == [130, 0, 3 + 67, 50 + 2300 + 200]
    words = lambda s: None if s is None else s.words
    add("_topk_cells hand probes", lambda big, s: idx._topk_cells(q8, 100, pb8, bs8, S.n, None, None, words(s)) if big else
        idx._topk_cells(q4, 50, pb, bs, IVF_HAND_SCAN, None, None, words(s)), full, k=50, err=1)
    radius = float(np.median(full[1]))
    add("_range_cells hand probes", lambda big, s: idx._range_cells(q8, -INF, pb8, bs8, S.n, None, words(s)) if big else
        idx._range_cells(q4, radius, pb, bs, IVF_HAND_SCAN, None, words(s)), full, radius=radius, err=1)
    # fill 3 across the kinds as well: top k <-> range
    by = {c.name: c for c in calls}
    by["search nprobe=8"].other, by["range_search_probed"].other = "range_search_probed", "search nprobe=8"
    idx._ws = None

    def resident():
        out = {"list_off": idx.list_off, "row_ids": idx.row_ids, "centroids": idx.quantizer._x[:idx.nlist], "sel": sel.words}
        if fam == "pq":
            out.update(codes=idx.pq._codes, pq_centroids=idx.pq.centroids)
        else:
            out["store"] = idx._store
        if fam == "sq8":
            out["trained"] = idx.trained
        return out
    return Case(idx, calls, resident)


# ---- LrxEncoder on llama_small_d64 ----------------------------------------------------------------------------------------------------------------------------------------------
def encoder_case():
    """The first three sequences of the golden batch (100 + 64 + 31 = 195 tokens: no multiple of 128, two row tiles) after a batch of 16 longer
    ones.  The goldens are the reference model's fp32 outputs, which the kernels meet within a band, not on bits -- so the expected result of
    a call is its own run in a fresh block, and that run is tied to the goldens without a bound of this file's: the sibling tests' own golden
    checks run here on the same library (test_gpu_encoder), and the pooled rows of the three sequences must be, on bits, rows 0 .. 2 of the
    whole golden batch's run -- the run those checks compare with the goldens."""
    import test_gpu_encoder as TE
    from helpers import load_model_golden
    cfg, w, g, ids, cu, max_len = load_model_golden("llama_small_d64")
    TE.test_golden_models_within_reference_bf16_band("llama_small_d64")
    enc = TE.make_encoder(cfg, w)
    T3 = int(cu[3])
    assert T3 % 128 != 0 and len(set(np.diff(cu[:4]).tolist())) == 3
    ids3, cu3, len3 = TE.to_dev(ids[:T3], torch.int32), TE.to_dev(cu[:4], torch.int32), int(np.diff(cu[:4]).max())
    rng = np.random.default_rng(2)
    lens = rng.integers(130, 200, 16)
    idsb = TE.to_dev(rng.integers(0, cfg.vocab_size, int(lens.sum())), torch.int32)
    cub = TE.to_dev(np.concatenate([[0], np.cumsum(lens)]), torch.int32)
    lenb = int(lens.max())
    pre, suf = ids3[:37].contiguous(), ids3[40:100].reshape(3, 20).contiguous()
    preb, sufb = idsb[:100].contiguous(), idsb[100:100 + 16 * 60].reshape(16, 60).contiguous()
    packed = lambda pooling: (lambda big: (enc.encode_packed(idsb, cub, lenb, pooling=pooling) if big else enc.encode_packed(ids3, cu3, len3, pooling=pooling),))
    calls = [Call("encode_packed lasttoken", packed("lasttoken"), other="encode_hidden"),
             Call("encode_packed mean", packed("mean"), other="encode_packed lasttoken"),
             Call("encode_hidden", lambda big: (enc.encode_hidden(idsb, cub, lenb) if big else enc.encode_hidden(ids3, cu3, len3),), other="encode_packed_sparse"),
             Call("encode_packed_sparse", lambda big: enc.encode_packed_sparse(idsb, cub, lenb) if big else enc.encode_packed_sparse(ids3, cu3, len3),
                  other="encode_prefixed"),
             Call("encode_prefixed", lambda big: (enc.encode_prefixed(preb, sufb) if big else enc.encode_prefixed(pre, suf),), other="encode_packed mean")]
    whole = {p: enc.encode_packed(TE.to_dev(ids, torch.int32), TE.to_dev(cu, torch.int32), max_len, pooling=p) for p in ("lasttoken", "mean")}
    enc._ws = None

    def resident():
        out = {"embed": enc.embed, "final_norm": enc.final_norm}
        for i, L in enumerate(enc.layers):
            out.update({f"layer{i}.{k}": v for k, v in L.items() if isinstance(v, torch.Tensor)})
        return out
    case = Case(enc, calls, resident)
    return case, whole


# ---- the cases: one per row of the issue's table (a row with several shapes has one per shape) ------------------------------------------------------------------------------------
CASES = {
    "flat d=64 n=3000 plain path": lambda: flat_case(64, 3000, {1: 10, 7: 10}, expect={7: "plain"}),
    "flat d=64 n=20000 two-pass chain": lambda: flat_case(64, 20000, {1: 10, 7: 10}, six_product=True, expect={7: dict(emit=True, fused=False, gemm=False)}),
    "flat d=1024 n=16500 fused and GEMM main pass": lambda: flat_case(1024, 16500, {7: 10, 130: 10},
                                                                      expect={7: dict(emit=True, fused=True), 130: dict(emit=True, gemm=True)}),
    "sq_fp16 n=1029 d=64": sq_fp16_case,
    "pq d=400 M=200": lambda: pq_case(400, 200),
    "pq d=64 M=8": lambda: pq_case(64, 8),
    "sq8 per-dimension range": lambda: sq8_case("d64"),
    "sq8 uniform range": lambda: sq8_case("d64_uniform"),
    "sq8 fallback band": lambda: sq8_case("zero_query"),
    "binary d=136 n=2500": lambda: binary_case(136, 2500, 7),
    "binary d=8192 n=1100": lambda: binary_case(8192, 1100, 5),
    "impact": impact_case,
    "refine over a flat store": lambda: refine_case("flat"),
    "refine over an fp16 store": lambda: refine_case("fp16"),
    "pretransform pca pq": pca_pq_case,
    "ivf flat": lambda: ivf_case("flat"),
    "ivf pq": lambda: ivf_case("pq"),
    "ivf sq_fp16": lambda: ivf_case("sq_fp16"),
    "ivf sq8": lambda: ivf_case("sq8"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_result_and_guards_do_not_depend_on_the_workspace_contents(name):
    built = CASES[name]()
    for case in built if isinstance(built, tuple) else (built,):
        run_case(case)
    assert errors() == 0


def test_encoder_result_and_guards_do_not_depend_on_the_workspace_contents():
    case, whole = encoder_case()
    run_case(case)
    by = {c.name: c for c in case.calls}
    for pooling in ("lasttoken", "mean"):                                # the fresh-block reference IS the golden batch's run, row for row
        assert same(by[f"encode_packed {pooling}"].want, (whole[pooling][:3],)), pooling
    assert errors() == 0
