"""Every filter stage of the bounded inner-product search against the fp64 model of search_reference.py -- not only the final (scores, ids),
which hide stage errors behind the exact rescoring and the gated fallback.  One search per case with the filter forced by search_flags, then
FlatIPIndex.last_chunk_state(): eps, the filter score of every list entry, the lists themselves, T', the band and the fallback flags.
The cases, their seeds and their preconditions are in search_reference.py / test_search_reference_host.py (checked there without a GPU).

Worst ratios measured on MI355X (test_zz_worst_case_summary prints them; each must stay <= 1, eps <= the written factor): |s~ - st64| / acc
0.0071, eps / eps_ref 1.002464 of 1.010206 allowed, list count / upper prediction 1.0000, band / upper prediction 1.0000 ("What the
stage tests pin")."""
import numpy as np
import pytest
import torch

import search_reference as R
from helpers import flat_ip_topk_fp64

pytestmark = pytest.mark.gpu

_RUNS = {}          # (case, flags) -> dict(state, model, stats): one search per case and process, shared (never modified)
ID_BASE = 1000


def _run(name, flags=None):
    from lightretriever_amd import FlatIPIndex, SQFp16Index, _lib
    c = R.case_spec(name)
    flags = c["flags"] if flags is None else flags
    if (name, flags) in _RUNS:
        return _RUNS[(name, flags)]
    X, q = R.case_data(name)
    k = c["k"]
    if c["index"] == "sq":
        idx = SQFp16Index(c["D"], capacity=c["N"], id_base=ID_BASE)
    else:
        idx = FlatIPIndex(c["D"], capacity=c["N"], id_base=ID_BASE)
        idx.shadow_f16 = c["shadow"]
    with pytest.raises(_lib.LrxError, match="no search has run"):
        idx.last_chunk_state()
    half = -(-c["N"] // 2)
    idx.add(torch.tensor(X[:half]))
    idx.add(torch.tensor(X[half:]))
    idx.search_flags = flags
    lib = _lib.lib()
    lib.lrx_search_fallback_count(1)
    D, I = idx.search(torch.tensor(q), k)
    fallbacks = int(lib.lrx_search_fallback_count(0))
    n = idx.last_chunk_state(max_entries=0)["count"]
    st = idx.last_chunk_state(max_entries=int(min(n.max(), 1 << 17)))
    assert torch.equal(idx.last_list_counts().cpu(), st["count"])          # the older statistic reads the same counters
    plan = {key: st[key] for key in ("emit", "fused", "gemm", "ss", "rb", "cap", "nsplit", "group_rows", "nsamp")}
    bounds = idx._bounds.cpu().numpy()
    model = R.StageModel(q, X, bounds, k, plan, c["index"] == "sq")
    _RUNS[(name, flags)] = dict(spec=c, flags=flags, D=D.cpu().numpy(), I=I.cpu().numpy(), fallbacks=fallbacks, st=st, plan=plan, model=model,
                                X=X, q=q, stats={})
    return _RUNS[(name, flags)]


def _check_lists(run):
    """(c) filter scores and (d) lists; returns the worst |s~ - st64| / acc."""
    c, st, m = run["spec"], run["st"], run["model"]
    N, k, cap = c["N"], c["k"], st["cap"]
    thr, eps = st["thr"].numpy().astype(np.float64), st["eps"].numpy().astype(np.float64)
    count = st["count"].numpy()
    rows_all, sc_all = st["rows"].numpy(), st["scores"].numpy().astype(np.float64)
    must, must_not = m.list_must(thr)
    Xe = R.f16_sat(run["X"]).astype(np.float32) if c["index"] == "sq" else run["X"]
    _, top = flat_ip_topk_fp64(run["q"], Xe, k)
    worst = 0.0
    for qi in range(c["Q"]):
        if count[qi] > cap:                        # an overflowed list is cut somewhere below cap (a wave that ran out of list space only
            continue                               # pushes the count past cap): the count is the signal, the entries say nothing
        n = int(count[qi])
        assert n <= rows_all.shape[1]
        rows, sc = rows_all[qi, :n], sc_all[qi, :n]
        assert (rows_all[qi, n:] == -1).all(), f"query {qi}: entries beyond the count"
        assert ((rows >= 0) & (rows < N)).all(), f"query {qi}: rows outside [0, N)"
        assert np.unique(rows).size == n, f"query {qi}: {n - np.unique(rows).size} rows listed twice"
        # (c) every entry's filter score: within acc of st64, hence within eps of the exact score
        err = np.abs(sc - m.st64[qi, rows])
        assert (err <= m.acc[qi, rows]).all(), f"query {qi}: filter score off by {(err / m.acc[qi, rows]).max():.3f} acc"
        assert (np.abs(sc - m.s64[qi, rows]) <= eps[qi]).all(), f"query {qi}: |s~ - s64| > eps"
        worst = max(worst, float((err / m.acc[qi, rows]).max()) if n else 0.0)
        listed = np.zeros(N, bool)
        listed[rows] = True
        main = ~m.in_sample
        assert (sc[main[rows]] >= thr[qi]).all(), f"query {qi}: a main-pass entry below thr"
        assert not (listed & must_not[qi] & main).any(), f"query {qi}: {(listed & must_not[qi] & main).sum()} main-pass rows listed below thr - acc"
        missing = must[qi] & ~listed
        assert not missing.any(), f"query {qi}: {missing.sum()} rows >= thr + acc not listed ({(missing & main).sum()} of the main pass), e.g. row {np.flatnonzero(missing)[:4]}"
        assert listed[top[qi]].all(), f"query {qi}: exact top-k rows missing from the list"
    return worst


def _check_case(run):
    c, st, m, plan = run["spec"], run["st"], run["model"], run["plan"]
    Q, k, N, cap = c["Q"], c["k"], c["N"], st["cap"]
    assert st["nq"] == Q and st["k"] == k and st["ntotal"] == N
    # the plan the host tests checked the preconditions for is the plan that ran
    want = R.expected_plan(N, c["D"], Q, k, c["has_shadow"], run["flags"], cus=torch.cuda.get_device_properties(0).multi_processor_count)
    assert plan == want, (plan, want)
    assert st["row_grouped"] is False
    # (b) eps
    eps = st["eps"].numpy().astype(np.float64)
    thr = st["thr"].numpy().astype(np.float64)
    assert (m.eps_ref <= eps).all(), f"eps below the bound: min ratio {(eps / m.eps_ref).min():.6f}"
    assert (eps <= m.eps_hi).all(), f"eps above the written safety factors: max ratio {(eps / m.eps_ref).max():.6f} > {m.eps_factor:.6f}"
    # (c), (d)
    worst_acc = _check_lists(run)
    # (e) T' = thr + 2 eps (fp64 sum of the two stored fp32 numbers; the stored thr = fl(T' - 2 eps) carries half an ulp: 2^-24 |thr|)
    lo, hi = m.threshold_bounds()
    T = thr + 2.0 * eps
    rnd = np.abs(thr) * 2.0 ** -24
    assert (T >= lo - rnd).all(), f"T' below the k-th group maximum by up to {(lo - T).max():.3e}"
    assert (T <= hi + rnd).all(), f"T' above the k-th sample score by up to {(T - hi).max():.3e}"
    # (f) band and fallback, with the library's own thr and eps
    count, flags, band = st["count"].numpy(), st["flags"].numpy(), st["band"].numpy()
    thr_s = np.minimum(thr, lo - rnd - 2.0 * eps)                       # sample rows may have entered at the group threshold
    list_lo, list_hi = m.list_count_bounds(thr, thr, thr_s)
    band_lo, band_hi = m.band_count_bounds(eps, eps)
    overflow = (band_lo > R.REF_CAND) | (list_lo > cap)
    assert set(np.flatnonzero(overflow).tolist()) == set(c["overflow"])
    benign = ~overflow
    assert (band_hi[benign] <= R.REF_CAND // st["nsplit"]).all() and (list_hi[benign] <= cap // 2).all()    # (host preconditions, with the GPU's own thr and eps)
    assert (flags[overflow] != 0).all(), "a query whose list or band must overflow was not flagged"
    assert (flags[benign] == 0).all(), f"{(flags[benign] != 0).sum()} queries flagged for the fallback without need"
    assert (count[benign] >= list_lo[benign]).all() and (count[benign] <= list_hi[benign]).all(), (count[benign], list_lo[benign], list_hi[benign])
    assert (band[benign] >= band_lo[benign]).all() and (band[benign] <= band_hi[benign]).all(), (band[benign], band_lo[benign], band_hi[benign])
    any_flag = st["any_flag"].numpy()
    for g in range(8):
        assert (any_flag[g] != 0) == bool((flags[g * 128:(g + 1) * 128] != 0).any()), f"any_flag[{g}] = {any_flag[g]}"
    assert run["fallbacks"] == int((flags != 0).sum())
    # (a) the result, last: a wrong stage is named by its own check above before it shows here
    Xe = R.f16_sat(run["X"]).astype(np.float32) if c["index"] == "sq" else run["X"]
    Dw, Iw = flat_ip_topk_fp64(run["q"], Xe, k)
    assert np.array_equal(run["I"], Iw + ID_BASE)
    assert np.array_equal(run["D"].view(np.int32), Dw.view(np.int32))
    run["stats"] = dict(acc=worst_acc, eps=float((eps / m.eps_ref).max()), eps_factor=m.eps_factor,
                        count=float((count[benign] / list_hi[benign]).max()) if benign.any() else 0.0,
                        band=float((band[benign] / band_hi[benign]).max()) if benign.any() else 0.0)
    print(f"\n{c['N']} x {c['D']}, {Q} queries, k = {k}: |s~ - st64| / acc <= {worst_acc:.4f}, eps / eps_ref <= {run['stats']['eps']:.6f}, "
          f"count / upper <= {run['stats']['count']:.4f}, band / upper <= {run['stats']['band']:.4f}, lists {count.min()}..{count.max()}, "
          f"band {band.min()}..{band.max()}, flagged {int((flags != 0).sum())}, plan {plan}")


@pytest.mark.parametrize("name", list(R.CASES))
def test_stages_against_the_fp64_model(name):
    _check_case(_run(name))


def test_chain_and_fused_launch_agree_on_eps():
    """The three-launch chain and the fused launch over the same index and queries: eps bit-equal (the same query_eps_block); both lists
    satisfy the list checks against their own thr (the two plans sample different blocks, so the lists themselves may differ)."""
    for name in ("fused_1_tile", "fused_7_tiles"):
        fused, chain = _run(name), _run(name, R.FILTER_SCORE_FREE | R.FUSED_NEVER)
        assert fused["st"]["fused"] and not chain["st"]["fused"]
        assert np.array_equal(fused["st"]["eps"].numpy().view(np.int32), chain["st"]["eps"].numpy().view(np.int32))
        _check_case(chain)
        _check_lists(fused)


def test_state_is_refused_when_no_lists_were_kept():
    from lightretriever_amd import FlatIPIndex, _lib
    X, q = R.case_data("wg_per_block_3_slices_ragged")
    idx = FlatIPIndex(X.shape[1], capacity=X.shape[0])
    idx.add(torch.tensor(X))
    idx.search_flags = 1                                                    # the score-matrix filter
    idx.search(torch.tensor(q), 3)
    with pytest.raises(_lib.LrxError, match="kept no candidate lists"):
        idx.last_chunk_state()
    small = FlatIPIndex(X.shape[1], capacity=4000)
    small.add(torch.tensor(X[:4000]))                                   # at most 4096 rows: the plain path
    small.search(torch.tensor(q), 3)
    with pytest.raises(_lib.LrxError, match="plain path"):
        small.last_chunk_state()
    idx.two_pass = False
    idx.search(torch.tensor(q), 3)
    with pytest.raises(_lib.LrxError, match="not a two-pass search"):
        idx.last_chunk_state()


def test_zz_worst_case_summary():
    """Over all cases: the largest |s~_gpu - st64| / acc, eps_gpu / eps_ref and count / upper prediction.  Each is a ratio against a term of
    the design's own error bound: <= 1 (eps: <= the written safety factor)."""
    runs = [_run(name) for name in R.CASES]
    for r in runs:
        if not r["stats"]:
            _check_case(r)
    acc = max(r["stats"]["acc"] for r in runs)
    eps = max(r["stats"]["eps"] for r in runs)
    cnt = max(r["stats"]["count"] for r in runs)
    band = max(r["stats"]["band"] for r in runs)
    print(f"\nstage tests, worst over {len(runs)} cases: |s~ - st64| / acc = {acc:.4f}, eps_gpu / eps_ref = {eps:.6f} "
          f"(allowed {max(r['stats']['eps_factor'] for r in runs):.6f}), list count / upper = {cnt:.4f}, band / upper = {band:.4f}")
    assert acc <= 1.0 and cnt <= 1.0 and band <= 1.0
    assert all(r["stats"]["eps"] <= r["stats"]["eps_factor"] for r in runs)
