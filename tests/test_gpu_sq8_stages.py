"""The stages of the 8-bit scalar-quantised search (k_sq8_prep, k_sq8_scan, k_sq8_select_rescore) one at a time, against the fp64 model of
sq8_stage_reference.py: what SQ8Index.last_chunk_state() finds in the workspace after one search per case -- the digit planes, scale, bias
and eps of k_sq8_prep, the filter scores and block maxima of k_sq8_scan -- and the (D, I) the rescoring makes of them.  The final result
alone hides a stage error behind the exact rescoring; the cases' preconditions are checked on the CPU (test_sq8_stage_reference_host.py)."""
import numpy as np
import pytest
import torch

import sq8_stage_reference as R
import sq8_yardstick as Y

pytestmark = pytest.mark.gpu

ID_BASE = 1000
_RUNS = {}


def run(name):
    """One search of the case (cached per process) -> what it returned and left behind, as host arrays."""
    if name in _RUNS:
        return _RUNS[name]
    from lightretriever_amd import SQ8Index, _lib
    lib = _lib.lib()
    c = R.case_spec(name)
    trained, codes, q = R.case_data(name)
    idx = SQ8Index(c["d"], c["qtype"], id_base=ID_BASE)
    idx.set_contents(torch.from_numpy(np.array(trained)), torch.from_numpy(np.array(codes)))
    qt = torch.from_numpy(np.array(q)).cuda()
    out = dict(case=c)
    if name == "padding":                                   # the same search before rows 300 .. 383 of the last block are filled
        D0, I0 = idx.search(qt, c["k"])
        out["clean"] = (D0.cpu().numpy(), I0.cpu().numpy(), idx.last_chunk_state()["blkmax"].numpy())
        pad = 384 - c["n"]
        dirty = np.concatenate([codes, R.padding_pattern(q, trained, pad)])
        blocked = idx.rows_to_blocked(torch.from_numpy(dirty))
        assert blocked.numel() == 384 * c["d"] <= idx._codes.numel()
        idx._codes[:blocked.numel()].copy_(blocked)
        assert idx.ntotal == c["n"] and torch.equal(idx.codes().cpu(), torch.from_numpy(np.array(codes)))
    torch.cuda.synchronize()
    lib.lrx_search_fallback_count(1)
    D, I = idx.search(qt, c["k"])
    torch.cuda.synchronize()
    out["fallbacks"] = int(lib.lrx_search_fallback_count(1))
    st = idx.last_chunk_state()
    out.update(D=D.cpu().numpy(), I=I.cpu().numpy(), st=st)
    if c["bad"]:
        good = R.good_queries(name)
        D1, I1 = idx.search(qt[torch.from_numpy(good).cuda()], c["k"])
        out["without_bad"] = (D1.cpu().numpy(), I1.cpu().numpy())
    q0, nq = st["q0"], st["nq"]
    out["chunk"] = None if (q0 == 0 and nq == c["Q"]) else (q0, nq)
    out["good"] = np.array([i - q0 for i in R.good_queries(name) if q0 <= i < q0 + nq], dtype=np.int64)   # within the chunk
    _RUNS[name] = out
    return out


def chunk_model(name):
    return R.case_model(name, run(name)["chunk"])


def device_prep(name):
    """(good, w, scale_dev, n_dev, bias_dev, eps_dev) of the chunk's good queries, fp64 / int64 / fp32 host arrays."""
    r = run(name)
    g, st = r["good"], r["st"]
    return (g, chunk_model(name).w[g], st["scale"].numpy()[g], st["n"].numpy().astype(np.int64)[g], st["bias"].numpy()[g], st["eps"].numpy()[g])


def device_filter(name):
    """(v, isum) of the model filter score evaluated on the DEVICE's scale, digits and bias, good queries x rows."""
    g, _, scale, n, bias, _ = device_prep(name)
    m = chunk_model(name)
    if np.array_equal(n, m.n[g]):
        isum = m.isum[g]
        return scale[:, None] * isum + bias[:, None], isum
    return R.filter_scores(scale, n, bias, R.centred(m.codes))


def worst_ratio(name):
    """max |score - s64| / eps_dev over the good queries and rows of the chunk (0 / 0 = 0)."""
    r = run(name)
    g, _, _, _, _, eps = device_prep(name)
    m = chunk_model(name)
    err = np.abs(r["st"]["scores"].numpy()[g, :m.rows].astype(np.float64) - m.s64[g])
    e = eps.astype(np.float64)[:, None]
    assert (err[np.broadcast_to(e == 0, err.shape)] == 0).all()
    return float((err / np.where(e > 0, e, 1.0)).max()), err, e


def eps_reference(name):
    g, w, scale, n, _, _ = device_prep(name)
    m = chunk_model(name)
    return R.eps_of(R.eps_terms(m.q[g], m.trained, w, scale, n))


def test_state_is_refused_before_the_first_search_and_layout_matches_the_run():
    from lightretriever_amd import SQ8Index, _lib
    idx = SQ8Index(64)
    with pytest.raises(_lib.LrxError, match="no search has run"):
        idx.last_chunk_state()
    r = run("two_chunks")
    st = r["st"]
    assert (st["q0"], st["nq"], st["qpad"], st["row0"], st["rows"], st["k"], st["ntotal"]) == (128, 1, 16, 0, 500, 10, 500)
    assert st["layout"]["qc"] == 128 and st["layout"]["qpad"] == 128 and st["layout"]["ld"] == 512
    assert st["hi"].shape == (16, 256) and st["n"].shape == (1, 256) and st["scores"].shape == (1, 512) and st["blkmax"].shape == (1, 4)
    st = run("d1024")["st"]
    assert (st["q0"], st["nq"], st["qpad"]) == (0, 128, 128) and st["scores"].shape == (128, 1024) and st["blkmax"].shape == (128, 8)


@pytest.mark.parametrize("name", list(R.CASES))
def test_digits(name):
    r = run(name)
    st, nq = r["st"], r["st"]["nq"]
    hi, lo = st["hi"].numpy().astype(np.int64), st["lo"].numpy().astype(np.int64)
    tiles = -(-nq // 16)
    assert st["qpad"] == hi.shape[0] == 16 * (1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 8)
    assert (np.abs(hi) <= 127).all() and (lo >= -64).all() and (lo <= 63).all()
    assert not hi[nq:].any() and not lo[nq:].any()                            # the padding queries' tiles
    assert np.array_equal(st["n"].numpy(), (128 * hi + lo)[:nq])
    g, w, scale, n, _, _ = device_prep(name)
    wmax = np.abs(w).max(1)
    assert (scale * R.NMAX >= wmax).all() and (scale * R.NMAX <= wmax * (1 + 2.0 ** -21)).all()
    pos = scale > 0
    assert not n[~pos].any()
    x = w[pos] / scale[pos][:, None]
    assert (np.abs(np.rint(x)) <= R.NMAX).all()                               # (the clamp never acts)
    near_half = np.abs(x - np.floor(x) - 0.5) < 2.0 ** -40
    assert ((n[pos] == np.rint(x)) | (near_half & (np.abs(n[pos] - x) <= 0.5 + 2.0 ** -40))).all()
    for z in r["case"]["zero"]:
        assert scale[z] == 0 and not n[z].any()


@pytest.mark.parametrize("name", list(R.CASES))
def test_bias(name):
    g, w, _, _, bias, _ = device_prep(name)
    m = chunk_model(name)
    assert (np.abs(bias - m.bias[g]) <= R.bias_tolerance(m.q[g], m.trained, w)).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_filter_scores_and_block_maxima(name):
    r = run(name)
    g, _, scale, _, bias, _ = device_prep(name)
    m = chunk_model(name)
    rows = m.rows
    assert r["st"]["rows"] == rows
    sc = r["st"]["scores"].numpy()[g]
    v, isum = device_filter(name)
    tol = 2.0 ** -24 * np.abs(v) + 2.0 ** -52 * (np.abs(scale[:, None] * isum) + np.abs(bias)[:, None]) + 2.0 ** -149
    assert (np.abs(sc[:, :rows].astype(np.float64) - v) <= tol).all()
    # block maxima: the maximum of the matrix over each block's rows < n (equal values; equal non-zero floats have equal bits)
    nblk = -(-rows // 128)
    padded = np.full((len(g), nblk * 128), -np.inf, np.float32)
    padded[:, :rows] = sc[:, :rows]
    bm = r["st"]["blkmax"].numpy()[g]
    assert bm.shape == (len(g), nblk) and np.array_equal(bm, padded.reshape(len(g), nblk, 128).max(2))
    if name == "padding":                                                      # the filled rows 300 .. 383 change neither maxima nor results
        D0, I0, bm0 = r["clean"]
        assert np.array_equal(bm0.view(np.int32), r["st"]["blkmax"].numpy().view(np.int32))
        assert np.array_equal(I0, r["I"]) and np.array_equal(D0.view(np.int32), r["D"].view(np.int32))
        assert (sc[:, rows:384].max(1) > bm.max(1)).all()                      # ... although they do beat every stored row in the matrix


@pytest.mark.parametrize("name", list(R.CASES))
def test_bound(name):
    g, _, _, _, _, eps = device_prep(name)
    ratio, err, e = worst_ratio(name)
    assert (err <= e).all()
    ref = eps_reference(name)
    assert (np.abs(eps.astype(np.float64) - ref.astype(np.float64)) <= 2 * np.spacing(ref).astype(np.float64)).all(), (eps, ref)
    if name in R.ALIGNED:                                                      # the test can see a bound that is too small
        assert 0.9 <= ratio <= 1, ratio


@pytest.mark.parametrize("name", list(R.CASES))
def test_results(name):
    r = run(name)
    c = r["case"]
    m = R.case_model(name)                                                     # every query of the call, not the last chunk only
    good = R.good_queries(name)
    Dw, Iw = Y.topk(m.s[good], c["k"])
    Iw = np.where(Iw >= 0, Iw + ID_BASE, -1)
    D, I = r["D"], r["I"]
    assert np.array_equal(I[good], Iw)
    nz = np.array([i for i, qi in enumerate(good) if qi not in c["zero"]], dtype=np.int64)
    assert np.array_equal(D[good][nz].view(np.int32), Dw[nz].view(np.int32))
    for z in c["zero"]:
        assert np.array_equal(I[z], ID_BASE + np.arange(c["k"])) and not D[z].view(np.int32).any()      # rows 0 .. 9, score +0
    assert r["fallbacks"] == len(c["zero"])                                    # the streaming form: the all-tie band of the zero query only
    if name in R.BAND_EDGE:                                                    # U, found only because the band is 2 eps wide, comes first
        U, _ = R.band_edge_rows(c)
        assert np.array_equal(I[:, 0], U + ID_BASE)
    if c["n"] < c["k"]:
        assert (I[:, c["n"]:] == -1).all() and (D[:, c["n"]:] == -np.finfo(np.float32).max).all()
    for b in c["bad"]:                                                         # a non-finite query: distinct valid rows or -1
        ids = I[b][I[b] >= 0]
        assert ((I[b] == -1) | ((I[b] >= ID_BASE) & (I[b] < ID_BASE + c["n"]))).all() and len(set(ids.tolist())) == len(ids)
    if c["bad"]:
        D1, I1 = r["without_bad"]
        assert np.array_equal(I[good], I1) and np.array_equal(D[good].view(np.int32), D1.view(np.int32))


def test_worst_case_summary():
    """Worst |score - s64| / eps_dev over every pair of a case's last chunk, and the range of eps_dev / eps_ref.  Measured on MI355X
    (eps_dev / eps_ref = 1.00000000 in every case: the two agree to the bit):
        d64 0.3064, d64_uniform 0.2978, d192 0.1632, d576_uniform 0.1207, d1024 0.0811, two_chunks 0.1171 (its last chunk: one query),
        one_row 0.0066, rows_127 0.2933, rows_128 0.2896, rows_129 0.3485, grid_stride 0.4327,
        aligned_d64 0.9847, aligned_d64_uniform 0.9850, aligned_d256 0.9862, aligned_d256_uniform 0.9859,
        band_edge 0.9792, band_edge_uniform 0.9805, offset 0.0299, subnormal 0.2175, const_cols 0.2025, padding 0.3130,
        zero_query 0.3198, nonfinite_query 0.2779 (the finite queries).
    Random rows stay below half of the bound; only the sign-aligned rows (and the rows of band_edge built from them) show whether it is tight.
    Nothing tighter than ratio <= 1 is asserted here."""
    print()
    for name in R.CASES:
        g, _, _, _, _, eps = device_prep(name)
        ratio, _, _ = worst_ratio(name)
        ref = eps_reference(name).astype(np.float64)
        rel = np.where(ref > 0, eps.astype(np.float64) / np.where(ref > 0, ref, 1.0), 1.0)
        print(f"{name:22s} worst |score - s64| / eps_dev = {ratio:.4f}   eps_dev / eps_ref in [{rel.min():.8f}, {rel.max():.8f}]")
        assert ratio <= 1
