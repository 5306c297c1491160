"""Binary flat index (BinaryFlatIndex, lrx_binary_ip_search / lrx_binary_hamming_search / lrx_binary_pack_rows, torch.ops.lrx.binary_topk,
FaissBinaryIndex / BinaryFaissSearch / HybridSearch(faiss_search_map="binary")) against tests/binary_yardstick.py.  Every comparison is exact:
packed bytes, int32 Hamming distances, ids and the BITS of the fp32 rerank scores."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binary_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- the yardstick's arithmetic on the GPU for the large shapes (checked against the numpy functions below) -------------------------------
def popcount64(x):
    x = x - ((x >> 1) & 0x5555555555555555)
    x = (x & 0x3333333333333333) + ((x >> 2) & 0x3333333333333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0F
    return (x * 0x0101010101010101) >> 56 & 0xFF


def hamming_t(qb, xb):
    """packed uint8 CUDA tensors [Q, B], [n, B] -> int32 [Q, n]."""
    B = xb.shape[1]
    pad = -B % 8
    if pad:
        qb, xb = torch.nn.functional.pad(qb, (0, pad)), torch.nn.functional.pad(xb, (0, pad))
    qw, xw = qb.contiguous().view(torch.int64), xb.contiguous().view(torch.int64)
    H = torch.empty(qb.shape[0], xb.shape[0], dtype=torch.int32, device=xb.device)
    for i in range(qb.shape[0]):
        H[i] = popcount64(xw ^ qw[i][None, :]).sum(dim=1).int()
    return H


def pack_t(x, threshold=0.0):
    """float CUDA tensor [n, d] -> packed uint8 [n, d / 8] (np.packbits order)."""
    w = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.int32, device=x.device)
    return ((x > threshold).view(x.shape[0], -1, 8).int() * w).sum(dim=2).to(torch.uint8)


def hamming_topk_t(H, k):
    Q, n = H.shape
    kk = min(k, n)
    key = (H.long() << 32) | torch.arange(n, device=H.device)[None, :]
    top = torch.topk(key, kk, dim=1, largest=False, sorted=True).values
    D = torch.full((Q, k), Y.INT_MAX, dtype=torch.int32, device=H.device)
    I = torch.full((Q, k), -1, dtype=torch.int64, device=H.device)
    D[:, :kk], I[:, :kk] = (top >> 32).int(), top & 0xFFFFFFFF
    return D, I


def rerank_t(q, xb, C, k, scores=None):
    """q fp32 [Q, d], packed rows xb, candidate rows C int64 [Q, kk] -> (D fp32 [Q, k], I): fp64 sums of +-q, rounded once; score desc, row asc."""
    Q, kk = C.shape
    D = torch.full((Q, k), -Y.FLT_MAX, dtype=torch.float32, device=q.device)
    I = torch.full((Q, k), -1, dtype=torch.int64, device=q.device)
    shifts = torch.arange(7, -1, -1, device=q.device)
    for i in range(Q):
        c = torch.sort(C[i]).values
        sign = ((xb[c][:, :, None].int() >> shifts) & 1).reshape(kk, -1).double() * 2 - 1
        s = (sign * q[i].double()[None, :]).sum(dim=1).float() if scores is None else scores(q[i], sign)
        v, o = torch.sort(s, descending=True, stable=True)
        m = min(k, kk)
        D[i, :m], I[i, :m] = v[:m], c[o[:m]]
    return D, I


def assert_same(got, want):
    Dg, Ig = got
    Dw, Iw = want
    assert torch.equal(Ig, Iw)
    assert Dg.dtype == Dw.dtype and torch.equal(Dg.view(torch.int32), Dw.view(torch.int32))


def random_packed(n, d, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (n, d // 8), dtype=torch.uint8, device="cuda", generator=g)


def build(xb, d, chunk=1 << 18, **kw):
    from lightretriever_amd import BinaryFlatIndex
    idx = BinaryFlatIndex(d, **kw)
    for s in range(0, xb.shape[0], chunk):
        idx.add(xb[s:s + chunk])
    return idx


def grid_q(Q, d, seed=1):
    return torch.from_numpy(Y.grid_queries(np.random.default_rng(seed), Q, d)).cuda()


def test_gpu_yardstick_helpers_equal_the_numpy_yardstick():
    rng = np.random.default_rng(0)
    for d in (64, 1544):
        x = rng.standard_normal((300, d)).astype(np.float32)
        q = Y.grid_queries(rng, 5, d)
        xb, qb = Y.pack(x), Y.pack(q)
        assert np.array_equal(pack_t(torch.from_numpy(x).cuda()).cpu().numpy(), xb)
        H = hamming_t(torch.from_numpy(qb).cuda(), torch.from_numpy(xb).cuda())
        assert np.array_equal(H.cpu().numpy(), Y.hamming(qb, xb))
        for k in (7, 400):
            D, I = hamming_topk_t(H, k)
            Dn, In = Y.hamming_topk(H.cpu().numpy(), k)
            assert np.array_equal(D.cpu().numpy(), Dn) and np.array_equal(I.cpu().numpy(), In)
        _, C = hamming_topk_t(H, 50)
        D, I = rerank_t(torch.from_numpy(q).cuda(), torch.from_numpy(xb).cuda(), C, 20)
        Dn, In = Y.search(q, xb, 20, binary_k=50)
        assert np.array_equal(I.cpu().numpy(), In) and np.array_equal(D.cpu().numpy().view(np.int32), Dn.view(np.int32))


# ---- pack ------------------------------------------------------------------------------------------------------------------------------------
def special_rows(n, d, thr, seed=0):
    """random rows with +-0, NaN, +-inf and values equal to the threshold sprinkled in."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    t = np.broadcast_to(np.asarray(thr, np.float32), (d,))
    for v in (0.0, -0.0, np.nan, np.inf, -np.inf):
        x[rng.random((n, d)) < 0.03] = v
    m = rng.random((n, d)) < 0.1
    x[m] = np.broadcast_to(t, (n, d))[m]
    return x


@pytest.mark.parametrize("d", [64, 1544, 2048])
@pytest.mark.parametrize("vector_threshold", [False, True])
def test_pack_equals_np_packbits(d, vector_threshold):
    from lightretriever_amd import BinaryFlatIndex
    n = 1000
    thr = np.random.default_rng(7).standard_normal(d).astype(np.float32) * 0.5 if vector_threshold else 0.25
    x = special_rows(n, d, thr)
    want = Y.pack(x, thr)
    assert want.shape == (n, d // 8)
    idx = BinaryFlatIndex(d, threshold=thr)
    idx.add(x[:300])                                               # numpy rows
    idx.add(torch.from_numpy(x[300:777]).cuda())                   # CUDA rows, a start that is not a block boundary
    slot = idx.append_slot(n - 777)
    assert slot.shape == (n - 777, d) and slot.dtype == torch.float32
    slot.copy_(torch.from_numpy(x[777:]))
    idx.commit(n - 777)
    assert idx.ntotal == n and idx._stage is None
    assert np.array_equal(idx.codes().cpu().numpy(), want)
    assert np.array_equal(idx.reconstruct_n(290, 20).cpu().numpy(), want[290:310])
    # rows that arrive packed, and the default threshold 0 with -0.0 / NaN / 0.0 rows
    idx2 = BinaryFlatIndex(d)
    idx2.add(want[:500])
    idx2.add(torch.from_numpy(want[500:]))
    assert np.array_equal(idx2.codes().cpu().numpy(), want)
    idx3 = BinaryFlatIndex(d)
    idx3.add(x)
    assert np.array_equal(idx3.codes().cpu().numpy(), Y.pack(x))
    with pytest.raises(ValueError):
        idx.add(np.zeros((3, d + 8), np.float32))
    with pytest.raises(ValueError):
        BinaryFlatIndex(100)


def test_reset_and_regrowth_keep_the_rows():
    d = 256
    xb = random_packed(5000, d)
    idx = build(xb, d, chunk=700)                                  # grows several times
    assert torch.equal(idx.codes(), xb)
    idx.reset()
    assert idx.ntotal == 0
    idx.add(xb[100:200])
    assert torch.equal(idx.codes(), xb[100:200])


def test_encoder_writes_a_chunk_through_index_in_place():
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd.retriever import BinaryFaissSearch, FaissBinaryIndex, FlatIPFaissSearch
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, hm, model = build_stack(cfg_o, w)
    corpus = synth_corpus(np.random.default_rng(0), 50)
    docs = list(corpus.values())
    dim = enc.cfg.hidden_size
    b = BinaryFaissSearch(model, batch_size=16)
    b._index_in_place(docs, list(range(len(docs))), dim)
    fl = FlatIPFaissSearch(model, batch_size=16)
    fl._index_in_place(docs, list(range(len(docs))), dim)
    bidx = b.faiss_index.index
    assert isinstance(b.faiss_index, FaissBinaryIndex) and bidx.ntotal == len(docs) and bidx._stage is None
    assert np.array_equal(bidx.codes().cpu().numpy(), Y.pack(fl.faiss_index.index.vectors.cpu().numpy()))


# ---- Hamming top-k and rerank ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,nq,k,binary_k", [
    (1_000_000, 2048, 100, 100, 1000),
    (10_000_000, 256, 16, 100, 1000),
    (100_000, 2048, 1000, 1000, 1000),
    (1_000_000, 2048, 1, 10, 1000),
    (300_000, 1544, 7, 50, 2048),          # d % 128 != 0, the largest binary_k
    (200_000, 4096, 9, 20, 300),           # the 16-query tile
    (20_000, 8192, 5, 10, 100),            # the 4-query tile with a histogram over 64 KiB
])
def test_hamming_topk_and_rerank_equal_the_yardstick(n, d, nq, k, binary_k):
    xb = random_packed(n, d)
    idx = build(xb, d)
    q = grid_q(nq, d)
    H = hamming_t(pack_t(q), xb)
    assert_same(idx.search(q, binary_k, rerank=False), hamming_topk_t(H, binary_k))
    assert_same(idx.search(q, k, rerank=False), hamming_topk_t(H, k))
    _, C = hamming_topk_t(H, binary_k)
    assert_same(idx.search(q, k, binary_k=binary_k), rerank_t(q, xb, C, k))


def test_tiny_shard_pads_beyond_ntotal():
    d = 128
    xb = random_packed(37, d)
    idx = build(xb, d, id_base=1000)
    q = grid_q(3, d)
    H = hamming_t(pack_t(q), xb)
    D, I = idx.search(q, 50, rerank=False)
    Dw, Iw = hamming_topk_t(H, 50)
    assert torch.equal(D, Dw) and torch.equal(I, torch.where(Iw >= 0, Iw + 1000, Iw))
    assert D[:, 37:].eq(Y.INT_MAX).all() and I[:, 37:].eq(-1).all()
    D, I = idx.search(q, 50, binary_k=60)
    Dw, Iw = rerank_t(q, xb, hamming_topk_t(H, 37)[1], 50)
    assert torch.equal(D.view(torch.int32), Dw.view(torch.int32)) and torch.equal(I, torch.where(Iw >= 0, Iw + 1000, Iw))
    assert D[:, 37:].eq(-Y.FLT_MAX).all() and I[:, 37:].eq(-1).all()
    from lightretriever_amd import BinaryFlatIndex
    empty = BinaryFlatIndex(d)
    D, I = empty.search(q, 5)
    assert D.eq(-Y.FLT_MAX).all() and I.eq(-1).all()
    D, I = empty.search(q, 5, rerank=False)
    assert D.eq(Y.INT_MAX).all() and I.eq(-1).all()


def test_clusters_of_identical_rows_the_lowest_row_rule_decides():
    d, n_clusters, copies = 512, 20, 10_000
    base = random_packed(n_clusters, d, seed=3)
    perm = torch.randperm(n_clusters * copies, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    xb = base.repeat_interleave(copies, dim=0)[perm]               # every cutoff bin holds 10 000 ties
    idx = build(xb, d)
    q = grid_q(12, d, seed=5)
    q[0] = (((base[0][:, None].int() >> torch.arange(7, -1, -1, device="cuda")) & 1).reshape(-1).float() * 2 - 1)   # cluster 0 at distance 0
    H = hamming_t(pack_t(q), xb)
    for k in (1000, 2048, 1):
        assert_same(idx.search(q, k, rerank=False), hamming_topk_t(H, k))
    _, C = hamming_topk_t(H, 1000)
    assert_same(idx.search(q, 100, binary_k=1000), rerank_t(q, xb, C, 100))


def test_ordinary_queries_equal_the_fp64_matmul():
    """Normalised random queries (not on the grid): the yardstick is torch's fp64 matmul of q with the +-1 rows, rounded to fp32 -- ids and bits."""
    n, d, nq, k, binary_k = 200_000, 2048, 50, 100, 1000
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(n, d, device="cuda", generator=g)
    q = torch.randn(nq, d, device="cuda", generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    from lightretriever_amd import BinaryFlatIndex
    idx = BinaryFlatIndex(d, capacity=n)
    idx.add(x)
    xb = pack_t(x)
    assert torch.equal(idx.codes(), xb)
    _, C = hamming_topk_t(hamming_t(pack_t(q), xb), binary_k)
    assert_same(idx.search(q, k, binary_k=binary_k), rerank_t(q, xb, C, k, scores=lambda qi, sign: (sign @ qi.double()).float()))


def test_thresholds_row_map_and_the_torch_op():
    from lightretriever_amd import torch_ops  # noqa: F401
    n, d, nq, k = 50_000, 768, 33, 40
    xb = random_packed(n, d)
    idx = build(xb, d, id_base=7)
    q = grid_q(nq, d)
    tvec = torch.from_numpy(np.random.default_rng(2).integers(-1024, 1025, size=d) / 1024.0).float().cuda()
    row_map = torch.randperm(n, device="cuda") + 5_000_000_000
    for thr in (0, 0.5, tvec):
        H = hamming_t(pack_t(q, thr), xb)
        Dw, Iw = rerank_t(q, xb, hamming_topk_t(H, 200)[1], k)
        D, I = idx.search(q, k, binary_k=200, threshold=thr)
        assert torch.equal(D.view(torch.int32), Dw.view(torch.int32)) and torch.equal(I, Iw + 7)
        D, I = idx.search(q, k, binary_k=200, threshold=thr, row_map=row_map)
        assert torch.equal(D.view(torch.int32), Dw.view(torch.int32)) and torch.equal(I, row_map[Iw])
        tt = thr if isinstance(thr, torch.Tensor) else torch.tensor([float(thr)])
        assert_same(torch.ops.lrx.binary_topk(q, idx._codes, n, k, 200, True, tt, 7, None), idx.search(q, k, binary_k=200, threshold=thr))
        assert_same(torch.ops.lrx.binary_topk(q, idx._codes, n, k, 200, False, tt, 0, row_map), idx.search(q, k, rerank=False, threshold=thr, row_map=row_map))
    assert_same(torch.ops.lrx.binary_topk(q, idx._codes, n, k), (idx.search(q, k)[0], idx.search(q, k)[1] - 7))
    for bad in (dict(k=0), dict(k=11, binary_k=10), dict(k=5, binary_k=2049)):
        with pytest.raises(ValueError):
            idx.search(q, **bad)
    with pytest.raises(ValueError):
        idx.search(q, 2049, rerank=False)
    with pytest.raises(NotImplementedError):
        idx.search(q, 5, score_function="cos_sim")
    with pytest.raises(RuntimeError):
        torch.ops.lrx.binary_topk(q, idx._codes[:100], n, k)


def test_save_load_round_trip(tmp_path):
    from lightretriever_amd import BinaryFlatIndex
    n, d = 70_001, 1544
    xb = random_packed(n, d)
    idx = build(xb, d)
    path = str(tmp_path / "a.bin.faiss")
    idx.save(path, chunk_rows=30_000)
    assert os.path.getsize(path) == 33 + n * d // 8
    back = BinaryFlatIndex.load(path, chunk_rows=25_000)
    assert back.d == d and back.ntotal == n and torch.equal(back.codes(), xb) and torch.equal(back.reconstruct_n(0, n), xb)
    q = grid_q(20, d)
    assert_same(back.search(q, 30, binary_k=500), idx.search(q, 30, binary_k=500))
    assert_same(back.search(q, 30, rerank=False), idx.search(q, 30, rerank=False))


def test_resident_memory_is_one_bit_per_dimension():
    n, d = 1_000_000, 2048
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    from lightretriever_amd import BinaryFlatIndex
    idx = BinaryFlatIndex(d, capacity=n)
    for s in range(0, n, 1 << 18):
        idx.add(random_packed(min(1 << 18, n - s), d, seed=s))
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated() - before
    assert idx._codes.numel() == -(-n // 128) * 128 * d // 8
    assert resident <= idx._codes.numel() + (1 << 20)


# ---- the searchers over a corpus in several chunks ----------------------------------------------------------------------------------------
class TableModel:
    """encode_corpus / encode_queries by lookup: the embeddings are the test's own."""

    def __init__(self, table):
        self.table = table

    def _rows(self, texts):
        return torch.stack([self.table[t["text"] if isinstance(t, dict) else t] for t in texts]).cuda()

    def encode_queries(self, queries, **kw):
        return {"dense_reps": self._rows(queries)}

    def encode_corpus(self, corpus, **kw):
        return {"dense_reps": self._rows(corpus)}


def test_searchers_over_several_chunks_equal_the_yardstick(tmp_path):
    from lightretriever_amd.retriever import BinaryFaissSearch, HybridSearch
    rng = np.random.default_rng(9)
    d, n, top_k, binary_k, chunk = 64, 90, 12, 20, 32
    emb = Y.grid_queries(rng, n, d)
    emb[[6, 7, 40, 41, 42, 70, 71, 72]] = emb[5]                  # nine identical documents, three in each chunk: equal bits and equal scores
    ids = [f"d{i:03d}" for i in rng.permutation(n)]
    corpus = {pid: {"text": "x" * (200 - j) + pid} for j, pid in enumerate(ids)}      # longest first = this order
    qs = {"q0": "query zero", "q1": "query one", ids[7]: "query that is a document", "q3": "query three"}
    qemb = Y.grid_queries(rng, len(qs), d)
    qemb[1] = emb[5]                                              # scores that tie across the copies
    qemb[2] = emb[7]
    table = {corpus[pid]["text"]: torch.from_numpy(emb[j]) for j, pid in enumerate(ids)}
    table.update({t: torch.from_numpy(qemb[i]) for i, t in enumerate(qs.values())})
    model = TableModel(table)

    def want(ignore_identical_ids, threshold=0, top_k=top_k):
        out = {}
        for i, qid in enumerate(qs):
            hits = []
            for s in range(0, n, chunk):
                xb = Y.pack(emb[s:s + chunk], threshold)
                D, I = Y.search(qemb[i:i + 1], xb, top_k, binary_k=binary_k, threshold=threshold)
                hits += [(float(sc), ids[s + j]) for sc, j in zip(D[0].tolist(), I[0].tolist()) if j >= 0 and not (ignore_identical_ids and ids[s + j] == qid)]
            hits.sort(key=lambda h: (h[0], h[1]), reverse=True)   # score descending, equal scores: the larger pid first (the reference's heap)
            out[qid] = {pid: sc for sc, pid in hits[:top_k]}
        return out
    for ign in (False, True):
        s = BinaryFaissSearch(model, batch_size=8, corpus_chunk_size=chunk, binary_k=binary_k)
        assert s.search(corpus, qs, top_k=top_k, ignore_identical_ids=ign) == want(ign)
        h = HybridSearch(model, batch_size=8, corpus_chunk_size=chunk, faiss_search_map="binary", binary_k=binary_k)
        assert h.search(corpus, qs, top_k=top_k, ignore_identical_ids=ign) == want(ign)
    for small in (2, 4):      # the cut falls inside the nine copies: the lower rows survive each chunk, the larger pids survive the merge
        s = BinaryFaissSearch(model, batch_size=8, corpus_chunk_size=chunk, binary_k=binary_k)
        got = s.search(corpus, qs, top_k=small)
        assert got == want(False, top_k=small) and len(set(got["q1"].values())) == 1 and len(got["q1"]) == small
    h = HybridSearch(model, batch_size=8, corpus_chunk_size=chunk, faiss_search_map="binary", binary_k=binary_k, threshold=0.5)
    assert h.search(corpus, qs, top_k=top_k) == want(False, 0.5)
    with pytest.raises(ValueError, match="binary_k"):
        BinaryFaissSearch(model, batch_size=8, binary_k=5).search(corpus, qs, top_k=6)
    # index / save / load of the searcher, rerank=False through FaissBinaryIndex
    s = BinaryFaissSearch(model, batch_size=8, binary_k=binary_k)
    s.index(torch.from_numpy(emb), ids)
    s.save(str(tmp_path), "p")
    assert os.path.exists(tmp_path / "p.bin.faiss") and os.path.exists(tmp_path / "p.bin.tsv")
    t = BinaryFaissSearch(model, batch_size=8, binary_k=binary_k)
    t.load(str(tmp_path), "p")
    qd = torch.from_numpy(qemb).cuda()
    assert t.retrieve_with_emb(qd, list(qs), top_k) == s.retrieve_with_emb(qd, list(qs), top_k)
    D, I = s.faiss_index.search(qd, 5, rerank=False)
    Dw, Iw = Y.hamming_topk(Y.hamming(Y.pack(qemb), Y.pack(emb)), 5)
    assert D.dtype == torch.int32 and np.array_equal(D.cpu().numpy(), Dw) and np.array_equal(I.cpu().numpy(), Iw)
