"""CPU tests of the host-side logic: collator vs the fixture produced by the reference's EncodeCollator, text formatting,
corpus sorting, shard assignment, pair packing, and the N>1 exchange over gloo (world_size 2)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import lrx_oracle as O
from helpers import GOLDEN


@pytest.fixture(scope="module")
def tok():
    from transformers import PreTrainedTokenizerFast
    return PreTrainedTokenizerFast.from_pretrained(os.path.join(GOLDEN, "tok"))


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(GOLDEN, "collator.json")))


def test_doc_collator_matches_reference_tokens(tok, fx):
    from lightretriever_amd.modeling import EncodeCollator
    coll = EncodeCollator(tok, encode_is_query=False, q_max_len=fx["q_max_len"], p_max_len=fx["p_max_len"], return_padded=True)
    out = coll(fx["docs"])
    ids, mask = np.array(fx["doc_input_ids"]), np.array(fx["doc_attention_mask"])
    np.testing.assert_array_equal(out["padded_input_ids"].numpy(), ids)
    np.testing.assert_array_equal(out["padded_attention_mask"].numpy(), mask)
    nested, _, _, cu, max_len = O.pack_padded(ids, mask)             # packed output == the reference's unpad of its own batch
    np.testing.assert_array_equal(out["input_ids"].numpy(), nested)
    np.testing.assert_array_equal(out["cu_seqlens"].numpy(), cu)
    assert out["max_seqlen"] == max_len == fx["p_max_len"]
    assert out["input_ids"].dtype == torch.int32 and out["cu_seqlens"].dtype == torch.int32
    # prompt column is string-prepended
    p = coll([fx["doc_prompted"]])
    np.testing.assert_array_equal(p["padded_input_ids"].numpy(), np.array(fx["doc_prompted_input_ids"]))


def test_query_collator_matches_reference_tokens(tok, fx):
    from lightretriever_amd.modeling import EncodeCollator
    coll = EncodeCollator(tok, encode_is_query=True, q_max_len=fx["q_max_len"], p_max_len=fx["p_max_len"])
    out = coll(fx["queries"])
    np.testing.assert_array_equal(out["nonctx_tok_emb_input_ids"].numpy(), np.array(fx["qry_nonctx_input_ids"]))
    np.testing.assert_array_equal(out["nonctx_tok_emb_offsets"].numpy(), np.array(fx["qry_nonctx_offsets"]))
    assert out["nonctx_tok_emb_input_ids"].dtype == torch.int64


def test_query_collator_lm_inputs_match_reference_tokens(tok):
    """Round 5: queries that go through the LM (symmetric dense vector, input-embedding bag): `prompt + text` with specials, truncation to
    q_max_len -- the packed form of the reference collator's input_ids / attention_mask (exact_search_base.py:333-345), next to the
    EmbeddingBag fields when both are asked for."""
    from helpers import load_query_modes
    from lightretriever_amd.modeling import EncodeCollator, LrxExactSearchModel
    _, _, g, meta = load_query_modes()
    items = LrxExactSearchModel(model=None, tokenizer=tok).parse_texts(meta["queries"], prompt=meta["prompt"])
    q_max_len = int(g["q_max_len"])
    out = EncodeCollator(tok, encode_is_query=True, q_max_len=q_max_len, p_max_len=64, noncontextual_query_embedding=False)(items)
    nested, _, _, cu, max_len = O.pack_padded(g["input_ids"], g["attention_mask"])
    np.testing.assert_array_equal(out["input_ids"].numpy(), nested)
    np.testing.assert_array_equal(out["cu_seqlens"].numpy(), cu)
    assert out["max_seqlen"] == max_len == q_max_len and "nonctx_tok_emb_input_ids" not in out
    both = EncodeCollator(tok, encode_is_query=True, q_max_len=q_max_len, p_max_len=64, noncontextual_query_embedding=True, query_lm_inputs=True)(items)
    np.testing.assert_array_equal(both["input_ids"].numpy(), nested)
    np.testing.assert_array_equal(both["nonctx_tok_emb_input_ids"].numpy(), g["nonctx_ids"])
    np.testing.assert_array_equal(both["nonctx_tok_emb_offsets"].numpy(), g["nonctx_offsets"])
    bag_only = EncodeCollator(tok, encode_is_query=True, q_max_len=q_max_len, p_max_len=64, noncontextual_query_embedding=True)(items)
    assert set(bag_only) == {"nonctx_tok_emb_input_ids", "nonctx_tok_emb_offsets"}
    bare = EncodeCollator(tok, encode_is_query=True, q_max_len=q_max_len, p_max_len=64, noncontextual_query_embedding=False)(meta["queries"])
    np.testing.assert_array_equal(bare["input_ids"].numpy(), O.pack_padded(g["input_ids_noprompt"], g["attention_mask_noprompt"])[0])


def test_format_text_rules():
    from lightretriever_amd.modeling import format_text
    assert format_text({"title": "T", "text": "x"}) == "T x"
    assert format_text({"title": "", "text": "x"}) == "x"
    assert format_text({"text": "x", "prompt": "p: "}) == "x"
    assert format_text({"title": "T", "text": "x", "prompt": "p: "}, prepend_prompt=True) == "p: T x"


def test_parse_texts_prompt_rules(tok):
    from lightretriever_amd.modeling import LrxExactSearchModel
    m = LrxExactSearchModel(model=None, tokenizer=tok)
    assert m.parse_texts(["a", "b"], prompt="P ") == [{"text": "a", "prompt": "P "}, {"text": "b", "prompt": "P "}]
    assert m.parse_texts([{"text": "a", "prompt": "X"}], prompt="P ") == [{"text": "a", "prompt": "X"}]   # existing prompt wins
    assert m.parse_texts(["a"], prompt="") == [{"text": "a"}]
    m.append_prompt_sep = True
    assert m.parse_texts(["a"], prompt="P")[0]["prompt"] == "P" + tok.sep_token + " "
    with pytest.raises(NotImplementedError):
        m.parse_texts(("a",))
    with pytest.raises(AssertionError):
        m.parse_texts([])


def test_corpus_sort_and_id_columns():
    from lightretriever_amd.retriever import _sorted_corpus, _ids_and_list
    corpus = {"a": {"text": "xx"}, "b": {"text": "xxxx", "title": "t"}, "c": {"text": "xx"}, "d": "xxxxxxx"}
    ids, docs = _sorted_corpus(corpus)
    assert ids == O.sort_corpus_ids_longest_first(corpus) == ["d", "b", "a", "c"]      # stable for equal lengths
    assert docs[1] == corpus["b"]
    assert _ids_and_list({"q1": "x", "q2": "y"}) == (["q1", "q2"], ["x", "y"])
    with pytest.raises(NotImplementedError):
        _sorted_corpus([1, 2])
    with pytest.raises(NotImplementedError):
        _ids_and_list(["x"])
    import datasets
    ds = datasets.Dataset.from_list([{"foo": "1", "text": "abc"}])
    with pytest.raises(KeyError):
        _sorted_corpus(ds)
    with pytest.raises(KeyError):
        _ids_and_list(ds)
    ds2 = datasets.Dataset.from_list([{"_id": "1", "text": "a"}, {"_id": "2", "text": "abc"}])
    assert _sorted_corpus(ds2)[0] == ["2", "1"]


def test_shard_assignment_is_a_partition():
    from lightretriever_amd.sharded import batches_for_rank, local_to_global_rows
    n, bs = 1003, 64
    for world in (1, 2, 3, 8):
        rows = [local_to_global_rows(n, bs, r, world) for r in range(world)]
        allrows = torch.cat(rows).sort().values
        assert torch.equal(allrows, torch.arange(n))
        sizes = [len(r) for r in rows]
        assert max(sizes) - min(sizes) <= bs
        assert batches_for_rank(n, bs, 0, world)[0] == (0, 64)


def test_pair_packing_roundtrip():
    from lightretriever_amd.sharded import pack_pairs, unpack_pairs
    D = torch.tensor([[0.5, -1.25, -3.4028235e38, 1e-20], [1.0, 0.0, -0.0, 3.0]], dtype=torch.float32)
    I = torch.tensor([[0, 123456789, -1, 2 ** 31 - 1], [5, 6, 7, 9_999_999]], dtype=torch.int64)
    d, i = unpack_pairs(pack_pairs(D, I))
    assert torch.equal(d.view(torch.int32), D.view(torch.int32)) and torch.equal(i, I)


def _gloo_worker(rank, world, port, q, X, k, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lightretriever_amd.sharded import exchange_topk, local_to_global_rows
    rows = local_to_global_rows(X.shape[0], 16, rank, world).numpy()      # interleaved batches of 16 rows
    D, I = O.flat_ip_topk(q, X[rows], k)                                    # oracle stands in for the HIP shard search on CPU
    I = np.where(I >= 0, rows[np.clip(I, 0, None)], -1)                      # local -> global rows (row_map)
    Dp, Ip = exchange_topk(torch.from_numpy(D), torch.from_numpy(I))
    Dm, Im = O.merge_topk(list(Dp.numpy()), list(Ip.numpy()), k)
    ret[rank] = (Dm, Im)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_search_over_gloo_world2():
    """N>1 path on CPU: two processes, interleaved row shards, all-gather of packed pairs, merge == whole-index search."""
    import torch.multiprocessing as mp
    rng = np.random.default_rng(3)
    X = O.l2_normalize(rng.standard_normal((150, 32)).astype(np.float32))
    X[7] = X[140]                      # a cross-shard tie
    q = O.l2_normalize(rng.standard_normal((6, 32)).astype(np.float32))
    k = 20
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 29500 + os.getpid() % 2000
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q, X, k, ret)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    Dw, Iw = O.flat_ip_topk(q, X, k)
    for r in range(2):
        np.testing.assert_array_equal(ret[r][1], Iw)
        np.testing.assert_array_equal(ret[r][0], Dw)


def _bench_rank_worker(rank, world, port, index_rows, q, X, k, ret):
    """One rank of `bench.py --gpus world` as far as its bookkeeping goes: contiguous shard by bench.shard_split, local top-k (the oracle
    stands in for the HIP shard search), ids = id_base + local row, pack -> all-gather -> merge; plus the MAX-over-ranks reduction of the
    timing and the all-gather of the shard sizes bench.py prints as `shard_rows_per_rank`."""
    import sys
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from lightretriever_amd.sharded import exchange_topk
    rows, base = bench.shard_split(index_rows, rank, world)
    D, I = O.flat_ip_topk(q, X[base:base + rows], k)
    I = np.where(I >= 0, I + base, -1)
    Dp, Ip = exchange_topk(torch.from_numpy(D), torch.from_numpy(I))
    Dm, Im = O.merge_topk(list(Dp.numpy()), list(Ip.numpy()), k)
    sizes = torch.empty(world, dtype=torch.int64)
    dist.all_gather_into_tensor(sizes, torch.tensor([rows], dtype=torch.int64))
    t = torch.tensor([1.0 + rank], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    # the `sharded` leg's bookkeeping (BASELINE configs[3] / configs[4]: 10M rows over the communicator): gathered shard sizes + the
    # MIN-reduced "fits" flag every rank branches on
    sizes10m = torch.empty(world, dtype=torch.int64)
    dist.all_gather_into_tensor(sizes10m, torch.tensor([bench.shard_split(10_000_000, rank, world)[0]], dtype=torch.int64))
    fits = torch.tensor([0 if rank == 2 else 1], dtype=torch.int64)
    dist.all_reduce(fits, op=dist.ReduceOp.MIN)
    assert sizes10m.tolist() == [2_500_000] * 4 and int(fits.item()) == 0 and bench.reduce_max(float(rank), torch.device("cpu"), True) == 3.0
    # (the helpers bench.py itself uses: over gloo the tiny collectives live on the host -- coll_device -- whatever device the rank computes on)
    assert bench.coll_device(torch.device("cuda", 0)) == torch.device("cpu") and bench.gather_counts(100 + rank, torch.device("cuda", 0), True) == [100, 101, 102, 103]
    ret[rank] = (Dm, Im, sizes.tolist(), base, float(t.item()))
    dist.barrier()
    dist.destroy_process_group()


def test_bench_shard_split_covers_every_row_for_any_world_size():
    """`index_rows // world` rows per rank silently dropped the remainder for a world size that does not divide the
    index; bench.shard_split hands the remainder out one row each."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    for n in (1_000_000, 10_000_000, 1_000_003, 17, 5):
        for world in (1, 2, 3, 4, 6, 7, 8):
            parts = [bench.shard_split(n, r, world) for r in range(world)]
            assert parts[0][1] == 0 and sum(p[0] for p in parts) == n
            for (ra, ba), (rb, bb) in zip(parts, parts[1:]):
                assert bb == ba + ra and 0 <= ra - rb <= 1            # contiguous, disjoint, sizes within one row of each other
    assert [bench.shard_split(1_000_000, r, 8) for r in range(8)] == [(125_000, 125_000 * r) for r in range(8)]
    # BASELINE configs[3] / configs[4]: 10M rows over 8 ranks (bench.py's `sharded` leg), and over world sizes that do not divide them
    assert [bench.shard_split(10_000_000, r, 8) for r in range(8)] == [(1_250_000, 1_250_000 * r) for r in range(8)]
    assert [bench.shard_split(10_000_000, r, 3)[0] for r in range(3)] == [3_333_334, 3_333_333, 3_333_333]
    assert bench.shard_split(10_000_000, 6, 7) == (1_428_571, 10_000_000 - 1_428_571)


def test_bench_rank_bookkeeping_over_gloo_world4():
    """The N > 1 path of bench.py on CPU with FOUR ranks and an index size 4 does not divide: every rank ends with the whole-index top-k,
    the gathered shard sizes add up to the index, the timing reduction is the maximum over the ranks."""
    import torch.multiprocessing as mp
    rng = np.random.default_rng(5)
    n, world, k = 203, 4, 15
    X = O.l2_normalize(rng.standard_normal((n, 32)).astype(np.float32))
    X[50] = X[151]                     # a cross-shard tie
    q = O.l2_normalize(rng.standard_normal((5, 32)).astype(np.float32))
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 31500 + os.getpid() % 2000
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_bench_rank_worker, args=(r, world, port, n, q, X, k, ret)) for r in range(world)]
    [p.start() for p in procs]
    [p.join(180) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    Dw, Iw = O.flat_ip_topk(q, X, k)
    for r in range(world):
        Dm, Im, sizes, base, tmax = ret[r]
        np.testing.assert_array_equal(Im, Iw)
        np.testing.assert_array_equal(Dm, Dw)
        assert sizes == [51, 51, 51, 50] and base == sum(sizes[:r]) and tmax == 4.0


class _StubEncoder:
    """Deterministic stand-in for LrxEncoder.encode_prefixed on CPU: row = f(prefix, suffix ids); tests the slicing only."""
    class cfg:
        hidden_size = 8
    device = torch.device("cpu")

    def encode_prefixed(self, prefix_ids, suffix_ids, out=None, normalize=False):
        base = float(prefix_ids.sum())
        rows = suffix_ids[:, :1].float() * torch.arange(1, 9).float()[None, :] + base + suffix_ids[:, 1:2].float()
        out[:rows.shape[0]] = rows
        return out[:rows.shape[0]]


class _StubTok:
    bos_token_id, eos_token_id = 1, 2

    def __len__(self):
        return 203                                         # not divisible by the world size

    def encode(self, text, add_special_tokens=True):
        return ([1] if add_special_tokens else []) + [10 + len(w) for w in text.split()]


def _embbag_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lightretriever_amd.modeling import LrxHybridModel
    hm = LrxHybridModel(_StubEncoder(), normalize=True)
    table = hm.construct_embedding_bag_distributed(_StubTok(), prompt="query: find it", batch_size=16)
    ret[rank] = table.numpy()
    dist.barrier()
    dist.destroy_process_group()


def test_embedding_bag_vocab_slices_over_gloo_world2():
    """N1 multi-rank build: each rank builds one vocabulary slice, the all-gather gives every rank the whole table."""
    import torch.multiprocessing as mp
    from lightretriever_amd.modeling import LrxHybridModel
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 31500 + os.getpid() % 2000
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_embbag_worker, args=(r, 2, port, ret)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    want = LrxHybridModel(_StubEncoder()).construct_embedding_bag(_StubTok(), prompt="query: find it", batch_size=16).numpy()
    assert want.shape == (203, 8)
    for r in range(2):
        np.testing.assert_array_equal(ret[r], want)


def test_sparse_token_mask_matches_reference_rule(tok):
    """N2 host rule: get_sparse_attention_mask restated on the packed layout == the reference's padded masks (golden)."""
    from lightretriever_amd.modeling import sparse_token_mask, EncodeCollator
    g = np.load(os.path.join(GOLDEN, "sparse.npz"))
    sep = int(g["sep_token_id"])
    am = g["attention_mask"].astype(bool)
    ids, _, _, cu, _ = O.pack_padded(g["input_ids"], g["attention_mask"])
    np.testing.assert_array_equal(sparse_token_mask(ids, cu, sep, False).astype(bool), g["mask_plain"][am])
    np.testing.assert_array_equal(sparse_token_mask(ids, cu, sep, True).astype(bool), g["mask_noprompt"][am])
    np.testing.assert_array_equal(sparse_token_mask(ids, cu, None, True).astype(bool), g["mask_plain"][am])
    qm = g["attention_mask"][[0, 6]]
    ids2, _, _, cu2, _ = O.pack_padded(g["quirk_ids"], qm)
    np.testing.assert_array_equal(sparse_token_mask(ids2, cu2, sep, True).astype(bool), g["quirk_mask"][qm.astype(bool)])
    # the collator ships it next to the packed ids
    out = EncodeCollator(tok, encode_is_query=False, p_max_len=32, sparse_mask=True)([{"text": "dense retrieval with large models"}, {"text": "a"}])
    m, cu3 = out["sparse_mask"].numpy(), out["cu_seqlens"].numpy()
    assert m.dtype == np.uint8 and m.shape[0] == cu3[-1]
    assert m[cu3[:-1]].sum() == 0 and m[cu3[1:] - 1].sum() == 0 and m.sum() == cu3[-1] - 2 * (len(cu3) - 1)


def test_flat_index_file_layout_and_round_trip(tmp_path):
    """N4: the {prefix}.flat.faiss file is Faiss's IndexFlatIP serialisation (index_write.cpp): header bytes spelled out here."""
    import struct
    from lightretriever_amd import index_io as io
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1000, 64)).astype(np.float32)
    f = str(tmp_path / "my-index.flat.faiss")
    io.write_flat_ip(f, [x[:300], x[300:301], x[301:]], 64, 1000)
    raw = open(f, "rb").read()
    want = b"IxFI" + struct.pack("<i", 64) + struct.pack("<q", 1000) + struct.pack("<qq", 1 << 20, 1 << 20) + b"\x01" + struct.pack("<i", 0) \
        + struct.pack("<Q", 64000)
    assert raw[:len(want)] == want and len(want) == io.HEADER_BYTES == 45
    assert raw[len(want):] == x.tobytes()
    mm = io.read_flat_ip(f)
    assert mm.shape == (1000, 64) and not mm.flags.writeable
    np.testing.assert_array_equal(np.asarray(mm), x)
    io.write_flat_ip(str(tmp_path / "empty.faiss"), [], 32, 0)                       # empty shard (a rank without rows)
    assert io.read_flat_ip(str(tmp_path / "empty.faiss")).shape == (0, 32)
    with pytest.raises(ValueError):
        io.write_flat_ip(str(tmp_path / "bad.faiss"), [x[:10]], 64, 11)             # row count mismatch
    assert not os.path.exists(str(tmp_path / "bad.faiss"))                          # nothing half-written under the final name
    for corrupt in (b"IxF2" + raw[4:], raw[:-4], raw[:8] + struct.pack("<q", 999) + raw[16:]):
        open(str(tmp_path / "c.faiss"), "wb").write(corrupt)
        with pytest.raises(ValueError):
            io.read_flat_ip(str(tmp_path / "c.faiss"))
    # id map: same TSV as save_dict_to_tsv / load_tsv_to_dict (header row, QUOTE_MINIMAL)
    mapping = {"doc-1": 0, "with\ttab": 1, 'quo"te': 2, "ünï": 3}
    t = str(tmp_path / "my-index.flat.tsv")
    io.save_dict_to_tsv(mapping, t, keys=io.MAPPING_TSV_KEYS)
    assert open(t, encoding="utf-8").readline().rstrip("\r\n") == "beir-docid\tfaiss-docid"
    assert io.load_tsv_to_dict(t) == mapping
    assert io.shard_prefix("my-index") == "my-index" and io.shard_prefix("my-index", 3, 8) == "my-index.rank3-of-8"


def test_id_map_tsv_is_byte_equal_to_the_reference_written_file(tmp_path):
    """Row f-N4 pinned to the reference: tests/golden/persist_ref.json holds the bytes the reference's own save_dict_to_tsv wrote
    (retriever/faiss_search.py:28-33) for ids with tabs, quotes, commas, blanks, non-ASCII, an embedded line feed and the empty string,
    what its load_tsv_to_dict (:35-43) read back, and what DenseRetrievalFaissSearch.save / ._load (:99-123) name and return
    (tests/golden/gen_search_goldens.py:persist_goldens).  index_io must write the same bytes and read the reference's file the same way."""
    import base64
    import json
    from lightretriever_amd import index_io as io
    from lightretriever_amd.retriever import FlatIPFaissSearch
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "persist_ref.json")))
    ids = fx["ids"]
    mapping = {pid: i for i, pid in enumerate(ids)}
    for key, keys, header in (("tsv_with_header_b64", io.MAPPING_TSV_KEYS, True), ("tsv_no_header_b64", None, False)):
        want = base64.b64decode(fx[key])
        f = str(tmp_path / (key + ".tsv"))
        io.save_dict_to_tsv(mapping, f, keys=keys)
        assert open(f, "rb").read() == want, key                           # byte for byte what the reference writes
        ref_file = str(tmp_path / (key + ".ref.tsv"))
        open(ref_file, "wb").write(want)
        got = io.load_tsv_to_dict(ref_file, header=header)                  # the reference's file through this build's reader
        want_loaded = fx["loaded_with_header" if header else "loaded_no_header"]
        assert [[k, v] for k, v in got.items()] == want_loaded              # same keys, same order, same ints as the reference's reader
    # the reference's reader does not restore an embedded "\n" differently from this one, and every id survives the round trip
    assert [k for k, _ in fx["loaded_with_header"]] == ids

    class RecordingIndex:
        saved = []

        def save(self, fname):
            self.saved.append(os.path.basename(fname))
            open(fname, "wb").write(b"x")

    fs = FlatIPFaissSearch.__new__(FlatIPFaissSearch)
    fs.mapping, fs.faiss_index = {pid: i for i, pid in enumerate(ids[:6])}, RecordingIndex()
    out_dir = tmp_path / "saved"
    FlatIPFaissSearch.__mro__[1].save(fs, str(out_dir), "my-index", "flat")  # DenseRetrievalFaissSearch.save (faiss_search.py:111-123)
    assert sorted(os.listdir(out_dir)) == [n for n in fx["save_files"] if n != "m.tsv"]
    assert fs.faiss_index.saved == fx["save_index_file"]
    assert open(out_dir / "my-index.flat.tsv", "rb").read() == base64.b64decode(fx["save_tsv_b64"])
    fs2 = FlatIPFaissSearch.__new__(FlatIPFaissSearch)
    path, passage_ids = FlatIPFaissSearch.__mro__[1]._load(fs2, str(out_dir), "my-index", "flat")
    assert os.path.basename(path) == fx["load_faiss_path_basename"] and passage_ids == fx["load_passage_ids"]
    assert [[k, v] for k, v in fs2.mapping.items()] == fx["load_mapping"] and [[k, v] for k, v in fs2.rev_mapping.items()] == fx["load_rev_mapping"]


def test_flat_index_header_hand_derived_from_the_faiss_source():
    """The `.faiss` bytes for d = 64, ntotal = 3, written out by hand from Faiss's published serialiser -- NO Faiss build has verified
    this (faiss is neither in the reference tree nor in the image).  faiss/impl/index_write.cpp (v1.7.3 .. 1.8): write_index(), IndexFlat
    branch: `uint32_t h = fourcc("IxFI")` for METRIC_INNER_PRODUCT, WRITE1(h); write_index_header(): WRITE1(idx->d) [int, 4 B],
    WRITE1(idx->ntotal) [idx_t = int64], `idx_t dummy = 1 << 20; WRITE1(dummy); WRITE1(dummy);`, WRITE1(idx->is_trained) [bool, 1 B],
    WRITE1(idx->metric_type) [enum MetricType, 4 B; METRIC_INNER_PRODUCT = 0; metric_arg only when metric_type > 1]; then
    WRITEXBVECTOR(idxf->codes) (faiss/impl/io_macros.h): `size_t size = vec.size() / 4` [8 B, the float count] followed by the bytes.
    fourcc() (faiss/impl/io.cpp) packs the four characters little-endian, i.e. the file starts with the text "IxFI"."""
    from lightretriever_amd import index_io as io
    import tempfile
    x = np.arange(3 * 64, dtype=np.float32).reshape(3, 64) / 8
    want = bytes.fromhex(
        "49784649"            # 'I' 'x' 'F' 'I'
        "40000000"            # d = 64
        "0300000000000000"    # ntotal = 3
        "0000100000000000"    # dummy = 1 << 20
        "0000100000000000"    # dummy = 1 << 20
        "01"                  # is_trained
        "00000000"            # metric_type = METRIC_INNER_PRODUCT
        "c000000000000000"    # 192 floats follow
    )
    assert len(want) == 45
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "h.flat.faiss")
        io.write_flat_ip(f, [x], 64, 3)
        raw = open(f, "rb").read()
    assert raw[:45] == want
    assert raw[45:45 + 16] == bytes.fromhex("00000000" "0000003e" "0000803e" "0000c03e")      # 0, 1/8, 2/8, 3/8 as little-endian fp32
    assert len(raw) == 45 + 3 * 64 * 4


def test_prefetch_batches_keeps_order_propagates_errors_and_stops_clean():
    """The collate-ahead worker of encode_corpus: batches arrive in input order, a collator failure surfaces in the consumer,
    an abandoned iteration leaves no thread behind."""
    import threading
    import time
    from lightretriever_amd.modeling import _prefetch_batches

    def coll(x):
        time.sleep(0.002)
        return list(x)
    items = list(range(103))
    out = list(_prefetch_batches(coll, items, 10))
    assert [x for _, _, b in out for x in b] == items and out[-1][:2] == (100, 103) and len(out) == 11
    assert list(_prefetch_batches(coll, items[:7], 10)) == [(0, 7, items[:7])]          # single batch: no thread
    g = _prefetch_batches(coll, items, 10)
    next(g)
    g.close()

    def bad(x):
        if x[0] >= 30:
            raise ValueError("boom")
        return x
    with pytest.raises(ValueError, match="boom"):
        list(_prefetch_batches(bad, items, 10))
    time.sleep(0.05)
    assert not [t for t in threading.enumerate() if t.name == "lrx-collate"]


def test_token_budget_batches_merges_consecutive_packed_batches():
    """encode_corpus's batch merging on the host side: spans stay consecutive and complete, budgets are respected, cu_seqlens are
    re-based, padded batches and budget 0 pass through untouched."""
    import numpy as np
    import torch
    from lightretriever_amd.modeling import _token_budget_batches

    def mk(lens, tag, mask=False):
        b = {"input_ids": torch.arange(sum(lens), dtype=torch.int32) + 1000 * tag,
             "cu_seqlens": torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32), "max_seqlen": max(lens)}
        if mask:
            b["sparse_mask"] = torch.ones(sum(lens), dtype=torch.uint8) * tag
        return b
    gen = [(0, 3, mk([5, 4, 3], 0, True)), (3, 6, mk([3, 2, 2], 1, True)), (6, 9, mk([2, 1, 1], 2, True)), (9, 10, mk([1], 3, True))]
    out = list(_token_budget_batches(iter(gen), 20, 100))
    assert [(s, e) for s, e, _ in out] == [(0, 6), (6, 10)]
    b = out[0][2]
    assert b["cu_seqlens"].tolist() == [0, 5, 9, 12, 15, 17, 19] and b["max_seqlen"] == 5 and b["cu_seqlens"].dtype == torch.int32
    assert b["input_ids"].tolist() == list(range(12)) + list(range(1000, 1007)) and b["sparse_mask"].tolist() == [0] * 12 + [1] * 7
    assert [(s, e) for s, e, _ in _token_budget_batches(iter(gen), 0, 100)] == [(0, 3), (3, 6), (6, 9), (9, 10)]      # off
    assert [(s, e) for s, e, _ in _token_budget_batches(iter(gen), 1000, 6)] == [(0, 6), (6, 10)]                    # document cap
    assert [(s, e) for s, e, _ in _token_budget_batches(iter(gen), 1000, 1000)] == [(0, 10)]
    assert [(s, e) for s, e, _ in _token_budget_batches(iter(gen), 3, 1000)] == [(0, 3), (3, 6), (6, 9), (9, 10)]    # nothing fits together
    padded = [(0, 2, {"input_ids": torch.zeros(2, 4), "attention_mask": torch.ones(2, 4)}), (2, 4, mk([1, 1], 5)), (4, 6, mk([1, 1], 6))]
    out = list(_token_budget_batches(iter(padded), 100, 100))
    assert [(s, e) for s, e, _ in out] == [(0, 2), (2, 6)] and "attention_mask" in out[0][2]


def test_inference_arguments_accept_the_reference_cli_and_refuse_unimplemented_modes():
    """lightretriever.inference.arguments.InferenceArguments through HfArgumentParser (how eval/eval_arguments.py builds it): every
    model flag of the reference's launch scripts parses; options that select parts of the reference this path does not implement
    raise instead of being ignored."""
    import pytest
    from transformers import HfArgumentParser
    from lightretriever.inference.arguments import InferenceArguments
    parse = lambda *a: HfArgumentParser(InferenceArguments).parse_args_into_dataclasses(["--model_name_or_path", "meta-llama/Llama-3.2-1B",
                                                                                         "--model_type", "HybridModel", *a])[0]
    a = parse("--hybrid_use_emb_vector", "--noncontextual_query_embedding", "--lowercase", "--add_sep_token", "--add_bos_num", "1", "--add_eos_num", "1",
              "--pooling_strategy", "lasttoken", "--score_function", "cos_sim", "--attn_implementation", "flash_attention_2", "--cumulative_seq",
              "--liger_kernel", "--bf16", "--batch_size", "256", "--p_max_len", "512", "--q_max_len", "512", "--inference_arch", "PytorchRPCExactSearchModel",
              "--pad_to_multiple_of", "8", "--anserini_impact_search", "True")
    assert a.normalize is True and a.encode_sparse is False and a.lowercase and a.add_sep_token
    assert (a.pad_token, a.sep_token) == ("<|reserved_special_token_0|>", "<|reserved_special_token_1|>")      # llama defaults (arguments.py:286-310)
    b = parse("--hybrid_use_token_id_vector", "--sparse_use_relu", "--sparse_use_log_saturation", "--score_function", "dot")
    assert b.encode_sparse and b.normalize is False and b.sparse_use_relu and b.token_id_vector_type == "sum"
    # the reference's own eval recipe (eval/README.md:13-52): symmetric dense vector; and the LM-embedding-layer ablation
    c = parse("--hybrid_use_dense_vector", "--bf16", "--q_max_len", "512", "--p_max_len", "512", "--pooling_strategy", "lasttoken", "--sparse_use_max_aggregation",
              "True", "--sparse_use_relu", "--sparse_use_log_saturation", "--cumulative_seq", "--liger_kernel")
    assert c.hybrid_use_dense_vector and not c.hybrid_use_emb_vector and not c.encode_sparse and c.dtype == torch.bfloat16
    d = parse("--hybrid_use_emb_vector")
    assert d.hybrid_use_emb_vector and d.noncontextual_query_embedding is False
    for bad in (["--hybrid_use_emb_vector", "--untie_encoder"], ["--hybrid_use_emb_vector", "--enable_bidirectional_attention"],
                ["--hybrid_use_emb_vector", "--use_sparse_linear_projector"], ["--hybrid_use_emb_vector", "--sparse_remove_stopwords"],
                ["--hybrid_use_emb_vector", "--hybrid_model_architecture", "bert"],
                ["--hybrid_use_emb_vector", "--pooling_strategy", "none"], ["--hybrid_use_emb_vector", "--sparse_use_max_aggregation", "False"]):
        with pytest.raises(NotImplementedError):
            parse(*bad)
    with pytest.raises(ValueError, match="no vector type selected"):
        parse()
    # round 6: `--hybrid_use_sparse_vector` alone (LM-head sparse queries, the `spr` mode) is served; token-id queries only with their own flag
    sp = parse("--hybrid_use_sparse_vector", "--sparse_top_k_qry", "32")
    assert sp.hybrid_use_sparse_vector and sp.encode_sparse and not sp.hybrid_use_token_id_vector and sp.sparse_top_k_qry == 32
    # round 6: `--fp16` is accepted like `--bf16` (recorded in dtype; one arithmetic); both at once is the reference's own contradiction
    assert parse("--hybrid_use_emb_vector", "--fp16").dtype == torch.float16
    with pytest.raises(ValueError):
        parse("--hybrid_use_emb_vector", "--fp16", "--bf16")
    # round 6: sparse vectors restricted to the sequence's own tokens (modeling_hybrid.py:175-180) are served, each side by its own flag
    po = parse("--hybrid_use_sparse_vector", "--sparse_pool_from_original_input_ids_qry")
    assert po.sparse_pool_from_original_input_ids_qry and not po.sparse_pool_from_original_input_ids_psg
    # round 6: every vector-returning pooling strategy of finetune/dense_pooling.py:12-82 is served
    for st in ("cls", "mean", "second_to_last", "third_to_last", "avg_first_last", "avg_top2"):
        assert parse("--hybrid_use_dense_vector", "--pooling_strategy", st).pooling_strategy == st
    # the defaults are the reference's (finetune/arguments.py:175-195, inference/arguments.py:27,68): nothing selected, fp32 container, EncoderModel
    e = InferenceArguments(model_name_or_path="/x/llama")
    assert (e.model_type, e.bf16, e.hybrid_use_dense_vector, e.hybrid_use_emb_vector, e.noncontextual_query_embedding, e.hybrid_use_token_id_vector,
            e.pooling_strategy, e.dtype) == ("EncoderModel", False, False, False, False, False, None, None)
    with pytest.raises(NotImplementedError):
        InferenceArguments(model_name_or_path="/x/llama", model_type="RerankerModel")


def test_rpc_shard_mode_is_inactive_without_an_rpc_agent():
    """retriever._chunked_dense_search only takes the RPC-driven path when torch RPC is initialised and workers registered a model."""
    from lightretriever_amd import rpc_shards
    assert rpc_shards.rpc_workers() == []
    with pytest.raises(RuntimeError, match="no model registered"):
        saved = rpc_shards._WORKER.pop("model", None)
        try:
            rpc_shards._w_index([], [], 8, 4, 0, True, True)
        finally:
            if saved is not None:
                rpc_shards._WORKER["model"] = saved


def test_reference_eval_arguments_build_on_the_import_path_shim():
    """The reference's eval/eval_arguments.py declares EvalArguments as a dataclass subclass of lightretriever.inference.arguments
    .InferenceArguments and parses the flags of eval/call_evaluate_mteb.sh and the model flags of the launch scripts.
    tests/golden/eval_arguments.json (gen_eval_arguments_golden.py) holds what it parsed on the reference's own package.  Through this repo's
    import-path shim: the shim takes every base flag of that command line and leaves exactly the flags of the fields EvalArguments adds, each
    flag lands with the reference's value (normalize too, derived in __post_init__), and a dataclass subclass adding those fields parses the
    whole command line and runs the shim's __post_init__."""
    import dataclasses
    from typing import Optional
    from transformers import HfArgumentParser
    from lightretriever.inference.arguments import InferenceArguments
    import lightretriever_amd.inference as mine
    assert InferenceArguments is mine.InferenceArguments
    fx = json.load(open(os.path.join(GOLDEN, "eval_arguments.json")))
    argv, want = fx["argv"], fx["parsed"]
    eval_flags = {"--" + n for n in fx["eval_fields"]}
    a, rest = HfArgumentParser(InferenceArguments).parse_args_into_dataclasses(argv, return_remaining_strings=True)
    assert rest == [t for i, t in enumerate(argv) if t in eval_flags or (i and argv[i - 1] in eval_flags)]
    base_named = [t[2:] for t in argv if t.startswith("--") and t not in eval_flags]
    for name in base_named + ["normalize"]:
        assert getattr(a, name) == want[name], name
    assert a.normalize is True and a.encode_sparse is False
    assert a.model_type == "HybridModel" and a.inference_arch == "PytorchRPCExactSearchModel"
    extra = [n for n in fx["eval_fields"] if "--" + n in argv]
    EvalLike = dataclasses.make_dataclass("EvalLike", [(n, Optional[str], dataclasses.field(default=None)) for n in extra], bases=(InferenceArguments,))
    (e,) = HfArgumentParser(EvalLike).parse_args_into_dataclasses(argv)
    assert all(getattr(e, n) == str(want[n]) for n in extra)
    assert all(getattr(e, f.name) == getattr(a, f.name) for f in dataclasses.fields(InferenceArguments))


def test_bench_gpus_flag_is_checked_before_any_gpu_work():
    """`bench.py --gpus N` must never silently benchmark a different number of GPUs."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE=2 but --gpus 1" in r.stderr
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "64"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--gpus 64 but only" in r.stderr


def test_bench_legs_beyond_the_headline_need_full_before_any_gpu_work():
    """A plain bench.py run times the headline legs (encode, search) only; naming another leg without --full, or a leg that does not
    exist, is refused while the arguments are parsed."""
    import subprocess
    import sys
    bench = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
    for legs in ("sparse", "encode,configs", "cpu", "sharded"):
        r = subprocess.run([sys.executable, bench, "--gpus", "1", "--legs", legs], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--full is needed for --legs" in r.stderr, (legs, r.stderr[-500:])
    r = subprocess.run([sys.executable, bench, "--gpus", "1", "--full", "--legs", "encode,bogus"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "unknown --legs ['bogus']" in r.stderr


def test_bench_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    """bench.py --dump-outputs: float arrays as float32, integer ids as exact float64; an array over its share of the 64 MB budget becomes the
    same seeded sample of its rows on every run, with the row indices next to it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("lrx_bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    arrays = {"embeddings": torch.randn(256, 64, generator=g), "search_ids": torch.randint(0, 10_000_000, (100, 100), generator=g),
              "sparse_vectors": torch.randn(256, 70_000, generator=g)}
    for run in ("a", "b"):
        shapes = bench.dump_outputs(str(tmp_path / run), arrays)
        assert shapes["embeddings"] == [256, 64] and shapes["search_ids"] == [100, 100] and 0 < shapes["sparse_vectors"][0] < 256
        assert sum(os.path.getsize(p) for p in (tmp_path / run).iterdir()) <= 64_000_000
    emb = np.load(str(tmp_path / "a" / "embeddings.npy"))
    ids = np.load(str(tmp_path / "a" / "search_ids.npy"))
    assert emb.dtype == np.float32 and np.array_equal(emb, arrays["embeddings"].numpy())
    assert ids.dtype == np.float64 and np.array_equal(ids.astype(np.int64), arrays["search_ids"].numpy())
    rows = np.load(str(tmp_path / "a" / "sparse_vectors_rows.npy")).astype(np.int64)
    assert np.array_equal(np.load(str(tmp_path / "a" / "sparse_vectors.npy")), arrays["sparse_vectors"].numpy()[rows])
    for f in os.listdir(str(tmp_path / "a")):
        assert np.array_equal(np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))), f


def test_trained_like_synthetic_checkpoint_hits_its_regime_on_cpu():
    """lightretriever_amd/synth.py (the weight statistics tests/test_gpu_trained_like.py runs at full depth on the GPU) on a tiny config on
    the CPU: deterministic per seed, HF-complete state dict, and the calibrated regime -- logit spread 5-10 with a small bilinear part, a
    first-token sink, massive channels, Qwen-scale biases."""
    from lightretriever_amd import EncoderConfig
    from lightretriever_amd.synth import trained_like_state_dict
    for bias in (False, True):
        cfg = EncoderConfig(vocab_size=3000, hidden_size=256, num_layers=3, num_q_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=512,
                            qkv_bias=bias, rope_type="default", rope_theta=1e6 if bias else 5e5, max_positions=128)
        sd, st = trained_like_state_dict(cfg, seed=4, device=torch.device("cpu"))
        sd2, st2 = trained_like_state_dict(cfg, seed=4, device=torch.device("cpu"))
        assert st["summary"] == st2["summary"] and all(torch.equal(sd[k], sd2[k]) for k in sd)
        want = {"embed_tokens.weight", "norm.weight"} | {f"layers.{i}.{n}" for i in range(3) for n in (
            "self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight", "mlp.gate_proj.weight",
            "mlp.up_proj.weight", "mlp.down_proj.weight", "input_layernorm.weight", "post_attention_layernorm.weight")}
        if bias:
            want |= {f"layers.{i}.self_attn.{p}_proj.bias" for i in range(3) for p in "qkv"}
        assert set(sd) == want and all(v.dtype == torch.bfloat16 for v in sd.values())
        s = st["summary"]
        # (a 256-wide toy: the constant q / k components alone can exceed the target spread in a layer; the real widths stay within 5-11,
        # asserted on the GPU)
        assert 4.5 <= s["logit_sigma_min"] and s["logit_sigma_max"] <= 30 and s["top1_prob_mean"] > 0.5
        assert s["sink_mass_mean"] > 0.03 and s["stream_max_over_median_max"] > 200
        assert all(0.5 <= l["content_sigma"] <= 2.1 for l in st["layers"])
        if bias:
            assert s["max_abs_bias"] >= 100


def test_trace_checker_counts_foreign_kernels_between_the_markers(tmp_path):
    """tools/check_trace_clean.py: every non-liblrx kernel between k_trace_marker<0> and <1> is counted, wherever it sits."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def trace(names):
        f = tmp_path / "t_kernel_trace.csv"
        with open(f, "w") as fh:
            fh.write("Kernel_Name,Start_Timestamp,End_Timestamp\n")
            for i, n in enumerate(names):
                fh.write('"%s",%d,%d\n' % (n, 10 * i, 10 * i + 5))
        return subprocess.run([sys.executable, os.path.join(root, "tools", "check_trace_clean.py"), str(f), "3"], capture_output=True, text=True)

    chain = ["k_embedding_bag(float const*)", "k_pack_queries_xb(float const*)", "void k_filter_xreg<7, 4, false, 1>(x)", "k_sample_threshold(float const*)",
             "void k_filter_xreg_emit<7, 4, 2>(x)", "k_refine_band(x)", "k_refine_merge(x)", "k_topk_select_rescore(x)"]
    clean = ["at::native::fill(x)", "void k_trace_marker<0>()", "k_embedding_gather(x)", "void k_gemm_bf16_nt<2>(x)"] + chain * 3 + ["void k_trace_marker<1>()", "at::native::randn(x)"]
    r = trace(clean)
    assert r.returncode == 0 and "foreign (at::native ...) among them: 0" in r.stdout, r.stdout
    dirty = clean[:10] + ["void at::native::vectorized_elementwise_kernel<4>(x)"] + clean[10:]
    r = trace(dirty)
    assert r.returncode == 1 and "among them: 1" in r.stdout, r.stdout
    late = clean[:-2] + ["at::native::late(x)"] + clean[-2:]        # after the last search but still inside the window
    assert trace(late).returncode == 1
    assert trace(clean[:4] + chain * 2 + clean[-2:]).returncode == 1      # too few searches
    assert trace([n for n in clean if "marker" not in n]).returncode == 2  # no markers


def test_encode_queries_routes_vector_types_without_a_gpu(tok):
    """Round 5: LrxExactSearchModel.encode_queries picks the collator outputs and the result keys from the model's flags (the reference's
    rule, finetune/modeling_hybrid.py:362-366 + inference/exact_search_torchrpc.py:139-170); checked with a stand-in B3 operator on the CPU."""
    from lightretriever_amd.modeling import LrxExactSearchModel

    class FakeHybrid:
        def __init__(self, dense, emb, nonctx, sparse=False):
            self.hybrid_use_dense_vector, self.hybrid_use_emb_vector, self.noncontextual_query_embedding = dense, emb, nonctx
            self.encode_sparse, self.emb_bag, self.emb_bag_prompt, self.seen = sparse, None, None, []

        def construct_embedding_bag(self, tokenizer, prompt=None, batch_size=0):
            self.emb_bag, self.emb_bag_prompt = torch.zeros(len(tokenizer), 4), prompt

        def encode_query(self, batch):
            self.seen.append(sorted(batch))
            out = {}
            if self.hybrid_use_dense_vector:
                out["dense_reps"] = (batch["cu_seqlens"][1:] - batch["cu_seqlens"][:-1]).float()[:, None]        # = the sequence lengths
            if self.hybrid_use_emb_vector:
                n = batch["nonctx_tok_emb_offsets"].numel() if self.noncontextual_query_embedding else batch["cu_seqlens"].numel() - 1
                out["emb_reps"] = torch.full((n, 1), 7.0)
            return out

    qs = ["capital of france", "a", "dense retrieval with large language models"]
    # symmetric dense: LM inputs only, the prompt is part of the tokens, no table is built
    hm = FakeHybrid(True, False, False)
    m = LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=16, p_max_len=32)
    m.query_prompt = "query: "
    r = m.encode_queries(qs, batch_size=2)
    assert set(r) == {"dense_reps"} and r["dense_reps"].shape == (3, 1) and hm.emb_bag is None
    assert hm.seen == [["cu_seqlens", "input_ids", "max_seqlen"]] * 2
    want = [min(16, len(tok("query: " + q, add_special_tokens=True)["input_ids"])) for q in qs]
    assert r["dense_reps"][:, 0].tolist() == [float(x) for x in want]
    assert LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=16, single_tensor_output=True).encode_queries(qs, batch_size=8).shape == (3, 1)
    # both vectors (the released checkpoints' flags): one batch dict carries LM inputs and bag inputs; the table is built with the prompt
    hm = FakeHybrid(True, True, True, sparse=True)
    m = LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=16)
    m.query_prompt = "query: "
    r = m.encode_queries(qs, batch_size=8)
    assert set(r) == {"dense_reps", "emb_reps", "token_id_reps"} and hm.emb_bag_prompt == "query: "
    assert hm.seen == [["cu_seqlens", "input_ids", "max_seqlen", "nonctx_tok_emb_input_ids", "nonctx_tok_emb_offsets"]]
    assert len(r["token_id_reps"]) == 3 and all(isinstance(d, dict) for d in r["token_id_reps"])
    # the input-embedding ablation: LM inputs, no table; asymmetric only: bag inputs only
    hm = FakeHybrid(False, True, False)
    assert set(LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=16).encode_queries(qs, batch_size=8)) == {"emb_reps"} and hm.emb_bag is None
    assert hm.seen == [["cu_seqlens", "input_ids", "max_seqlen"]]
    hm = FakeHybrid(False, True, True)
    assert set(LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=16).encode_queries(qs, batch_size=8)) == {"emb_reps"}
    assert hm.seen == [["nonctx_tok_emb_input_ids", "nonctx_tok_emb_offsets"]]
    # token-id-only model: nothing goes through the operator
    hm = FakeHybrid(False, False, False, sparse=True)
    assert set(LrxExactSearchModel(model=hm, tokenizer=tok, q_max_len=16).encode_queries(qs, batch_size=8)) == {"token_id_reps"} and hm.seen == []


def test_host_threads_per_rank_divides_the_usable_cores(monkeypatch):
    """Round 6: one process per GPU shares the node's host cores -- the tokenizer pool of a rank gets cores / ranks
    threads (at least one), never the default of every visible CPU."""
    from lightretriever_amd import inference
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(16)), raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    one = inference.host_threads_per_rank()
    assert 1 <= one <= 16
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "8")
    assert inference.host_threads_per_rank() == max(1, one // 8)
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "64")
    assert inference.host_threads_per_rank() == 1


def test_prefetched_token_budget_batches_preserve_input_order():
    """encode()'s host pipeline -- collation one worker thread ahead (_prefetch_batches) + token-budget merging (_token_budget_batches) -- hands
    the encoder every document exactly once, in input order, whatever the batch size and budget: row i of the output is input i
    (inference/exact_search_torchrpc.py:243-295 assembles by index for the same guarantee)."""
    from lightretriever_amd.modeling import _prefetch_batches, _token_budget_batches
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 60, size=1003).tolist()
    items = [{"i": i, "n": n} for i, n in enumerate(lens)]

    def coll(batch):                                            # packed collator stand-in: the document's index as its token ids
        ids = torch.cat([torch.full((b["n"],), b["i"], dtype=torch.int32) for b in batch])
        return {"input_ids": ids, "cu_seqlens": torch.tensor([0] + list(np.cumsum([b["n"] for b in batch])), dtype=torch.int32),
                "max_seqlen": max(b["n"] for b in batch)}

    for bs, budget, max_docs in ((16, 500, 64), (7, 0, 64), (64, 4000, 100), (1003, 10 ** 6, 10 ** 6), (5, 10 ** 6, 11)):
        seen = []
        for s, e, b in _token_budget_batches(_prefetch_batches(coll, items, bs), budget, max_docs):
            cu = b["cu_seqlens"].tolist()
            assert e - s == len(cu) - 1 and (budget <= 0 or cu[-1] <= max(budget, max(lens[s:e]) * bs)) and e - s <= max(max_docs, bs)
            for j in range(e - s):
                seg = b["input_ids"][cu[j]:cu[j + 1]]
                assert seg.numel() == lens[s + j] and bool((seg == s + j).all())
            seen.extend(range(s, e))
        assert seen == list(range(len(items)))
