"""GPU: the sharded search path over RCCL (backend "nccl") with a 1-rank process group on cuda:0 -- exercises
init_process_group, all_gather_into_tensor of the packed [Q,k] pairs and the on-device merge exactly as bench.py --gpus N
does (N>1 itself is covered on CPU by the gloo world-2 test; multi-GPU runs are the driver's)."""
import os

import numpy as np
import pytest
import torch

from oracle import lrx_oracle as O

pytestmark = pytest.mark.gpu


def test_sharded_finish_over_rccl_single_rank():
    import torch.distributed as dist
    from lightretriever_amd import FlatIPIndex
    from lightretriever_amd.sharded import ShardedFlatIPIndex, exchange_topk, local_to_global_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29600 + os.getpid() % 1000), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        rng = np.random.default_rng(0)
        X = O.l2_normalize(rng.standard_normal((3000, 64)).astype(np.float32))
        q = O.l2_normalize(rng.standard_normal((9, 64)).astype(np.float32))
        rows = local_to_global_rows(3000, 64, 0, 1)
        idx = FlatIPIndex(64)
        idx.add(X)
        sh = ShardedFlatIPIndex(idx, row_map=rows.cuda())
        D, I = idx.search(torch.from_numpy(q).cuda(), 10)
        Dp, Ip = exchange_topk(D, I, force_collective=True)          # real RCCL all-gather even with one rank
        assert Dp.shape == (1, 9, 10) and torch.equal(Dp[0], D) and torch.equal(Ip[0], I)
        Dm, Im = sh.search(torch.from_numpy(q).cuda(), 10)
        Do, Io = O.flat_ip_topk(q, X, 10)
        np.testing.assert_array_equal(Im.cpu().numpy(), Io)
        t = torch.tensor([1.5], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)                       # the timing reduction bench.py uses
        dist.barrier()
        assert t.item() == 1.5
    finally:
        dist.destroy_process_group()


def _search_worker(rank, world, port, ret):
    """One rank of a two-process run on the same GPU (gloo process group; RCCL refuses two ranks on one device): the full
    B1 flow -- HybridSearch.search over a synthetic corpus -- with the chunk's batches sharded over the ranks."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from test_gpu_api import build_stack, synth_corpus
        from helpers import load_model_golden
        from lightretriever_amd.retriever import HybridSearch
        cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
        tok, enc, hm, model = build_stack(cfg_o, w)
        corpus = synth_corpus(np.random.default_rng(0), 150)
        queries = {"q0": "capital of france", "q1": "dense retrieval models", "q2": "amd instinct memory"}
        res = HybridSearch(model, batch_size=16, corpus_chunk_size=70).search(corpus, queries, top_k=12)
        ret[rank] = {q: dict(v) for q, v in res.items()}
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_search_flow_sharded_over_two_ranks_equals_single_process():
    """SURVEY 8e through the reference-shaped entry point: two processes, interleaved batches per chunk, all-gather + merge ->
    the same hits (ids and scores) as one process holding the whole corpus."""
    import torch.multiprocessing as mp
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd.retriever import HybridSearch
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, hm, model = build_stack(cfg_o, w)
    corpus = synth_corpus(np.random.default_rng(0), 150)
    queries = {"q0": "capital of france", "q1": "dense retrieval models", "q2": "amd instinct memory"}
    want = HybridSearch(model, batch_size=16, corpus_chunk_size=70).search(corpus, queries, top_k=12)
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 30500 + os.getpid() % 1000
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_search_worker, args=(r, 2, port, ret)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    for r in range(2):
        assert set(ret[r]) == set(want)
        for q in want:
            assert list(ret[r][q]) == list(want[q]) or set(ret[r][q]) == set(want[q])
            for pid, sc in want[q].items():
                assert abs(ret[r][q][pid] - sc) < 1e-6


def _rpc_worker(rank, world, port, ret):
    """One process of the reference's launch shape (eval/eval_utils.py:launch_eval): torch RPC, a model on every rank, only rank 0
    drives the search; the other rank serves calls inside rpc.shutdown().  Both processes share cuda:0 here."""
    from torch.distributed import rpc
    import sys
    os.environ.setdefault("TP_SOCKET_IFNAME", "lo")
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd import rpc_shards
    from lightretriever_amd.retriever import HybridSearch
    opts = rpc.TensorPipeRpcBackendOptions(init_method=f"tcp://127.0.0.1:{port}", _transports=["shm", "uv"], _channels=["cma", "mpt_uv", "basic"])
    rpc.init_rpc(name=f"worker{rank}", rank=rank, world_size=world, rpc_backend_options=opts)
    try:
        cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
        tok, enc, hm, model = build_stack(cfg_o, w)
        rpc_shards.register_worker(model)                       # what PytorchRPCExactSearchModel.__init__ does on every rank
        rpc.api._wait_all_workers(60)
        if rank == 0:
            corpus = synth_corpus(np.random.default_rng(0), 150)
            queries = {"q0": "capital of france", "q1": "dense retrieval models", "q2": "amd instinct memory", "d7": corpus["d7"]["text"]}
            searcher = HybridSearch(model, batch_size=16, corpus_chunk_size=70)
            rpc_shards.PIECE_DOCS = 20                          # a worker's share of a chunk (~35 documents) travels in two pieces
            res = searcher.search(corpus, queries, top_k=12, ignore_identical_ids=True)
            ret["rpc"] = {q: dict(v) for q, v in res.items()}
            ret["workers"] = rpc_shards.rpc_workers()
            # a direct encode call (MTEB's non-retrieval tasks): spans go to the workers, rows come back in input order
            model.corpus_prompt = "passage: "                      # set on the driving rank only, like evaluate_mteb.py does
            docs = list(corpus.values())[:70]
            enc_out = model.encode_corpus(docs, batch_size=16)
            ret["enc"] = enc_out["dense_reps"].cpu().numpy()
            ret["enc_np_type"] = type(model.encode_corpus(docs, batch_size=16, convert_to_tensor=False)["dense_reps"]).__name__
    finally:
        rpc.shutdown()


def test_search_driven_from_rank0_over_rpc_equals_single_process():
    """The unchanged eval driver's launch: shards on the RPC workers, texts out, per-shard top-k back, merge on rank 0 -> the same
    hits (ids and scores) as one process holding the whole corpus."""
    import torch.multiprocessing as mp
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_api import build_stack, synth_corpus
    from helpers import load_model_golden
    from lightretriever_amd.retriever import HybridSearch
    cfg_o, w, _, _, _, _ = load_model_golden("llama_small_d64")
    tok, enc, hm, model = build_stack(cfg_o, w)
    corpus = synth_corpus(np.random.default_rng(0), 150)
    queries = {"q0": "capital of france", "q1": "dense retrieval models", "q2": "amd instinct memory", "d7": corpus["d7"]["text"]}
    want = HybridSearch(model, batch_size=16, corpus_chunk_size=70).search(corpus, queries, top_k=12, ignore_identical_ids=True)
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 31500 + os.getpid() % 1000
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rpc_worker, args=(r, 2, port, ret)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    assert ret["workers"] == ["worker0", "worker1"]
    got = ret["rpc"]
    assert set(got) == set(want) and "d7" not in got["d7"]
    for q in want:
        assert set(got[q]) == set(want[q])
        for pid, sc in want[q].items():
            assert abs(got[q][pid] - sc) < 1e-6
    model.corpus_prompt = "passage: "
    local = model.encode_corpus(list(corpus.values())[:70], batch_size=16)["dense_reps"].cpu().numpy()
    assert ret["enc"].shape == local.shape and np.array_equal(ret["enc"], local) and ret["enc_np_type"] == "ndarray"


def _bench_line(extra_env, *flags):
    """bench.py in a fresh child process (it initialises the GPU itself) -> its JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    env.pop("LRX_FORCE_COLLECTIVE", None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--legs", "encode,search", *flags],
                         env=env, capture_output=True, text=True, timeout=900)
    # (an aborting process group ends stderr with a long backtrace: the lines naming the error come first)
    errors = [l for l in out.stderr.splitlines() if "rror" in l or "xception" in l or "what()" in l]
    assert out.returncode == 0, "\n".join(errors[:20]) + "\n...\n" + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_bench_with_a_forced_one_rank_rccl_group_matches_the_plain_run():
    """VERDICT r3 item 4 (`--gpus 8` has never run with more than one RCCL rank on hardware): LRX_BENCH_FORCE_DIST=1 makes the N = 1 run
    take every step of the N > 1 path -- init_process_group("nccl"), the all-gather of the shard sizes, barrier + MAX reduction around the
    timed regions, wire words -> all_gather_into_tensor -> merge in every search pass.  Its line must carry the distributed bookkeeping and
    agree with the plain run within 3 % (docs/s; the search pays one extra collective + merge per pass: within 15 %)."""
    plain = _bench_line({})
    forced = _bench_line({"LRX_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(29800 + os.getpid() % 1000), "RANK": "0",
                          "WORLD_SIZE": "1", "LOCAL_RANK": "0"}, "--full", "--legs", "encode,search,sharded", "--sharded-rows", "1000000")
    for line in (plain, forced):
        assert line["n_gpus"] == 1 and line["rccl_ranks"] == 1 and line["scaling"] == "weak" and line["steps"] == 4 and line["warmup"] == 1
        s = line["search"]
        assert s["rccl_ranks"] == 1 and s["shard_rows_per_rank"] == [1_000_000] and s["shard_rows"] == 1_000_000 and s["index_rows"] == 1_000_000
        assert s["scaling"].startswith("strong") and s["passes"] == 20
        assert line["config"]["parallelism"] == "dp1" and line["config"]["global_batch"] == 256
        # round 5: the timed mode is the library default (fp32 residual stream) and says so; the queries/sec half of the metric is carried as scalars at
        # the top level, inside `config` / `roofline`, and in `headline` -- the last key of the line
        assert line["config"]["stream_mode"].startswith("fp32-stream") and "fp32-stream" in line["config"]["workload"]
        assert line["search_qps"] == s["value"] == line["config"]["search_qps"] == line["headline"]["search_qps"] and list(line)[-1] == "headline"
        assert line["search_roofline_frac"] == s["roofline"]["frac"] == line["roofline"]["search_frac"] and line["search_alg_bytes"] == s["roofline"]["algorithmic_bytes"]
        assert line["headline"]["docs_per_s"] == line["value"] and line["headline"]["stream_mode"] == line["config"]["stream_mode"]
    # round 6: over a communicator the line also carries BASELINE configs[3] / configs[4] (row-sharded 4096- and 256-wide indexes; here
    # --sharded-rows 1 000 000 on the one rank) and the 8B encoder under weak scaling -- local / exchange / merge split by HIP events
    assert "configs" not in plain
    # (a plain run measures the headline only: the search leg's extras and the per-class table come with --full)
    assert "other_query_counts" not in plain["search"] and plain["search"]["two_in_flight"] is None and plain["roofline"]["per_class_ms_per_step"] is None
    assert "other_query_counts" in forced["search"] and forced["roofline"]["per_class_ms_per_step"]["gemm_swiglu"] > 0
    fc = forced["configs"]
    for key, dim in (("config3_10Mx4096", 4096), ("config4_10Mx256_mrl", 256)):
        c = fc[key]
        assert c["rccl_ranks"] == 1 and c["shard_rows_per_rank"] == [1_000_000] and c["index_rows"] == 1_000_000 and c["dim"] == dim
        assert c["queries_per_s"] > 0 and c["local_search_ms"] > 0 and c["exchange_ms"] > 0 and c["merge_ms"] > 0
        assert c["ms_per_pass"] >= 0.9 * (c["local_search_ms"] + c["exchange_ms"] + c["merge_ms"])
        assert c["two_in_flight"]["identical_to_one_at_a_time"] is True and c["two_in_flight"]["queries_per_s"] > 0
        assert c["roofline"]["bound"] == "hbm" and 0.05 < c["roofline"]["frac"] < 1.0
    e8 = fc["config3_encode_llama31_8b"]
    assert e8["n_gpus"] == 1 and e8["scaling"] == "weak" and e8["docs_per_s"] > 50 and 0.2 < e8["roofline"]["frac"] < 1.0
    assert abs(forced["value"] / plain["value"] - 1) < 0.03, (forced["value"], plain["value"])
    assert forced["search"]["value"] > 0.85 * plain["search"]["value"], (forced["search"]["value"], plain["search"]["value"])
    print("bench N=1 plain %.1f docs/s, %.0f q/s; forced 1-rank RCCL group %.1f docs/s, %.0f q/s" % (
        plain["value"], plain["search"]["value"], forced["value"], forced["search"]["value"]))
