"""GPU parity: every liblrx kernel (called through the C ABI) against the CPU oracle on seeded inputs."""
import os

import numpy as np
import pytest
import torch

import attn_reference as AR
import elementwise_reference as ER
from oracle import lrx_oracle as O
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def bf16_t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev()).to(torch.bfloat16).contiguous()


def f16_t(a: np.ndarray) -> torch.Tensor:
    """q | k | v activations are fp16 since round 3 (the fused QKV + RoPE projection writes fp16)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev()).to(torch.float16).contiguous()


def f32(t: torch.Tensor) -> np.ndarray:
    return t.float().cpu().numpy()


def rnd(rng, *shape, scale=1.0):
    return O.round_bf16(rng.standard_normal(shape).astype(np.float32) * scale)


def bf16_ulp_close(got, want, ulps=1.0, atol=1e-6):
    """|got-want| <= ulps * 2^-8 * |want| (one bf16 ulp is 2^-7 relative at worst; allow rounding-boundary flips)."""
    tol = ulps * (2.0 ** -7) * np.abs(want) + atol
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{bad.sum()} / {bad.size} mismatches, max abs diff {np.abs(got - want).max()}"


def test_embedding_gather_exact():
    from lightretriever_amd import ops
    rng = np.random.default_rng(0)
    table = rnd(rng, 500, 192)
    ids = rng.integers(0, 500, size=1031).astype(np.int32)
    out = ops.embedding_gather(bf16_t(table), torch.from_numpy(ids).to(dev()))
    np.testing.assert_array_equal(f32(out), table[ids])


@pytest.mark.parametrize("rows,H", [(1, 64), (37, 256), (300, 2048), (9, 4096)])
def test_rmsnorm(rows, H):
    from lightretriever_amd import ops
    rng = np.random.default_rng(rows)
    x, w = rnd(rng, rows, H, scale=3.0), O.round_bf16(1 + 0.1 * rng.standard_normal(H).astype(np.float32))
    y = ops.rmsnorm(bf16_t(x), bf16_t(w), 1e-5)
    bf16_ulp_close(f32(y), O.rmsnorm(x, w, 1e-5, bf16=True), ulps=1.01)


@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (300, 192, 128), (256, 256, 64), (777, 1000, 512), (1024, 3072, 2048), (515, 2048, 8192)])
def test_gemm_plain_and_bias(M, N, K):
    from lightretriever_amd import ops
    rng = np.random.default_rng(M + N + K)
    A, B = rnd(rng, M, K), rnd(rng, N, K, scale=0.05)
    bias = rnd(rng, N)
    want = A @ B.T
    got = ops.gemm_bf16_nt(bf16_t(A), bf16_t(B))
    bf16_ulp_close(f32(got), want, ulps=1.01, atol=2e-3)
    got_b = ops.gemm_bf16_nt(bf16_t(A), bf16_t(B), bias=bf16_t(bias))
    bf16_ulp_close(f32(got_b), want + bias, ulps=1.01, atol=2e-3)


def test_gemm_identity_asymmetric():
    """A = I against an asymmetric B catches a transposed C write or a wrong fragment map exactly."""
    from lightretriever_amd import ops
    K = 256
    A = np.eye(K, dtype=np.float32)
    B = (np.arange(320)[:, None] * 3 + np.arange(K)[None, :] % 7).astype(np.float32) % 61  # small ints, bf16-exact
    got = ops.gemm_bf16_nt(bf16_t(A), bf16_t(B))
    np.testing.assert_array_equal(f32(got), O.round_bf16(B.T))


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1000, 2048, 2048), (131, 64, 8192)])
def test_gemm_residual_inplace(M, N, K):
    from lightretriever_amd import ops
    rng = np.random.default_rng(K + M)
    A, B, R = rnd(rng, M, K), rnd(rng, N, K, scale=0.05), rnd(rng, M, N)
    r = bf16_t(R)
    got = ops.gemm_bf16_nt(bf16_t(A), bf16_t(B), resid=r, epilogue=1, out=r)  # C aliases resid
    # reference arithmetic of a bf16 model: residual + linear(x), both bf16 -> bf16(bf16(A B^T) + R).  A 1-ulp flip of the
    # inner rounding (fp32 summation order) moves the result by one ulp of the product, hence the |P| term.
    P = A @ B.T
    want = O.round_bf16(O.round_bf16(P) + R)
    tol = 1.01 * 2.0 ** -7 * (np.abs(P) + np.abs(want)) + 1e-6
    bad = np.abs(f32(got) - want) > tol
    assert not bad.any(), f"{bad.sum()} mismatches, max diff {np.abs(f32(got) - want).max()}"
    assert (f32(got) == want).mean() > 0.97      # and the vast majority is bit-identical to the bf16 reference arithmetic


@pytest.mark.parametrize("M,I,K", [(200, 128, 64), (513, 512, 256), (300, 8192, 2048)])
def test_gemm_swiglu(M, I, K):
    from lightretriever_amd import ops, interleave_gate_up
    rng = np.random.default_rng(I)
    A, Wg, Wu = rnd(rng, M, K), rnd(rng, I, K, scale=0.05), rnd(rng, I, K, scale=0.05)
    wgu = interleave_gate_up(torch.from_numpy(Wg), torch.from_numpy(Wu)).to(dev()).to(torch.bfloat16)
    got = ops.gemm_bf16_nt(bf16_t(A), wgu, epilogue=2)
    g, u = A @ Wg.T, A @ Wu.T
    want = g / (1 + np.exp(-g)) * u
    bf16_ulp_close(f32(got), want, ulps=1.05, atol=2e-3)


def test_positions_match_packing_oracle():
    from lightretriever_amd import ops
    lens = [5, 1, 64, 17, 1, 130]
    mask = np.zeros((len(lens), max(lens)), np.int64)
    for i, n in enumerate(lens):
        mask[i, :n] = 1
    _, pos, _, cu, _ = O.pack_padded(mask.copy(), mask)
    got = ops.build_positions(torch.from_numpy(cu).to(dev()), int(cu[-1]))
    np.testing.assert_array_equal(got.cpu().numpy(), pos)


@pytest.mark.parametrize("d,rope_type", [(64, "llama3"), (128, "default"), (128, "llama3")])
def test_rope_table_is_the_fp32_table_of_the_hf_restatement(d, rope_type):
    """cos/sin are fp32 (LlamaRotaryEmbedding's fp32 values; HF's bf16 run rounds them afterwards, the kernels do not)."""
    from lightretriever_amd import rope_tables, EncoderConfig
    ocfg = O.EncoderConfig(100, 4 * d, 1, 4, 2, d, 64, rope_type=rope_type, rope_original_max_position=64, max_positions=512)
    cfg = EncoderConfig(100, 4 * d, 1, 4, 2, d, 64, rope_type=rope_type, rope_original_max_position=64, max_positions=512)
    cos, sin = rope_tables(cfg)
    oc, osn = O.rope_table(ocfg, 512)
    np.testing.assert_allclose(cos.numpy(), oc, atol=2e-4)             # (fp32 angle position * inv_freq up to ~500 rad: 1 ulp of the angle is 3e-5)
    np.testing.assert_allclose(sin.numpy(), osn, atol=2e-4)


def attn_oracle(qkv, cu, nq, nkv, d):
    T = qkv.shape[0]
    q = qkv[:, :nq * d].reshape(T, nq, d)
    k = qkv[:, nq * d:(nq + nkv) * d].reshape(T, nkv, d)
    v = qkv[:, (nq + nkv) * d:].reshape(T, nkv, d)
    out = np.zeros((T, nq, d), np.float32)
    grp = nq // nkv
    for b in range(len(cu) - 1):
        s, e = cu[b], cu[b + 1]
        L = e - s
        causal = np.tril(np.ones((L, L), bool))
        for hq in range(nq):
            sc = (q[s:e, hq] @ k[s:e, hq // grp].T) * np.float32(d ** -0.5)
            sc = np.where(causal, sc, -np.inf)
            p = np.exp(sc - sc.max(-1, keepdims=True))
            out[s:e, hq] = (p / p.sum(-1, keepdims=True)) @ v[s:e, hq // grp]
    return out.reshape(T, nq * d)


def attn_within_bound(got: torch.Tensor, O64: torch.Tensor, A64: torch.Tensor):
    """the derived bound of tests/attn_reference.py against the float64 reference (beside, not instead of, the numpy oracle's tolerance)"""
    ratio = AR.worst_ratio(got, O64, A64)
    print(f"worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"worst |err| / bound = {ratio:.3f}"


VARLEN_CASES = [
    (64, 4, 2, [1, 2, 31, 32, 33, 63, 64, 65, 100, 128, 129, 200]),
    (64, 8, 2, [512, 7, 300]),
    (64, 2, 2, [96, 5]),
    (128, 2, 1, [1, 64, 65, 130, 257]),
    (128, 4, 1, [512, 33]),
    (128, 12, 2, [200, 64, 1]),      # Qwen2.5-1.5B head layout: GQA group 6 -> two workgroups of 3 heads
    (128, 14, 2, [130, 65]),         # group 7 (Qwen2.5-7B): parts of 4 + 3 heads, one idle wave pair
    (128, 8, 1, [97, 256]),          # group 8: 4 + 4
    (64, 12, 2, [140, 31]),
    (64, 6, 1, [70, 129]),
    (128, 6, 2, [200, 64, 1]),       # group 3 (Llama-3.2-3B: 24 q / 8 kv heads)
    (128, 5, 1, [131, 40]),          # group 5: parts of 3 + 2 heads
    (128, 12, 1, [97, 130]),         # group 12: three workgroups of 4 heads
    (64, 3, 1, [150, 33]),           # groups 3, 5, 7, 16 at head_dim 64: the LDS-resident kernel hands out (head, q block) tasks for any group
    (64, 10, 2, [129, 64]),
    (64, 7, 1, [100, 2]),
    (64, 16, 1, [90, 70]),
    (64, 14, 2, [512, 511, 1]),      # Qwen2.5-0.5B head layout at the resident kernel's longest sequence
    (64, 8, 2, [600, 40]),           # longer than 512 tokens: the tiled kernel at head_dim 64
    (64, 3, 1, [530, 33]),           # ... with an odd group
    (64, 16, 1, [513, 70]),          # ... group 16: two workgroups of 8 heads
    (128, 4, 1, [700, 64]),
]


@pytest.mark.parametrize("d,nq,nkv,lens", VARLEN_CASES)
def test_attention_varlen_causal(d, nq, nkv, lens):
    from lightretriever_amd import ops
    rng = np.random.default_rng(sum(lens) + d)
    T = sum(lens)
    qkv = rnd(rng, T, (nq + 2 * nkv) * d)
    qkv[:, :nq * d] *= 2.0  # peaky softmax
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    got = ops.attn_varlen_causal(f16_t(qkv), torch.from_numpy(cu).to(dev()), max(lens), nq, nkv, d)
    want = attn_oracle(qkv, cu, nq, nkv, d)
    np.testing.assert_allclose(f32(got), want, atol=2e-2, rtol=2e-2)
    # rows are convex combinations of v: a tighter relative check on the row norms catches scale errors
    assert abs(np.linalg.norm(f32(got)) / np.linalg.norm(want) - 1) < 3e-3
    attn_within_bound(got, *AR.causal_gqa_fp64(f16_t(qkv), cu, nq, nkv, d))


def test_attention_forced_max_jump():
    """One key with a huge score late in the sequence forces the online-softmax rescale branch (alpha << 1)."""
    from lightretriever_amd import ops
    rng = np.random.default_rng(5)
    d, nq, nkv, L = 64, 4, 2, 160
    qkv = rnd(rng, L, (nq + 2 * nkv) * d, scale=0.3)
    qkv[100, nq * d:nq * d + d] = O.round_bf16(qkv[150, :d] * 40)  # key 100 (kv head 0) aligned with q row 150 of head 0
    cu = np.array([0, L], np.int32)
    got = ops.attn_varlen_causal(f16_t(qkv), torch.from_numpy(cu).to(dev()), L, nq, nkv, d)
    np.testing.assert_allclose(f32(got), attn_oracle(qkv, cu, nq, nkv, d), atol=2e-2, rtol=2e-2)
    attn_within_bound(got, *AR.causal_gqa_fp64(f16_t(qkv), cu, nq, nkv, d))


def pool_norm_bf16_by_the_rounding_rule(got, x, w, cu, pooling, out_dim, normalize, eps=1e-5):
    """The comparison rule of tests/elementwise_reference.py for k_pool_norm on a bf16 stream: every pooled token's final-norm row is HF's
    bf16(w * bf16(x * rstd)) BIT FOR BIT, except where the float64 x * rstd lies within the kernel's derived fp32 error budget of a bf16
    rounding boundary (either neighbour there; at most 2 % of the elements, proven on the host for these inputs); the mean adds the tokens
    in fp32.  A normalised result is held against the float64 normalisation of the kernel's own un-normalised rows, which are checked first."""
    from lightretriever_amd import ops
    H = x.shape[1]
    _, info = ER.pool_norm(x, w, cu, eps, pooling, out_dim, False, f32=False)
    un = got if not normalize else ops.pool_norm(bf16_t(x), bf16_t(w), torch.from_numpy(np.asarray(cu, np.int32)).to(dev()), eps, out_dim, False, pooling=pooling)
    un = f32(un).astype(np.float64)
    lo, hi, share = ER.pool_allowed(info, w, H, out_dim, f32=False)
    assert share <= ER.NEAR_CAP
    single = np.array([t is not None and len(t) == 1 for t in info["tokens"]])[:, None]
    ok = np.where(single, (un == lo) | (un == hi), (un >= lo) & (un <= hi))
    assert ok.all(), f"{int((~ok).sum())} / {ok.size} elements outside what the rounding rule allows, first at {np.argwhere(~ok)[0].tolist()}"
    if normalize:
        ER.assert_rel(f32(got), ER.l2_normalize(un), ER.normalize_budget(out_dim), "normalised")


@pytest.mark.parametrize("H,out_dim,normalize", [(256, 256, True), (256, 64, True), (2048, 2048, True), (2048, 256, False)])
def test_pool_norm(H, out_dim, normalize):
    from lightretriever_amd import ops
    x, w, cu = ER.legacy_pool_inputs(H, out_dim, [3, 1, 40, 17])                        # (the seeds this test always had)
    got = ops.pool_norm(bf16_t(x), bf16_t(w), torch.from_numpy(cu).to(dev()), 1e-5, out_dim, normalize)
    pool_norm_bf16_by_the_rounding_rule(got, x, w, cu, "lasttoken", out_dim, normalize)
    if normalize:
        np.testing.assert_allclose(np.linalg.norm(f32(got), axis=1), 1.0, atol=1e-5)


@pytest.mark.parametrize("pooling", ["cls", "mean", "lasttoken", "second_to_last", "third_to_last"])
def test_pool_norm_strategies_against_the_reference_pooling(pooling):
    """pooling() of finetune/dense_pooling.py:12-82 (tests/golden/pooling.npz holds its outputs on random tensors): k_pool_norm with an identity
    norm weight on rows pre-scaled to unit RMS is the bare pooling -- 1e-6; then with a real norm on an fp32 stream against the oracle (the
    fp32 norm + fp32 accumulation in token order) and on a bf16 stream (HF's rounding order)."""
    from lightretriever_amd import _lib, ops
    g = np.load(os.path.join(GOLDEN, "pooling.npz"))
    for name in ("ragged", "allfull"):
        h, m = g[f"fn_{name}_hidden"].astype(np.float64), g[f"fn_{name}_mask"]
        # unit-RMS rows go through the norm unchanged (up to eps = 0): the kernel's output is then the reference's pooling of those rows
        hn = (h / np.sqrt((h * h).mean(-1, keepdims=True))).astype(np.float32)
        H = hn.shape[-1]
        pad = np.zeros(hn.shape[:2] + (64 - H,), np.float32)                                   # H = 48 -> 64 columns; zeros keep the mean of squares ...
        hp = np.concatenate([hn, pad], -1) * np.float32(np.sqrt(64 / H))                       # ... once the rows are rescaled to unit RMS over 64
        packed, cu = hp[m.astype(bool)], np.concatenate([[0], np.cumsum(m.sum(1))]).astype(np.int32)
        got = ops.pool_norm(torch.from_numpy(packed).to(dev()), bf16_t(np.ones(64, np.float32)), torch.from_numpy(cu).to(dev()), 0.0, normalize=False,
                            pooling=pooling)
        want = O.pool_padded(hn, m, pooling)
        np.testing.assert_allclose(f32(got)[:, :H] / np.float32(np.sqrt(64 / H)), want, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(O.pool_padded(g[f"fn_{name}_hidden"], m, pooling), g[f"fn_{name}_{pooling}"], atol=1e-6)   # (the restatement is the reference's)
    x, w, cu = ER.legacy_strategy_inputs([3, 40, 17, 129, 5])                            # (the seed this test always had)
    for out_dim, normalize in ((256, True), (64, True), (256, False)):
        got32 = ops.pool_norm(torch.from_numpy(x).to(dev()), bf16_t(w), torch.from_numpy(cu).to(dev()), 1e-5, out_dim, normalize, pooling=pooling)
        pooled = O.pool_packed(O.rmsnorm(x, w, 1e-5, bf16=False), cu, pooling)[:, :out_dim]
        np.testing.assert_allclose(f32(got32), O.l2_normalize(pooled) if normalize else pooled, atol=2e-5, rtol=1e-5)
        got16 = ops.pool_norm(bf16_t(x), bf16_t(w), torch.from_numpy(cu).to(dev()), 1e-5, out_dim, normalize, pooling=pooling)
        pool_norm_bf16_by_the_rounding_rule(got16, x, w, cu, pooling, out_dim, normalize)
    # the two-layer strategies need a second hidden state: not this entry point's (lrx_encode_packed_pooled serves them) -- refused, not guessed
    if pooling == "mean":
        for st in ("avg_first_last", "avg_top2"):
            with pytest.raises(Exception, match="other hidden state"):
                ops.pool_norm(torch.from_numpy(x).to(dev()), bf16_t(w), torch.from_numpy(cu).to(dev()), 1e-5, out_dim, True, pooling=st)
    # a sequence shorter than the strategy needs (the reference asserts, dense_pooling.py:63-66): a zero row + the input-error counter
    if pooling in ("second_to_last", "third_to_last"):
        lib = _lib.lib()
        lib.lrx_device_error_count(1)
        cu1 = torch.tensor([0, 1, 6], dtype=torch.int32, device=dev())
        out = ops.pool_norm(torch.from_numpy(x[:6]).to(dev()), bf16_t(w), cu1, 1e-5, normalize=True, pooling=pooling)
        assert float(out[0].abs().max()) == 0.0 and float(out[1].norm()) > 0.99 and lib.lrx_device_error_count(1) == 1


def test_embedding_bag_bit_exact():
    from lightretriever_amd import ops
    rng = np.random.default_rng(11)
    V, H, pad = 300, 256, 7
    table = rng.standard_normal((V, H)).astype(np.float32)
    lens = [5, 0, 1, 17, 3, 0]
    ids = rng.integers(0, V, size=sum(lens)).astype(np.int64)
    ids[2] = pad
    ids[-1] = pad
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    tt, ti, to = torch.from_numpy(table).to(dev()), torch.from_numpy(ids).to(dev()), torch.from_numpy(offs).to(dev())
    raw = ops.embedding_bag_mean(tt, ti, to, padding_idx=pad)
    np.testing.assert_array_equal(f32(raw), O.embedding_bag_mean(table, ids, offs, pad))   # same fp32 summation order
    emb = ops.embedding_bag_mean(tt, ti, to, padding_idx=pad, out_dim=64, normalize=True)
    np.testing.assert_allclose(f32(emb), O.encode_query_emb(table, ids, offs, pad, dense_shrink_dim=64), atol=1e-6)
    # and against torch.nn.EmbeddingBag itself (the reference's query operator) on the same device
    bag = torch.nn.EmbeddingBag.from_pretrained(tt, padding_idx=pad)
    np.testing.assert_allclose(f32(raw), f32(bag(ti, to)), atol=1e-6)
    # round 2 kernel: bags longer than one 256-id chunk, the 2048-wide rows of the 1B table, an output width that is not a multiple
    # of four (scalar path), out-of-range ids counted in the divisor but not summed -- all still the sequential fp32 sums
    V2, H2 = 500, 2048
    table2 = rng.standard_normal((V2, H2)).astype(np.float32)
    lens2 = [600, 1, 257, 0, 32]
    ids2 = rng.integers(0, V2, size=sum(lens2)).astype(np.int64)
    ids2[[3, 300, 599, 700]] = pad
    offs2 = np.concatenate([[0], np.cumsum(lens2)[:-1]]).astype(np.int64)
    t2, i2, o2 = torch.from_numpy(table2).to(dev()), torch.from_numpy(ids2).to(dev()), torch.from_numpy(offs2).to(dev())
    np.testing.assert_array_equal(f32(ops.embedding_bag_mean(t2, i2, o2, padding_idx=pad)), O.embedding_bag_mean(table2, ids2, offs2, pad))
    np.testing.assert_array_equal(f32(ops.embedding_bag_mean(t2, i2, o2, padding_idx=pad, out_dim=250)), O.embedding_bag_mean(table2, ids2, offs2, pad)[:, :250])
    np.testing.assert_allclose(f32(ops.embedding_bag_mean(t2, i2, o2, padding_idx=pad, out_dim=256, normalize=True)),
                               O.encode_query_emb(table2, ids2, offs2, pad, dense_shrink_dim=256), atol=1e-6)
    ids3 = ids2.copy(); ids3[[10, 650]] = V2 + 5          # out of range: skipped in the sum, counted like the scalar kernel does
    i3 = torch.from_numpy(ids3).to(dev())
    a4 = f32(ops.embedding_bag_mean(t2, i3, o2, padding_idx=pad))
    a1 = f32(ops.embedding_bag_mean(t2, i3, o2, padding_idx=pad, out_dim=2047))
    np.testing.assert_array_equal(a4[:, :2047], a1)


def test_attention_last_tile_only_and_gather():
    """The pooled tail of the final layer: only the q tile holding each sequence's last token is computed, and those
    rows are bit-identical to the full kernel's rows; gather_last_rows compacts them."""
    from lightretriever_amd import ops
    rng = np.random.default_rng(21)
    d, nq, nkv, lens = 64, 8, 2, [1, 64, 65, 200, 512, 129]
    T = sum(lens)
    qkv = f16_t(rnd(rng, T, (nq + 2 * nkv) * d))
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(dev())
    full = ops.attn_varlen_causal(qkv, cu, max(lens), nq, nkv, d)
    last = ops.attn_varlen_causal(qkv, cu, max(lens), nq, nkv, d, last_tile_only=True)
    g_full, g_last = ops.gather_last_rows(full, cu), ops.gather_last_rows(last, cu)
    assert torch.equal(g_full, g_last)
    cu_h = cu.cpu().numpy()
    np.testing.assert_array_equal(f32(g_full), f32(full)[cu_h[1:] - 1])
    for b, n in enumerate(lens):      # rows outside the last tile were not touched (zeros), rows inside match
        t0 = ((n - 1) // 64) * 64
        assert torch.equal(last[cu_h[b] + t0:cu_h[b + 1]], full[cu_h[b] + t0:cu_h[b + 1]])
        assert (last[cu_h[b]:cu_h[b] + t0] == 0).all()


@pytest.mark.parametrize("d,nq,nkv,bias,scaled", [(64, 4, 2, False, False), (128, 2, 1, True, True), (64, 32, 8, False, True), (128, 6, 2, True, False)])
def test_gemm_qkv_rope_fused_equals_fp32_projection_then_rope(d, nq, nkv, bias, scaled):
    """lrx_gemm_qkv_rope_fused (round 3): weights / bias in rotary-pair order, rotation on the fp32 accumulators with the fp32 table, fp16
    out in pair order == fp32 x W^T (* row scale) + b, apply_rotary_pos_emb (modeling_llama.py:130-160) in fp32, ONE rounding to fp16."""
    from lightretriever_amd import ops, rope_tables, EncoderConfig
    rng = np.random.default_rng(d + nq)
    T, K = 333, 256
    N = (nq + 2 * nkv) * d
    cfg = EncoderConfig(100, nq * d, 1, nq, nkv, d, 64, rope_type="llama3", rope_original_max_position=64, max_positions=128)
    cos, sin = rope_tables(cfg)
    cos, sin = cos.to(dev()), sin.to(dev())
    A, W = bf16_t(rnd(rng, T, K)), bf16_t(rnd(rng, N, K, scale=0.05))
    b = bf16_t(rnd(rng, N)) if bias else None
    rs = torch.from_numpy(rng.uniform(0.2, 3.0, size=T).astype(np.float32)).to(dev()) if scaled else None
    pos = torch.from_numpy(rng.integers(0, 128, size=T).astype(np.int32)).to(dev())
    t = A.double() @ W.double().T
    if scaled:
        t = t * rs.double()[:, None]
    if bias:
        t = t + b.double()
    qk = t[:, :(nq + nkv) * d].reshape(T, nq + nkv, d)
    c, s_ = cos[pos.long()].double()[:, None, :], sin[pos.long()].double()[:, None, :]
    x1, x2 = qk[..., :d // 2], qk[..., d // 2:]
    want = torch.cat([torch.cat([x1 * c - x2 * s_, x2 * c + x1 * s_], -1).reshape(T, -1), t[:, (nq + nkv) * d:]], 1).float()
    perm = ops.rotary_pair_order(nq, nkv, d).to(dev())
    got_p = ops.gemm_qkv_rope(A, W[perm].contiguous(), pos, cos, sin, nq, nkv, d, bias=b[perm].contiguous() if bias else None, rscale=rs)
    assert got_p.dtype == torch.float16
    got = torch.empty_like(got_p)
    got[:, perm] = got_p                                                    # back to the logical column order
    diff = (got.float() - want).abs()
    assert (diff <= 2.0 ** -10 * want.abs() + 2e-4).all(), diff.max()        # one fp16 rounding (+ fp32 accumulation order)
    assert (got == want.to(torch.float16)).float().mean() > 0.99
    assert torch.equal(perm[(nq + nkv) * d:], torch.arange((nq + nkv) * d, N, device=perm.device))    # v columns stay in place


PREFIX_SUFFIX_CASES = [(64, 4, 2, 9, 2, 37), (64, 32, 8, 22, 2, 5), (128, 8, 1, 3, 3, 11), (64, 2, 2, 0, 2, 4), (128, 4, 4, 40, 1, 3),
                                              # round 2: the matrix-core kernel (P1 <= 64): 32-sequence blocks with a ragged tail, two prefix tiles,
                                              # GQA groups of 6 (Qwen2.5-1.5B) and 4 suffix tokens; and shapes that keep the VALU kernel
                                              (64, 32, 8, 21, 2, 100), (64, 8, 8, 33, 2, 65), (128, 12, 2, 21, 2, 70), (128, 32, 8, 64, 2, 33), (64, 4, 1, 1, 4, 64),
                                              (64, 8, 2, 70, 2, 9), (128, 28, 4, 21, 2, 40)]


@pytest.mark.parametrize("d,nq,nkv,P1,S2,n", PREFIX_SUFFIX_CASES)
def test_attention_prefix_suffix_equals_full_causal(d, nq, nkv, P1, S2, n):
    """Suffix queries over a shared prefix == the suffix rows of full causal attention on [prefix + suffix] per sequence."""
    from lightretriever_amd import ops
    rng = np.random.default_rng(d + nq + P1 + n)
    W = (nq + 2 * nkv) * d
    pre = rnd(rng, P1, W)
    suf = rnd(rng, n * S2, W)
    suf[:, :nq * d] *= 2.0
    prefix_kv = np.ascontiguousarray(pre[:, nq * d:])
    got_t = ops.attn_prefix_suffix(f16_t(suf), f16_t(prefix_kv).reshape(P1, 2 * nkv * d), n, S2, nq, nkv, d)
    got = f32(got_t)
    L = P1 + S2
    full = np.concatenate([np.concatenate([pre, suf[i * S2:(i + 1) * S2]]) for i in range(n)])
    cu = (np.arange(n + 1) * L).astype(np.int32)
    want = attn_oracle(full, cu, nq, nkv, d).reshape(n, L, nq * d)[:, P1:].reshape(n * S2, nq * d)
    np.testing.assert_allclose(got, want, atol=2e-2, rtol=2e-2)
    assert abs(np.linalg.norm(got) / np.linalg.norm(want) - 1) < 3e-3
    attn_within_bound(got_t, *AR.prefix_suffix_fp64(f16_t(suf), f16_t(prefix_kv).reshape(P1, 2 * nkv * d), n, S2, nq, nkv, d))


def test_uniform_layout():
    from lightretriever_amd import ops
    cu, pos = ops.uniform_layout(7, 3, 11, dev())
    assert cu.cpu().tolist() == [0, 3, 6, 9, 12, 15, 18, 21]
    assert pos.cpu().tolist() == [11, 12, 13] * 7


# ---- folded RMSNorm: row scale applied to the accumulator, sum of squares emitted by the residual epilogue ----------------
@pytest.mark.parametrize("M,H,I", [(300, 256, 128), (1000, 2048, 512), (77, 1536, 256)])
def test_folded_norm_gemms_equal_norm_then_gemm(M, H, I):
    """x -> RMSNorm(gamma) -> SwiGLU GEMM == SwiGLU GEMM on x with gamma folded into the weights and the row scale applied to the fp32
    accumulator, up to the two bf16 roundings of the normalised activations that the folded form no longer does; and the residual
    epilogue's per-tile sums of squares reproduce the statistic of the rows it wrote."""
    from lightretriever_amd import ops
    from lightretriever_amd.encoder import interleave_gate_up
    rng = np.random.default_rng(M + H)
    eps = 1e-5
    x = rnd(rng, M, H, scale=1.7)
    gamma = O.round_bf16(1.0 + 0.3 * rng.standard_normal(H).astype(np.float32))
    Wg, Wu = rnd(rng, I, H, scale=0.05), rnd(rng, I, H, scale=0.05)
    r = (1.0 / np.sqrt((x.astype(np.float64) ** 2).mean(1) + eps)).astype(np.float32)
    got_r = f32(ops.row_rscale(bf16_t(x), eps))
    np.testing.assert_allclose(got_r, r, rtol=3e-6)
    # exact-arithmetic target: silu(g) * u with g, u = (r x * gamma) . W^T in fp32/fp64
    hn = (x * r[:, None] * gamma[None, :]).astype(np.float64)
    g, u = hn @ Wg.T.astype(np.float64), hn @ Wu.T.astype(np.float64)
    want = (g / (1 + np.exp(-g)) * u).astype(np.float32)
    Wgu_f = interleave_gate_up(torch.from_numpy(O.round_bf16(Wg * gamma[None, :])), torch.from_numpy(O.round_bf16(Wu * gamma[None, :])))
    got, _ = ops.gemm_bf16_nt_fused(bf16_t(x), Wgu_f.to("cuda").to(torch.bfloat16).contiguous(), epilogue=2, rscale=torch.from_numpy(r).cuda())
    # the unfolded pipeline on the same inputs: normalised rows rounded to bf16 (twice, like LlamaRMSNorm), plain SwiGLU GEMM
    hn16 = ops.rmsnorm(bf16_t(x), bf16_t(gamma), eps)
    Wgu = interleave_gate_up(torch.from_numpy(Wg), torch.from_numpy(Wu)).to("cuda").to(torch.bfloat16).contiguous()
    ref16 = f32(ops.gemm_bf16_nt(hn16, Wgu, epilogue=2))
    rel = lambda a: np.linalg.norm(a - want) / np.linalg.norm(want)
    assert rel(f32(got)) < 6e-3 and rel(f32(got)) <= 1.25 * rel(ref16)       # at least as close to exact arithmetic as the HF rounding order
    assert abs(np.linalg.norm(f32(got)) / np.linalg.norm(want) - 1) < 2e-3
    # residual epilogue: out = bf16(bf16(act . Wd^T) + x); ss_part sums to the sum of squares of the rows written
    act, Wd = rnd(rng, M, I), rnd(rng, H, I, scale=0.05)
    out, ss = ops.gemm_bf16_nt_fused(bf16_t(act), bf16_t(Wd), resid=bf16_t(x), epilogue=1, want_ss=True)
    assert ss.shape == ((H + 255) // 256, M) and torch.isfinite(ss).all()
    want_ss = (out.float() ** 2).sum(1)
    np.testing.assert_allclose(f32(ss.sum(0)), f32(want_ss), rtol=2e-6)
    np.testing.assert_allclose(f32(ops.finalize_rscale(ss, H, eps)), 1.0 / np.sqrt(f32(want_ss) / H + eps), rtol=3e-6)
    out2, ss2 = ops.gemm_bf16_nt_fused(bf16_t(act), bf16_t(Wd), resid=bf16_t(x), epilogue=1, want_ss=True)
    assert torch.equal(ss, ss2) and torch.equal(out, out2)                                         # no atomics: bitwise repeatable


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1000, 2048, 2048), (131, 64, 512), (513, 1536, 8960)])
def test_precise_stream_residual_gemm(M, N, K):
    """lrx_gemm_bf16_nt_resid32 (round 3): x32 += A . B^T with one rounding to fp32, a16 = bf16(x32 * gamma), ss_part from the fp32 row."""
    from lightretriever_amd import ops
    rng = np.random.default_rng(M + N)
    A, B = rnd(rng, M, K), rnd(rng, N, K, scale=0.05)
    x0 = (rng.standard_normal((M, N)) * 3).astype(np.float32)
    gamma = O.round_bf16(1.0 + 0.3 * rng.standard_normal(N).astype(np.float32))
    x32 = torch.from_numpy(x0.copy()).cuda()
    a16, ss = ops.gemm_resid32(bf16_t(A), bf16_t(B), x32, gamma=bf16_t(gamma), want_ss=True)
    want = x0.astype(np.float64) + A.astype(np.float64) @ B.astype(np.float64).T
    np.testing.assert_allclose(f32(x32), want, rtol=3e-6, atol=1e-5 * max(1.0, (K / 128) ** 0.5))     # fp32 accumulation over K products
    wa = torch.from_numpy((f32(x32) * gamma[None, :]).astype(np.float32)).to(torch.bfloat16)
    assert (a16.cpu() == wa).float().mean() > 0.999 and bf16_ulp_close(f32(a16), wa.float().numpy(), ulps=1.01) is None
    np.testing.assert_allclose(f32(ss.sum(0)), (f32(x32).astype(np.float64) ** 2).sum(1), rtol=3e-6)
    # repeatable bit for bit (no atomics), and without the optional outputs
    x32b = torch.from_numpy(x0.copy()).cuda()
    a16b, ssb = ops.gemm_resid32(bf16_t(A), bf16_t(B), x32b, gamma=bf16_t(gamma), want_ss=True)
    assert torch.equal(x32, x32b) and torch.equal(a16, a16b) and torch.equal(ss, ssb)
    x32c = torch.from_numpy(x0.copy()).cuda()
    a_none, ss_none = ops.gemm_resid32(bf16_t(A), bf16_t(B), x32c, want_a16=False)
    assert a_none is None and ss_none is None and torch.equal(x32c, x32)


def test_precise_stream_embedding_and_final_norm():
    from lightretriever_amd import _lib, ops
    rng = np.random.default_rng(2)
    V, H, eps = 90, 320, 1e-5
    table = bf16_t(rnd(rng, V, H))
    gamma = bf16_t(O.round_bf16(1.0 + 0.2 * rng.standard_normal(H).astype(np.float32)))
    ids = torch.tensor([3, 89, 0, 17, 90, -2], dtype=torch.int32, device="cuda")
    _lib.lib().lrx_device_error_count(1)
    x32, a16, rs = ops.embed_stream32(table, ids, gamma, eps)
    good = [0, 1, 2, 3]
    assert torch.equal(x32[good], table[ids[good].long()].float()) and (x32[4:] == 0).all()
    assert torch.equal(a16[good], (table[ids[good].long()].float() * gamma.float()).to(torch.bfloat16))
    np.testing.assert_allclose(f32(rs)[good], 1.0 / np.sqrt((f32(x32)[good].astype(np.float64) ** 2).mean(1) + eps), rtol=2e-6)
    assert _lib.lib().lrx_device_error_count(1) == 2
    x = torch.from_numpy((rng.standard_normal((37, H)) * 5).astype(np.float32)).cuda()
    y = ops.rmsnorm_f32(x, gamma, eps)
    want = (x.double() * torch.rsqrt(x.double().pow(2).mean(1, keepdim=True) + eps) * gamma.double()).float()
    assert bf16_ulp_close(f32(y), f32(want.to(torch.bfloat16)), ulps=1.01) is None
    cu = torch.tensor([0, 10, 11, 37], dtype=torch.int32, device="cuda")
    p32 = ops.pool_norm(x, gamma, cu, eps)                                   # fp32 rows: fp32 norm, no bf16 rounding inside
    wantp = torch.nn.functional.normalize(want.double()[cu[1:].long() - 1] * 0 + (x.double() * torch.rsqrt(x.double().pow(2).mean(1, keepdim=True) + eps)
                                                                                  * gamma.double())[cu[1:].long() - 1], dim=-1)
    np.testing.assert_allclose(f32(p32), wantp.float().cpu().numpy(), atol=2e-6)


@pytest.mark.parametrize("name", ["llama_small_d64", "llama_small_d128"])
def test_precise_stream_encoder_is_closer_to_fp32_than_the_bf16_stream(name):
    """The same checkpoint through the bf16-stream pipeline and the precise one (fp32 stream, exact weights, norm weight on the operand):
    both inside the reference's bf16 band; the precise one closer to the fp32 golden; encode_hidden / prefixed follow the same mode."""
    from dataclasses import asdict, replace
    from helpers import load_model_golden, min_cos
    from lightretriever_amd import EncoderConfig, LrxEncoder
    cfg_o, w, g, ids, cu, max_len = load_model_golden(name)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    tid, tcu = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    out, hid = {}, {}
    # lrx_encoder_config.precise_stream: 0 = bf16 stream (folded norms), 1 = fp32 stream with bf16 GEMM operands, 2 = with fp16 operands (round 6,
    # on request), 3 = with the QKV projection's operands in fp16 (round 6: the default)
    for mode, (precise, operands) in ((0, (False, None)), (1, (True, "bf16")), (2, (True, "fp16")), (3, (True, None))):
        enc = LrxEncoder(replace(EncoderConfig(**asdict(cfg_o)), precise_stream=precise, operand_dtype=operands), sd)
        assert enc._ccfg.precise_stream == mode and enc._ccfg.norm_folded == int(not precise)
        assert enc.operand_mode == ("bf16", "bf16", "fp16", "fp16_qkv")[mode] and enc.operand_f16 == (mode == 2)
        out[mode] = enc.encode_packed(tid, tcu, max_len).cpu().numpy()
        hid[mode] = enc.encode_hidden(tid, tcu, max_len).float()
        pooled = torch.nn.functional.normalize(hid[mode][tcu[1:].long() - 1], dim=-1).cpu().numpy()
        assert min_cos(pooled, out[mode]) > 1 - 2e-5                         # pooled tail == pooling the full forward (bf16 hidden output)
    ref = g["dense_reps"]
    e_fast, e_prec, e_f16, e_qkv = (1 - min_cos(out[m], ref) for m in (0, 1, 2, 3))
    print("%s: 1 - cos vs the reference's fp32 output: bf16 stream %.2e, fp32 stream + bf16 operands %.2e, + fp16 QKV operands %.2e, + fp16 operands %.2e" % (
        name, e_fast, e_prec, e_qkv, e_f16))
    assert e_prec <= max(1e-4, 0.8 * e_fast), (e_prec, e_fast)
    assert e_f16 <= max(1e-5, 0.5 * e_prec), (e_f16, e_prec)                  # three more mantissa bits on every GEMM operand
    assert e_qkv <= max(1e-5, e_prec), (e_qkv, e_prec)                        # ... on the QKV projection's alone
    assert min_cos(out[1], out[0]) > 0.999 and min_cos(out[2], out[1]) > 0.9995 and min_cos(out[3], out[1]) > 0.9995
    with pytest.raises(ValueError):                                           # fp16 operands belong to the fp32 stream
        LrxEncoder(replace(EncoderConfig(**asdict(cfg_o)), precise_stream=False, operand_dtype="fp16"), sd)


def test_fp16_operands_are_refused_where_fp16_cannot_hold_them():
    """The two ways a checkpoint can leave fp16's range.  (1) Projection weights scaled below fp16's subnormals (the scale moved into the norm weight:
    the same function in bf16 / fp32): the load-time check keeps bf16 operands by default, with a warning, and refuses an explicit 'fp16_qkv'.
    (2) An activation operand x * gamma beyond 65504 with weights that convert fine (gamma scaled up, nothing scaled down): the store saturates and
    the saturation counter -- the one LrxExactSearchModel turns into an error -- counts it; bf16 operands take the same checkpoint without a count
    from the operand (q|k|v saturate on their own there, so that side is not asserted)."""
    import warnings
    from dataclasses import asdict, replace
    from helpers import load_model_golden
    from lightretriever_amd import EncoderConfig, LrxEncoder, _lib
    cfg_o, w, _, ids, cu, max_len = load_model_golden("llama_small_d64")
    tid, tcu = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    base = EncoderConfig(**asdict(cfg_o))
    # (1) wqkv * 2^-30, input_layernorm * 2^30: exact in bf16, gone in fp16
    sd = {k: torch.from_numpy(v).clone() for k, v in w.items()}
    for k in list(sd):
        if k.endswith(("q_proj.weight", "k_proj.weight", "v_proj.weight")):
            sd[k] = (sd[k].float() * 2.0 ** -30).to(torch.bfloat16)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        enc = LrxEncoder(base, sd)
    assert enc.operand_mode == "bf16" and any("fp16" in str(r.message) for r in rec)
    with pytest.raises(ValueError, match="fp16"):
        LrxEncoder(replace(base, operand_dtype="fp16_qkv"), sd)
    # (2) input_layernorm * 2^40 on the original projections: x * gamma ~ 1e10
    sd2 = {k: torch.from_numpy(v).clone() for k, v in w.items()}
    for k in list(sd2):
        if k.endswith("input_layernorm.weight"):
            sd2[k] = (sd2[k].float() * 2.0 ** 40).to(torch.bfloat16)
    lib = _lib.lib()
    enc2 = LrxEncoder(base, sd2)
    assert enc2.operand_mode == "fp16_qkv"
    lib.lrx_device_saturation_count(1)
    enc2.encode_packed(tid, tcu, max_len)
    torch.cuda.synchronize()
    assert lib.lrx_device_saturation_count(1) > 0


@pytest.mark.parametrize("operands", [None, "fp16", "bf16"])
@pytest.mark.parametrize("name", ["llama_small_d64", "qwen2_small"])
def test_precise_stream_covers_every_encode_entry_point(name, operands):
    """The fp32 residual stream (bf16 and fp16 GEMM operands) through the other users of the layer loop: lrx_encode_packed_sparse (dense rows equal lrx_encode_packed's, sparse
    rows track the bf16-stream ones), lrx_encode_prefixed (shared prefix == the same sequences encoded in full), ragged batches with a
    one-token sequence, and a Qwen-style model (q|k|v bias in rotary-pair order)."""
    from dataclasses import asdict, replace
    from helpers import load_model_golden, min_cos
    from lightretriever_amd import EncoderConfig, LrxEncoder
    if name == "qwen2_small":
        cfg_o = O.EncoderConfig(vocab_size=300, hidden_size=256, num_layers=3, num_q_heads=2, num_kv_heads=1, head_dim=128, intermediate_size=320,
                                rms_eps=1e-6, rope_theta=1e6, rope_type="default", qkv_bias=True, max_positions=256)
        w = O.random_weights(cfg_o, seed=9, std=0.05)
        rng = np.random.default_rng(3)
        lens = [70, 1, 33, 128, 5]
        ids = rng.integers(0, 300, size=sum(lens)).astype(np.int32)
        cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        max_len = max(lens)
    else:
        cfg_o, w, _, ids, cu, max_len = load_model_golden(name)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    tid, tcu = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    want = O.encode_passage(cfg_o, w, ids, cu, bf16=False)
    encs = {p: LrxEncoder(replace(EncoderConfig(**asdict(cfg_o)), precise_stream=p, operand_dtype=operands if p else None), sd) for p in (False, True)}
    assert encs[True].operand_mode == (operands or "fp16_qkv")
    out = {p: e.encode_packed(tid, tcu, max_len) for p, e in encs.items()}
    assert 1 - min_cos(out[True].cpu().numpy(), want) <= max(1e-4, 0.8 * (1 - min_cos(out[False].cpu().numpy(), want)))
    dense, sparse = encs[True].encode_packed_sparse(tid, tcu, max_len)
    assert torch.allclose(dense, out[True], atol=1e-6)                              # (pooled tail vs full last layer: same rows)
    _, sparse_b = encs[False].encode_packed_sparse(tid, tcu, max_len)
    nz = (sparse > 0) | (sparse_b > 0)
    assert (sparse[nz] - sparse_b[nz]).abs().max() < 0.15 and ((sparse > 0) == (sparse_b > 0)).float().mean() > 0.99
    # shared-prefix encode in the precise mode == the same sequences encoded in full
    B, P1, S2 = 9, 6, 2
    rng = np.random.default_rng(1)
    prefix = torch.from_numpy(rng.integers(0, cfg_o.vocab_size, size=P1).astype(np.int32)).cuda()
    suffix = torch.from_numpy(rng.integers(0, cfg_o.vocab_size, size=(B, S2)).astype(np.int32)).cuda()
    fast = encs[True].encode_prefixed(prefix, suffix)
    full_ids = torch.cat([torch.cat([prefix, suffix[b]]) for b in range(B)]).contiguous()
    full_cu = (torch.arange(B + 1, dtype=torch.int32, device="cuda") * (P1 + S2)).contiguous()
    full = encs[True].encode_packed(full_ids, full_cu, P1 + S2, normalize=False)
    assert min_cos(fast.cpu().numpy(), full.cpu().numpy()) > 1 - 2e-4 and torch.allclose(fast.norm(dim=1), full.norm(dim=1), rtol=5e-3)


def test_folded_and_unfolded_encoders_agree_and_both_match_fp32():
    """Same checkpoint through both pipelines: pooled embeddings within bf16 noise of each other, and the folded one is not
    further from the fp32 oracle than the HF rounding order is."""
    from dataclasses import asdict, replace
    from helpers import load_model_golden, min_cos
    from lightretriever_amd import EncoderConfig, LrxEncoder
    cfg_o, w, g, ids, cu, max_len = load_model_golden("llama_small_d64")
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    outs = {}
    for fold in (True, False):
        enc = LrxEncoder(replace(EncoderConfig(**asdict(cfg_o)), fold_norm=fold), sd)
        outs[fold] = enc.encode_packed(torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), max_len).cpu().numpy()
    assert min_cos(outs[True], outs[False]) > 0.9995
    ref = g["dense_reps"]
    assert min_cos(outs[True], ref) > 0.999 and min_cos(outs[True], ref) >= min_cos(outs[False], ref) - 2e-4


def test_embedding_gather_never_reads_outside_the_table():
    """an out-of-range / negative token id gives a zero row and raises the device-side counter instead of an
    out-of-bounds HBM read; the fused encoder uses the same kernel."""
    from lightretriever_amd import _lib, ops
    lib = _lib.lib()
    lib.lrx_device_error_count(1)
    table = torch.randn(50, 64, device="cuda").bfloat16()
    ids = torch.tensor([0, 49, 50, -1, 7, 1 << 30], dtype=torch.int32, device="cuda")
    out = ops.embedding_gather(table, ids)
    assert torch.equal(out[[0, 1, 4]], table[[0, 49, 7]]) and (out[[2, 3, 5]] == 0).all()
    assert lib.lrx_device_error_count(1) == 3 and lib.lrx_device_error_count(0) == 0
