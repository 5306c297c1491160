"""The dispatch of the encoder's layer loop (run_layers in lightretriever_amd/csrc/lrx_capi.hip) against the same chain written in Python from
the exported kernel calls, BIT FOR BIT, in the three operand modes.

The kernel-level tests pin each instantiation on its own (tests/test_gpu_gemm_reference.py, test_gpu_attn_reference.py,
test_gpu_elementwise_reference.py); what they cannot see is which instantiation the encoder launches where.  The format flags of run_layers:

                                     "bf16" (precise_stream 1)   "fp16" (2)    "fp16_qkv" (3, the default)
  embedding: a16                     bf16                        fp16          fp16            f16q
  QKV projection: A, wqkv            bf16                        fp16          fp16            f16q
  attention: output                  bf16                        fp16          bf16            mode == 2
  o-projection: A, wo | a16          bf16 | bf16                 fp16 | fp16   bf16 | bf16     f16 | f16
  gate-up + SwiGLU: A, wgu, output   bf16                        fp16          bf16            f16
  down-projection: A, wdown | a16    bf16 | bf16                 fp16 | fp16   bf16 | fp16     f16 | f16q

The o-projection and the down-projection differ in mode 3 only.  Every step of the chain is deterministic (fixed summation orders, no float
atomics), so the hidden states of lrx_encode_hidden must equal the chain's to the bit; a flag handed to the wrong launch feeds a GEMM the
wrong format's bits and changes every element.  One tiny configuration: 2 layers, H = 256, I = 512, 4 / 2 heads of 64, 300 tokens."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ("bf16", "fp16", "fp16_qkv")
LENS = [97, 130, 73]


@functools.lru_cache(maxsize=None)
def _encoder(mode):
    from lightretriever_amd.encoder import EncoderConfig, LrxEncoder
    cfg = EncoderConfig(vocab_size=512, hidden_size=256, num_layers=2, num_q_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=512,
                        qkv_bias=True, max_positions=256, precise_stream=True, operand_dtype=mode)
    enc = LrxEncoder.random_init(cfg, seed=3, std=0.05)
    assert enc.operand_mode == mode
    return enc


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 512, (sum(LENS),), generator=g, dtype=torch.int32).cuda()
    cu = torch.tensor([0] + LENS, dtype=torch.int64).cumsum(0).to(torch.int32).cuda()
    return ids, cu


def chain(enc, ids, cu):
    """run_layers + the final norm of lrx_encode_hidden, from the exported calls, in its order and with its flags"""
    from lightretriever_amd import ops
    c, mode = enc.cfg, enc.operand_mode
    f16, f16q = mode == "fp16", mode in ("fp16", "fp16_qkv")
    fmt = lambda flag: "fp16" if flag else "bf16"
    dt = lambda flag: torch.float16 if flag else torch.bfloat16
    T, H, nq, nkv, d, eps = ids.numel(), c.hidden_size, c.num_q_heads, c.num_kv_heads, c.head_dim, c.rms_eps
    max_seqlen = max(LENS)
    pos = ops.build_positions(cu, T)
    items = ops.attn_work_list(cu, T, max_seqlen, nq, nkv, d)
    x32, a, rsA = ops.embed_stream32(enc.embed, ids, enc.layers[0]["ln1"], eps, a16_dtype=dt(f16q))
    for l, L in enumerate(enc.layers):
        last = l == c.num_layers - 1
        qkv = torch.empty(T, (nq + 2 * nkv) * d, dtype=torch.float16, device=ids.device)
        ops.gemm_qkv_rope_slice(a, L["wqkv_c"], pos, enc.rope_cos, enc.rope_sin, nq, nkv, d, 0, nq + 2 * nkv, qkv, bias=L["bqkv_c"], rscale=rsA,
                                operands=fmt(f16q))
        h = ops.attn_varlen_causal(qkv, cu, max_seqlen, nq, nkv, d, work_list=items, out_dtype=dt(f16))
        a, ss = ops.gemm_resid32(h, L["wo_c"], x32, gamma=L["ln2"], want_ss=True, operands=fmt(f16), a16_dtype=dt(f16))
        rsB = ops.finalize_rscale(ss, H, eps)
        act, _ = ops.gemm_bf16_nt_fused(a, L["wgu_c"], epilogue=2, rscale=rsB, operands=fmt(f16))
        a, ss = ops.gemm_resid32(act, L["wdown_c"], x32, gamma=None if last else enc.layers[l + 1]["ln1"], want_a16=not last, want_ss=not last,
                                 operands=fmt(f16), a16_dtype=dt(f16q))
        if not last:
            rsA = ops.finalize_rscale(ss, H, eps)
    return ops.rmsnorm_f32(x32, enc.final_norm, eps)


@pytest.mark.parametrize("mode", MODES)
def test_encoder_hidden_states_equal_the_chain_of_exported_calls(mode):
    from lightretriever_amd import _lib
    enc = _encoder(mode)
    ids, cu = _batch()
    _lib.lib().lrx_device_saturation_count(1), _lib.lib().lrx_device_error_count(1)
    got = enc.encode_hidden(ids, cu, max(LENS))
    want = chain(enc, ids, cu)
    assert got.dtype == want.dtype == torch.bfloat16 and got.shape == want.shape == (sum(LENS), 256)
    assert torch.isfinite(got.float()).all() and float(got.float().abs().mean()) > 0.1
    diff = got.view(torch.int16) != want.view(torch.int16)
    assert not diff.any(), f"{mode}: {int(diff.sum())} / {diff.numel()} hidden-state elements differ from the chain of exported calls"
    assert _lib.lib().lrx_device_saturation_count(1) == 0 and _lib.lib().lrx_device_error_count(1) == 0
    # the weights the chain used are the formats the table names
    L = enc.layers[0]
    h, b = torch.float16, torch.bfloat16
    assert [L[k].dtype for k in ("wqkv_c", "wo_c", "wgu_c", "wdown_c")] == {"bf16": [b, b, b, b], "fp16": [h, h, h, h], "fp16_qkv": [h, b, b, b]}[mode]


def test_the_three_modes_are_three_different_functions():
    """... so that the equality above can tell a mode from its neighbour: the same weights (seed) and batch give different bits per mode"""
    ids, cu = _batch()
    out = {m: _encoder(m).encode_hidden(ids, cu, max(LENS)) for m in MODES}
    for a in MODES:
        for b in MODES:
            if a < b:
                assert (out[a] != out[b]).float().mean() > 0.05, (a, b)
