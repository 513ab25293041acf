"""MXFP8 KV cache on MI355X: the quantizing cache write and mx8_dequant bit for bit against the torch
definition of the format (ops/decode.py), the KV8 decode-attention kernels against the bf16 kernels on
the dequantized cache, and a Llama with kv_cache_dtype="mxfp8" end to end (graphs vs eager, bf16 GPU
vs the fp32 CPU model on the same cache bytes)."""

import pytest
import torch

import neuronx_distributed_llama3_2_amd.ops as ops
from neuronx_distributed_llama3_2_amd.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
L = 2304                          # cache length: more than one 1,024-key split
POISON_CODE, POISON_E = 0x7E, 140  # 448 * 2^13, about 3.7e6: finite (0 x V stays 0), one unmasked read owns the softmax


def _write_inputs(B, T, Hkv, D, seed):
    """K / V as strided slices of a [B, T, Hq + 2 Hkv, D] QKV buffer: magnitudes over 20 binades, a zero
    block, blocks with amax 500 * 2^k (saturating), exact nearest-even ties and E4M3 subnormals."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, T, 4 + 2 * Hkv, D)
    m = 1.0 + torch.rand(shape, generator=g)
    e = torch.randint(-14, 6, shape, generator=g).float()
    s = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    qkv = s * m * torch.exp2(e)
    k, v = qkv[:, :, 4:4 + Hkv], qkv[:, :, 4 + Hkv:]
    k[0, 0, 0, :32] = 0.0
    v[1, 0, 1, 32:64] = 0.0
    for i, kk in enumerate((-9, 0, 7)):
        k[i % B, 0, 1, :32] = torch.randn(32, generator=g) * 2.0 ** kk
        k[i % B, 0, 1, 3 + i] = 500.0 * 2.0 ** kk
        v[i % B, T - 1, 0, 7] = -500.0 * 2.0 ** kk
    ties = torch.tensor([256.0, 17.0, 18.0, 19.0, 21.0, -23.0, 1.0625, 1.1875, -1.0625, 17.5, 16.5, 2.0 ** -9,
                         2.0 ** -10, 3 * 2.0 ** -10, -5 * 2.0 ** -10, 2.0 ** -11, 7 * 2.0 ** -9 + 2.0 ** -10,
                         2.0 ** -6 - 2.0 ** -10, 0.0, -0.0, 448.0, 464.0, -480.0, 449.0, 36.0, 44.0, 52.0, 60.0,
                         0.4375, 0.40625, 0.46875, 3.25])
    v[2, 0, 0, :32] = ties * 2.0 ** -5
    k[1, T - 1, 1, D - 32:] = ties * 2.0 ** 3
    return qkv.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 5])
def test_kv_cache_write_native_equals_quantizer(D, T):
    assert _ext.ext_available(), "HIP extension must be built for GPU tests"
    B, Hkv, Lmax = 3, 2, 256
    qkv, _, _ = _write_inputs(B, T, Hkv, D, seed=D + T)
    k, v = qkv[:, :, 4:4 + Hkv], qkv[:, :, 4 + Hkv:]
    assert not k.is_contiguous()
    pos = torch.tensor([0, 100, Lmax - 2], dtype=torch.int32)      # the last passes Lmax when T = 5
    idx = torch.tensor([2, 0, 3], dtype=torch.int32)
    fill = lambda *s: torch.full(s, 0xAB, dtype=torch.uint8, device=DEV)
    kc, vc = fill(4, Hkv, Lmax, D), fill(4, Hkv, Lmax, D)
    ks, vs = fill(4, Hkv, Lmax, D // 32), fill(4, Hkv, Lmax, D // 32)
    qkv_d = qkv.to(DEV)
    ops.kv_cache_write(qkv_d[:, :, 4:4 + Hkv], qkv_d[:, :, 4 + Hkv:], kc, vc, pos.to(DEV), idx.to(DEV), k_scale=ks, v_scale=vs)
    # the CPU path of the same op is the torch quantizer (tests/test_kv_cache_mxfp8.py)
    fc = lambda *s: torch.full(s, 0xAB, dtype=torch.uint8)
    rkc, rvc, rks, rvs = fc(4, Hkv, Lmax, D), fc(4, Hkv, Lmax, D), fc(4, Hkv, Lmax, D // 32), fc(4, Hkv, Lmax, D // 32)
    ops.kv_cache_write(k, v, rkc, rvc, pos, idx, k_scale=rks, v_scale=rvs)
    codes, e = ops.quantize_mxfp8(k)
    assert torch.equal(rkc[2, :, 0:T], codes[0].transpose(0, 1)) and int(e.min()) >= 1 and (rkc != 0xAB).any()
    for name, got, ref in (("k codes", kc, rkc), ("v codes", vc, rvc), ("k scale", ks, rks), ("v scale", vs, rvs)):
        bad = (got.cpu() != ref).nonzero()
        assert bad.numel() == 0, (name, bad[:8].tolist(), got.cpu()[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
    # row 1 of the cache is nobody's: untouched, like every slot outside the written rows (equal to the reference's fill)
    assert bool((kc[1] == 0xAB).all()) and bool((vs[1] == 0xAB).all())


def test_mx8_dequant_native_equals_torch():
    native = _ext.ext()
    g = torch.Generator().manual_seed(0)
    # every code under a spread of scales (NaN codes excluded: the quantizer never emits them)
    codes = torch.arange(256, dtype=torch.uint8).repeat(48).reshape(2, 3, 16, 128)
    codes[(codes & 0x7F) == 0x7F] = 0x7E
    scale = torch.randint(67, 200, (2, 3, 16, 4), generator=g).to(torch.uint8)
    ref = ops.dequantize_mxfp8(codes, scale)
    got = native.mx8_dequant(codes.to(DEV), scale.to(DEV))
    assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), ref)
    # strided (a slice along the key axis) and misaligned (byte offset 1) operands
    got = native.mx8_dequant(codes.to(DEV)[:, :, 3:11], scale.to(DEV)[:, :, 3:11])
    assert torch.equal(got.cpu(), ref[:, :, 3:11])
    buf = torch.zeros(codes.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = codes.to(DEV).reshape(-1)
    got = native.mx8_dequant(buf[1:].view(codes.shape), scale.to(DEV))
    assert torch.equal(got.cpu(), ref)


def _quant_caches(B, Hkv, D, T, seq, window, seed):
    """Quantized random caches with every slot outside each row's visible span [first key of the oldest
    new token, seq_len) overwritten by the poison code and scale."""
    g = torch.Generator().manual_seed(seed)
    kc, ks = ops.quantize_mxfp8(torch.randn(B, Hkv, L, D, generator=g))
    vc, vs = ops.quantize_mxfp8(torch.randn(B, Hkv, L, D, generator=g))
    pos = torch.arange(L)
    for b, s in enumerate(seq):
        lo = max(0, s - (T - 1) - window) if window and window < L else 0
        out = (pos < lo) | (pos >= s)
        for c, sc in ((kc, ks), (vc, vs)):
            c[b, :, out] = POISON_CODE
            sc[b, :, out] = POISON_E
    return kc, ks, vc, vs


@pytest.mark.parametrize("window", [0, 200])
@pytest.mark.parametrize("Hq,Hkv,T", [(8, 2, 1), (8, 2, 4), (8, 1, 3)])   # M = 4, 16 (KV8 kernel), 24 (dequantize fallback)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_kv8_equals_bf16_on_dequantized(D, Hq, Hkv, T, window):
    """torch.equal to the native bf16 kernels on the dequantized cache: the conversion is exact and
    nothing after the loads changes (two-launch path, no atomics).  The poison (finite, 3.7e6) fills
    every slot no row may read; the fp32 CPU reference over the quantized cache saw none of it."""
    assert _ext.ext_available(), "HIP extension must be built for GPU tests"
    B = 4
    seq = [L, T, 1229, 777]
    kc, ks, vc, vs = _quant_caches(B, Hkv, D, T, seq, window, seed=D + T + window)
    torch.manual_seed(2)
    q = (torch.randn(B, T, Hq, D) * 2).to(torch.bfloat16)
    seq_t = torch.tensor(seq, dtype=torch.int32)
    ref = ops.decode_attention(q, kc, vc, seq_t, window=window, k_scale=ks, v_scale=vs)      # CPU fallback
    assert torch.isfinite(ref).all() and ref.abs().max() < 100, "the reference saw the poison"
    d = lambda t: t.to(DEV)
    kd, vd = ops.dequantize_mxfp8(kc, ks), ops.dequantize_mxfp8(vc, vs)
    perm = torch.tensor([2, 0, 3, 1], dtype=torch.int32)      # sequence b lives in cache row perm[b]
    inv = torch.argsort(perm)
    for idx in (None, perm):
        rows = (lambda t: d(t)) if idx is None else (lambda t: d(t[inv.long()]))
        ci = None if idx is None else d(idx)
        got = ops.decode_attention(d(q), rows(kc), rows(vc), d(seq_t), ci, window=window, k_scale=rows(ks), v_scale=rows(vs))
        bf = ops.decode_attention(d(q), rows(kd), rows(vd), d(seq_t), ci, window=window)
        assert torch.isfinite(got).all()
        assert torch.equal(got, bf), (idx is None, (got.float() - bf.float()).abs().max().item())
        rel = ((got.cpu().float() - ref.float()).abs().max() / ref.float().abs().max()).item()
        assert rel < 2e-2, rel
    if (Hq, Hkv, T) == (8, 2, 4):
        # misaligned codes (byte offset 1) and non-contiguous caches (a longer allocation's first L keys)
        # take the dequantize fallback and still match
        bf = ops.decode_attention(d(q), d(kd), d(vd), d(seq_t), window=window)
        buf = torch.zeros(kc.numel() + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = d(kc).reshape(-1)
        got = ops.decode_attention(d(q), buf[1:].view(kc.shape), d(vc), d(seq_t), window=window, k_scale=d(ks), v_scale=d(vs))
        assert torch.equal(got, bf)
        big = lambda t: torch.cat([d(t), torch.zeros_like(d(t)[:, :, :64])], 2)[:, :, :L]
        assert not big(kc).is_contiguous()
        got = ops.decode_attention(d(q), big(kc), big(vc), d(seq_t), window=window, k_scale=big(ks), v_scale=big(vs))
        assert torch.equal(got, bf)


def _llama_cfg(hidden, window, max_pos=1024):
    from transformers import LlamaConfig

    cfg = LlamaConfig(hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=2, vocab_size=1000, max_position_embeddings=max_pos, rms_norm_eps=1e-5,
                      rope_theta=500000.0, tie_word_embeddings=True, eos_token_id=2)
    cfg.sliding_window = window
    return cfg


def _model(cfg, sd, dtype, device, graphs=True, steps=8, **kw):
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    icfg = InferenceConfig(batch_size=2, seq_len=256, max_context_length=128, use_hip_graphs=graphs,
                           decode_graph_steps=steps, kv_cache_dtype="mxfp8", **kw)
    m = LlamaForCausalLMInference(cfg, icfg, dtype=dtype, device=device, init_weights=False)
    m._load_full(hf_to_nxd(sd, cfg))
    return m


@pytest.mark.parametrize("window", [None, 16])
def test_mxfp8_generation_graphs_match_eager_and_fp32_cpu(window):
    """2-layer Llama, hidden 512, kv_cache_dtype="mxfp8", deterministic=True: graphed prefill + hipGraph
    decode give the eager tokens, and one bf16 decode step on the GPU matches the fp32 CPU model holding
    the same cache bytes within the bf16-vs-fp32 bound of test_inference_gpu.py (3e-2 of the largest
    logit)."""
    from transformers import LlamaForCausalLM as HF

    cfg = _llama_cfg(512, window)
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in HF(cfg).state_dict().items()}
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (2, 40))
    dev = torch.device(DEV)
    g = _model(cfg, sd, torch.bfloat16, dev, graphs=True, steps=8, deterministic=True, prefill_graphs=True)
    e = _model(cfg, sd, torch.bfloat16, dev, graphs=False, steps=1, deterministic=True, prefill_graphs=False)
    assert e.model.kv_cache.dtype == torch.uint8 and e.model.kv_cache_scale is not None
    assert not e.model._decode_fusable(ids[:, :1].to(dev))
    a = g.generate(ids, max_new_tokens=24, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=24, eos_token_id=-1).cpu()
    assert a.shape == (2, 64)
    assert g._prefill_cache, "the prefill graph was not used"
    assert torch.equal(a, b), (a, b)
    assert e.model.kv_cache[:, :, :, :, :60].any() and e.model.kv_cache_scale[:, :, :, :, :60].all()
    cpu = _model(cfg, sd, torch.float32, torch.device("cpu"), graphs=False, steps=1)
    cpu.model.kv_cache.copy_(e.model.kv_cache.cpu())
    cpu.model.kv_cache_scale.copy_(e.model.kv_cache_scale.cpu())
    n = b.shape[1]
    last = b[:, -1:]
    pos = torch.full((2, 1), n - 1, dtype=torch.int64)
    sid = torch.arange(2)
    clen = torch.full((2,), n, dtype=torch.int32)
    lg = e.model.forward_tokens(last.to(dev), pos.to(dev), sid.to(dev), clen.to(dev)).float().cpu()
    lc = cpu.model.forward_tokens(last, pos, sid, clen).float()
    err = ((lg - lc).abs().max() / lc.abs().max()).item()
    print(f"window {window}: bf16 gpu vs fp32 cpu on the same MXFP8 cache, one decode step: {err:.3e}")
    assert err < 3e-2, err
