"""Fused decode over an MXFP8 KV cache on MI355X: the append form of the decode-attention kernel bit for bit against
kv_cache_write followed by decode_attention (outputs and all four cache tensors), the QKV launches without caches,
and a Llama with kv_cache_dtype="mxfp8" on the fused launches (graphs vs eager, bf16 GPU vs the fp32 CPU model on the
same cache bytes, the appended row against the bf16-cache model's)."""

import math

import pytest
import torch

import neuronx_distributed_llama3_2_amd.ops as ops
from test_kv_cache_mxfp8_gpu import _llama_cfg
from test_mxfp4_gpu import _random_mx

pytestmark = pytest.mark.gpu

DEV = "cuda"
LMAX = 256   # two splits of 128 keys, chunks of 64


def _both(D, Hq, Hkv, T, seq, pos0, window, idx=None):
    """The append form and the composition on clones of one random valid cache (one row more than the batch):
    asserts equal outputs and cache bytes, returns (output, caches after [kc, ks, vc, vs], q)."""
    B = len(seq)
    g = torch.Generator().manual_seed(D + 7 * T + seq[0])
    caches = [t.to(DEV) for _ in "kv" for t in ops.quantize_mxfp8(torch.randn(B + 1, Hkv, LMAX, D, generator=g))]
    qkv = torch.randn(B, T, Hq + 2 * Hkv, D, generator=g).to(torch.bfloat16).to(DEV)
    q, k, v = qkv[:, :, :Hq], qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:]
    dev32 = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)
    seq_t, pos_t, ci = dev32(seq), dev32(pos0), dev32(idx)
    a, b = [t.clone() for t in caches], [t.clone() for t in caches]
    ops.kv_cache_write(k, v, a[0], a[2], pos_t, ci, k_scale=a[1], v_scale=a[3])
    ref = ops.decode_attention(q, a[0], a[2], seq_t, ci, window=window, k_scale=a[1], v_scale=a[3])
    got = ops.decode_attention(q, b[0], b[2], seq_t, ci, window=window, k_scale=b[1], v_scale=b[3], k_new=k, v_new=v,
                               positions=pos_t)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max().item()
    for name, x, y in zip(("k codes", "k scale", "v codes", "v scale"), b, a):
        assert torch.equal(x, y), (name, (x != y).nonzero()[:4].tolist())
    assert not torch.equal(a[0], caches[0])   # the write wrote
    return got, a, q


def _fp64(q, caches, seq, window):
    """fp64 softmax attention of q [B, T, Hq, D] over the dequantized cache rows 0..B-1."""
    kd, vd = (ops.dequantize_mxfp8(caches[i].cpu(), caches[i + 1].cpu(), torch.float32).double() for i in (0, 2))
    B, T, Hq, D = q.shape
    out = torch.zeros(B, T, Hq, D, dtype=torch.float64)
    for b in range(B):
        kk, vv = (x[b, :, :seq[b]].repeat_interleave(Hq // kd.shape[1], 0) for x in (kd, vd))   # [Hq, L, D]
        s = torch.matmul(q[b].cpu().double().permute(1, 0, 2), kk.transpose(1, 2)) / math.sqrt(D)
        lim = seq[b] - (T - 1 - torch.arange(T))[:, None]
        ki = torch.arange(seq[b])[None, :]
        s = s.masked_fill((ki >= lim) | ((ki < lim - window) if window else False), float("-inf"))
        out[b] = torch.matmul(torch.softmax(s, -1), vv).permute(1, 0, 2)
    return out


@pytest.mark.parametrize("seq", ["T", 65, 130, 256])   # T: an empty cache before; 130 at T = 4: rows 126..129 straddle
@pytest.mark.parametrize("window", [None, 16])          # a chunk and a split boundary
@pytest.mark.parametrize("Hq,Hkv,T", [(8, 2, 1), (8, 2, 4), (4, 4, 3)])
@pytest.mark.parametrize("D", [64, 128])
def test_append_equals_write_then_attend(D, Hq, Hkv, T, window, seq):
    seq = T if seq == "T" else seq
    got, caches, q = _both(D, Hq, Hkv, T, [seq], [seq - T], window)
    if (Hq, Hkv, T, seq) == (8, 2, 4, 130):
        # per element against fp64, the bound of test_decode_attention_kv8_equals_bf16_on_dequantized
        ref = _fp64(q, caches, [seq], window)
        rel = ((got.cpu().double() - ref).abs().max() / ref.abs().max()).item()
        print(f"D {D} window {window}: append form vs fp64 over the dequantized cache: {rel:.3e}")
        assert rel < 2e-2, rel


@pytest.mark.parametrize("case", [
    dict(Hq=8, Hkv=2, T=4, seq=[130, 70], pos0=[126, 66], idx=[2, 0]),   # permuted cache rows, two lengths
    dict(Hq=8, Hkv=2, T=4, seq=[256], pos0=[254]),                       # rows 256, 257 are past the cache: dropped
    dict(Hq=8, Hkv=2, T=4, seq=[200], pos0=[100]),                       # new rows in the middle of the visible keys
    dict(Hq=8, Hkv=2, T=9, seq=[130], pos0=[121]),                       # M = 36 > 16: the write launch, then the call
], ids=["cache_idx", "dropped", "middle", "M36"])
@pytest.mark.parametrize("window", [None, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_append_other_layouts(D, window, case):
    _both(D, window=window, **case)


@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("mx", [False, True], ids=["bf16", "mxfp4"])
def test_qkv_launch_without_caches_writes_the_same_rows(mx, M):
    """dgemv(3) / dgemv_mx(3) with kc = vc = None: y as with caches, bit for bit; one cache without the other raises."""
    C = ops.ext()
    nq, nkv, D, K, P = 4, 2, 64, 512, 48
    N = (nq + 2 * nkv) * D
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(DEV)
    ang = 6.28 * torch.rand(P, D // 2, generator=g)
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    pos = torch.tensor([5, 40, 0, 31][:M], dtype=torch.int64, device=DEV)
    if mx:
        w, scale = (t.to(DEV) for t in _random_mx(N, K, 3, 121, 127))
    else:
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(DEV)

    def run(kc, vc):
        y = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        if mx:
            C.dgemv_mx(3, x, nw, 1e-5, w, scale, y, nq=nq, nkv=nkv, D=D, cos_t=cos, sin_t=sin, pos=pos, T=1, kc=kc, vc=vc)
        else:
            C.dgemv(3, x, nw, 1e-5, w, y, nq, nkv, D, cos, sin, pos, 1, kc, vc, None)
        return y

    kc, vc = (torch.zeros(M, nkv, P, D, dtype=torch.bfloat16, device=DEV) for _ in "kv")
    y = run(kc, vc)
    assert torch.equal(run(None, None), y) and y.any()
    for m in range(M):   # the cached launch did write: the k and v columns of y
        assert torch.equal(kc[m, :, int(pos[m])].reshape(-1), y[m, nq * D:(nq + nkv) * D])
        assert torch.equal(vc[m, :, int(pos[m])].reshape(-1), y[m, (nq + nkv) * D:])
    with pytest.raises(RuntimeError):
        run(kc, None)


def _model(cfg, sd, dtype, device, graphs, steps, **kw):
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    icfg = InferenceConfig(batch_size=2, seq_len=256, max_context_length=128, use_hip_graphs=graphs,
                           decode_graph_steps=steps, deterministic=True, **kw)
    m = LlamaForCausalLMInference(cfg, icfg, dtype=dtype, device=device, init_weights=False)
    m._load_full(hf_to_nxd(sd, cfg))
    return m


@pytest.mark.parametrize("weights", ["bf16", "mxfp4", "mxfp4_qkv"])
def test_mxfp8_cache_model_decodes_on_fused_launches(weights, monkeypatch):
    """2-layer Llama, hidden 512, 8/2 heads, kv_cache_dtype="mxfp8", knob 1: the new gate is open and the existing one
    shut, hipGraph generation gives the eager tokens, one decode step matches the fp32 CPU model holding the same cache
    bytes within the 3e-2 of test_mxfp8_generation_graphs_match_eager_and_fp32_cpu; bf16 weights: layer 0's appended
    row is quantize_mxfp8 of the row the bf16-cache fused model writes; knob 0: the unfused step, bit for bit."""
    from transformers import LlamaForCausalLM as HF

    monkeypatch.setenv("NXD_DECODE_FUSED_KV8", "1")
    monkeypatch.setenv("NXD_DECODE_FUSED_MX", "1")
    cfg = _llama_cfg(512, None)
    torch.manual_seed(0)
    sd = {k: v.detach().to(torch.bfloat16).float() for k, v in HF(cfg).state_dict().items()}   # one set of values for all
    kw = {} if weights == "bf16" else dict(quantized=True, quantization_type="mxfp4", quantize_qkv=weights == "mxfp4_qkv")
    dev = torch.device(DEV)
    g = _model(cfg, sd, torch.bfloat16, dev, True, 8, kv_cache_dtype="mxfp8", **kw)
    e = _model(cfg, sd, torch.bfloat16, dev, False, 1, kv_cache_dtype="mxfp8", **kw)
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (2, 40))
    a = g.generate(ids, max_new_tokens=16, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=16, eos_token_id=-1).cpu()
    assert a.shape == (2, 56) and torch.equal(a, b), (a[:, 40:], b[:, 40:])
    n = b.shape[1]
    last, pos = b[:, -1:], torch.full((2, 1), n - 1, dtype=torch.int64)
    sid, clen = torch.arange(2), torch.full((2,), n, dtype=torch.int32)
    step = lambda m, d: m.model.forward_tokens(last.to(d), pos.to(d), sid.to(d), clen.to(d))
    for m in (g, e):
        assert m.model._decode_fusable_kv8(last.to(dev)) == ("bf16" if weights == "bf16" else "mx")
        assert m.model._check_decode_fusable() is False and not m.model._decode_fusable_mx(last.to(dev))
    assert e.model.kv_cache.dtype == torch.uint8 and e.model.kv_cache_scale[:, :, :, :, :n - 1].all()

    cpu = _model(cfg, sd, torch.float32, torch.device("cpu"), False, 1, kv_cache_dtype="mxfp8", **kw)
    cpu.model.kv_cache.copy_(e.model.kv_cache.cpu())
    cpu.model.kv_cache_scale.copy_(e.model.kv_cache_scale.cpu())
    lg, lc = step(e, dev).float().cpu(), step(cpu, "cpu").float()
    err = ((lg - lc).abs().max() / lc.abs().max()).item()
    print(f"{weights}: fused bf16 gpu vs fp32 cpu on the same MXFP8 cache, one decode step: {err:.3e}")
    assert err < 3e-2, err

    if weights == "bf16":   # layer 0 sees the same inputs whatever the cache holds
        f = _model(cfg, sd, torch.bfloat16, dev, False, 1)
        f.generate(ids, max_new_tokens=1, eos_token_id=-1)
        assert f.model._decode_fusable(last.to(dev))
        step(f, dev)
        codes, scale = ops.quantize_mxfp8(f.model.kv_cache[0, :, :, :, n - 1])
        assert torch.equal(e.model.kv_cache[0, :, :, :, n - 1], codes) and codes.any()
        assert torch.equal(e.model.kv_cache_scale[0, :, :, :, n - 1], scale)

    monkeypatch.setenv("NXD_DECODE_FUSED_KV8", "0")
    e.model._decode_fused_kv8_ok = None
    d0 = step(e, dev)
    assert e.model._decode_fused_kv8_ok == ""
    e.set_fused_decode(False)
    assert torch.equal(d0, step(e, dev))
