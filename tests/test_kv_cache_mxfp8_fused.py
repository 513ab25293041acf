"""CPU side of the fused decode over an MXFP8 KV cache: the append keywords of ops.decode_attention are the
write followed by the attention, their TypeErrors, and the gate that routes an MXFP8-cache Llama."""

import types

import pytest
import torch

import neuronx_distributed_llama3_2_amd.ops as ops
from test_inference import _hf_model, _tiny_cfg


def _operands(T=3, B=2, Hq=4, Hkv=2, D=64, L=40):
    g = torch.Generator().manual_seed(T)
    caches = [t for _ in "kv" for t in ops.quantize_mxfp8(torch.randn(B + 1, Hkv, L, D, generator=g))]   # kc, ks, vc, vs
    qkv = torch.randn(B, T, Hq + 2 * Hkv, D, generator=g).to(torch.bfloat16)
    return caches, qkv[:, :, :Hq], qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:]


@pytest.mark.parametrize("window", [None, 5])
def test_append_keywords_equal_write_then_attend(window):
    caches, q, k, v = _operands()
    seq = torch.tensor([17, 40], dtype=torch.int32)
    pos = torch.tensor([14, 38], dtype=torch.int32)    # the second sequence's last row is past the cache: dropped
    idx = torch.tensor([2, 0], dtype=torch.int32)
    a, b = [t.clone() for t in caches], [t.clone() for t in caches]
    ops.kv_cache_write(k, v, a[0], a[2], pos, idx, k_scale=a[1], v_scale=a[3])
    ref = ops.decode_attention(q, a[0], a[2], seq, idx, window=window, k_scale=a[1], v_scale=a[3])
    got = ops.decode_attention(q, b[0], b[2], seq, idx, window=window, k_scale=b[1], v_scale=b[3], k_new=k, v_new=v,
                               positions=pos)
    assert torch.equal(got, ref) and not torch.equal(a[0], caches[0])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_append_keywords_type_errors():
    (kc, ks, vc, vs), q, k, v = _operands()
    seq, pos = torch.tensor([17, 40], dtype=torch.int32), torch.tensor([14, 37], dtype=torch.int32)
    for kw in (dict(k_new=k), dict(k_new=k, v_new=v), dict(positions=pos), dict(v_new=v, positions=pos)):
        with pytest.raises(TypeError):
            ops.decode_attention(q, kc, vc, seq, k_scale=ks, v_scale=vs, **kw)
    bf = ops.dequantize_mxfp8(kc, ks)
    with pytest.raises(TypeError):   # a bf16 cache has no append form
        ops.decode_attention(q, bf, bf, seq, k_new=k, v_new=v, positions=pos)


def test_fused_kv8_gate(monkeypatch):
    """Open for an MXFP8-cache Llama with head dim 64 whose weights one of the fused routes takes, while the existing
    gates stay shut; shut by the knobs, a bf16 cache, head dim 32, a query group past 16 rows, CPU ids."""
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    def gate(heads=2, **kw):
        cfg = _tiny_cfg(num_attention_heads=heads, num_key_value_heads=1)
        sd = {k: v.detach().to(torch.bfloat16) for k, v in _hf_model(cfg, seed=4).state_dict().items()}
        icfg = InferenceConfig(batch_size=2, seq_len=64, max_context_length=32, **kw)
        m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, init_weights=False)
        m._load_full(hf_to_nxd(sd, cfg))
        return m.model

    def rows(B, T=1):   # stands in for GPU input ids: the gate reads only these
        return types.SimpleNamespace(is_cuda=True, numel=lambda: B * T, shape=(B, T))

    mx = dict(quantized=True, quantization_type="mxfp4")
    monkeypatch.setenv("NXD_DECODE_FUSED_KV8", "1")
    monkeypatch.setenv("NXD_DECODE_FUSED_MX", "1")
    m = gate(kv_cache_dtype="mxfp8")
    assert m._check_decode_fusable_kv8() == "bf16" and m._check_decode_fusable() is False
    assert m._decode_fusable_kv8(rows(2)) == "bf16" and m._decode_fusable(rows(2)) is False
    assert m._decode_fusable_kv8(rows(9)) == "" and m._decode_fusable_kv8(rows(1, 9)) == ""   # 9 rows; G * T = 18
    assert m._decode_fusable_kv8(torch.zeros(1, 1, dtype=torch.int64)) == ""                   # CPU ids
    q = gate(kv_cache_dtype="mxfp8", **mx)
    assert q._check_decode_fusable_kv8() == "mx" and q._check_decode_fusable_mx() is False
    assert q._decode_fusable_kv8(rows(3)) == "mx" and q._decode_fusable_mx(rows(3)) is False
    for knob in ("NXD_DECODE_FUSED_KV8", "NXD_DECODE_FUSED"):
        monkeypatch.setenv(knob, "0")
        assert m._check_decode_fusable_kv8() == "" and q._check_decode_fusable_kv8() == ""
        monkeypatch.setenv(knob, "1")
    m.setup_kv_cache(2, 32)   # a new cache re-reads the knob
    assert m._decode_fused_kv8_ok is None
    assert gate()._check_decode_fusable_kv8() == ""                                  # bf16 cache: the existing gates'
    assert gate(heads=4, kv_cache_dtype="mxfp8")._check_decode_fusable_kv8() == ""   # head dim 32
