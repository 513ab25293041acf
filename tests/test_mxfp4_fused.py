"""CPU side of the fused MXFP4 decode launches: the composed fallback of ops.gemv.mx_decode_linear against the fp64
definition of its three forms, and the gate that routes a quantized Llama to them."""

import types

import pytest
import torch

from test_inference import _hf_model, _tiny_cfg
from test_mxfp4_gpu import _random_mx


@pytest.mark.parametrize("form", ["plain_norm", "resid", "glu_norm"])
def test_mx_decode_linear_fallback_matches_definition(form):
    from neuronx_distributed_llama3_2_amd.ops import gemv as ops

    K, N, M, eps = 96, 5, 3, 1e-5
    glu = form == "glu_norm"
    packed, scale = _random_mx(2 * N if glu else N, K, 3, 121, 127)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    y0 = torch.randn(M, N, generator=g).to(torch.bfloat16)
    wd = ops.dequantize_mxfp4(packed, scale, torch.float32).double()
    a = x.double()
    if form != "resid":
        a = (a * torch.rsqrt(a.pow(2).mean(-1, keepdim=True) + eps) * nw.double()).float().to(torch.bfloat16).double()
    acc = a @ wd.t()
    if form == "resid":
        res = y0.clone()
        out = ops.mx_decode_linear(x, packed, scale, residual=res)
        assert out is res
        ref = y0.double() + acc
    else:
        out = ops.mx_decode_linear(x, packed, scale, norm_weight=nw, eps=eps, glu=glu)
        ref = torch.nn.functional.silu(acc[:, :N]) * acc[:, N:] if glu else acc
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    torch.testing.assert_close(out.double(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)
    with pytest.raises(ValueError):
        ops.mx_decode_linear(x, packed, scale, glu=True, residual=y0)


def test_fused_mx_gate(monkeypatch):
    """Open for a bias-free MXFP4 Llama at up to three rows; shut by the knobs, a bias, an MXFP8 cache, a fourth row."""
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    cfg = _tiny_cfg()
    sd = {k: v.detach().to(torch.bfloat16) for k, v in _hf_model(cfg, seed=4).state_dict().items()}

    def gate(**kw):
        icfg = InferenceConfig(batch_size=2, seq_len=64, max_context_length=32, quantized=True, quantization_type="mxfp4", **kw)
        m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, init_weights=False)
        m._load_full(hf_to_nxd(sd, cfg))
        return m.model

    def rows(n):   # stands in for GPU input ids: the gate reads only these two
        return types.SimpleNamespace(is_cuda=True, numel=lambda: n)

    monkeypatch.setenv("NXD_DECODE_FUSED_MX", "1")
    m = gate()
    assert m._check_decode_fusable_mx() is True and m._check_decode_fusable() is False
    assert m._decode_fusable_mx(rows(3)) is True and m._decode_fusable_mx(rows(4)) is False
    assert m._decode_fusable_mx(torch.zeros(1, 1, dtype=torch.int64)) is False   # CPU ids
    for knob in ("NXD_DECODE_FUSED_MX", "NXD_DECODE_FUSED"):
        monkeypatch.setenv(knob, "0")
        assert m._check_decode_fusable_mx() is False
        monkeypatch.setenv(knob, "1")
    down = m.model.layers[1].mlp.down_proj
    down.bias = torch.nn.Parameter(torch.zeros(down.weight.shape[0], dtype=torch.bfloat16), requires_grad=False)
    assert m._check_decode_fusable_mx() is False
    assert gate(kv_cache_dtype="mxfp8")._check_decode_fusable_mx() is False
