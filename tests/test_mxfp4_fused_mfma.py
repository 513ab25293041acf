"""CPU side of the fused MXFP4 decode launches at 4-16 rows: the gate beside _decode_fusable_mx that routes a quantized
Llama to them, and ops.gemv.mx_decode_linear at 6 rows against the fp64 definition of its three forms."""

import types

import pytest
import torch

from test_inference import _hf_model, _tiny_cfg
from test_mxfp4_gpu import _random_mx


def test_fused_mx_rows_gate(monkeypatch):
    """Open at 4 and 8 rows under the knob at 16; shut at 9 rows, by the knob at 3, NXD_DECODE_FUSED_MX=0, an MXFP8
    cache, CPU ids and M * hidden > 32768 (the fused norm of the bf16 QKV launch ends there); the 1-3 row gate stays
    shut at four rows."""
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    def gate(cfg=None, **kw):
        cfg = cfg or _tiny_cfg()
        sd = {k: v.detach().to(torch.bfloat16) for k, v in _hf_model(cfg, seed=4).state_dict().items()}
        icfg = InferenceConfig(batch_size=2, seq_len=64, max_context_length=32, quantized=True, quantization_type="mxfp4", **kw)
        m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, init_weights=False)
        m._load_full(hf_to_nxd(sd, cfg))
        return m.model

    def rows(n):   # stands in for GPU input ids: the gates read only these two
        return types.SimpleNamespace(is_cuda=True, numel=lambda: n)

    def fresh(m, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m._decode_fused_mx_ok = None
        return m

    m = fresh(gate(), NXD_DECODE_FUSED_MX="1", NXD_DECODE_FUSED_MX_ROWS="16")
    assert m._decode_fusable_mx_rows(rows(4)) is True and m._decode_fusable_mx_rows(rows(8)) is True
    assert m._decode_fusable_mx_rows(rows(9)) is False and m._decode_fusable_mx_rows(rows(3)) is False
    assert m._decode_fusable_mx(rows(4)) is False
    assert m._decode_fusable_mx_rows(torch.zeros(4, 1, dtype=torch.int64)) is False   # CPU ids
    assert fresh(m, NXD_DECODE_FUSED_MX_ROWS="3")._decode_fusable_mx_rows(rows(4)) is False
    assert fresh(m, NXD_DECODE_FUSED_MX_ROWS="16", NXD_DECODE_FUSED_MX="0")._decode_fusable_mx_rows(rows(4)) is False
    monkeypatch.setenv("NXD_DECODE_FUSED_MX", "1")
    assert gate(kv_cache_dtype="mxfp8")._decode_fusable_mx_rows(rows(4)) is False
    wide = gate(_tiny_cfg(hidden_size=5120, num_attention_heads=32, intermediate_size=64, num_hidden_layers=1, vocab_size=64))
    assert wide._decode_fusable_mx_rows(rows(6)) is True and wide._decode_fusable_mx_rows(rows(7)) is False   # 7 x 5120


@pytest.mark.parametrize("form", ["plain_norm", "resid", "glu_norm"])
def test_mx_decode_linear_at_6_rows_matches_definition(form):
    """test_mx_decode_linear_fallback_matches_definition's check and tolerance at 6 rows."""
    from neuronx_distributed_llama3_2_amd.ops import gemv as ops

    K, N, M, eps = 96, 5, 6, 1e-5
    glu = form == "glu_norm"
    packed, scale = _random_mx(2 * N if glu else N, K, 3, 121, 127)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    y0 = torch.randn(M, N, generator=g).to(torch.bfloat16)
    a = x.double()
    if form != "resid":
        a = (a * torch.rsqrt(a.pow(2).mean(-1, keepdim=True) + eps) * nw.double()).float().to(torch.bfloat16).double()
    acc = a @ ops.dequantize_mxfp4(packed, scale, torch.float32).double().t()
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
