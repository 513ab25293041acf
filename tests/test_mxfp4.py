"""MXFP4 weight-only quantization on CPU: the quantizer's OCP MX v1.0 properties (exponent, nearest /
ties-to-even / saturation, idempotence), nibble packing, error handling, tensor-parallel sharding,
the MXFP4 linears' state-dict handling, and the quantized tiny Llama end to end (format:
neuronx_distributed_llama3_2_amd/ops/gemv.py)."""

import math
import os
import sys
import tempfile

import pytest
import torch

from test_inference import _hf_model, _inf_model, _tiny_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _ops():
    from neuronx_distributed_llama3_2_amd.ops import gemv

    return gemv


def _codes(packed):
    """packed uint8 [..., K/2] -> codes uint8 [..., K] (element 2j = low nibble of byte j)."""
    return torch.stack((packed & 0xF, packed >> 4), dim=-1).reshape(packed.shape[:-1] + (packed.shape[-1] * 2,))


def _spread(shape, seed):
    """Random floats with magnitudes spread over 2^-20 .. 2^4."""
    g = torch.Generator().manual_seed(seed)
    m = 1.0 + torch.rand(shape, generator=g)
    e = torch.randint(-20, 4, shape, generator=g).float()
    s = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return s * m * torch.exp2(e)


def _weights():
    a = _spread((7, 96), 0)
    a[0, :32] = 0.0                                   # an all-zero block
    a[1, 32:64] = 0.0
    a[1, 40] = -0.37                                  # a block holding a single non-zero
    a[2, 64:96] = 1.5                                 # a block of equal maxima
    a[2, 64:96:3] = -1.5
    # every tie of the grid, values above 6 * 2^X (X = 0 here: amax = 7.5), and both signs
    a[3, :32] = torch.tensor([7.5, -7.0, 6.5, 5.0, -5.0, 3.5, -3.5, 2.5, -2.5, 1.75, -1.75, 1.25, -1.25, 0.75, -0.75,
                              0.25, -0.25, 0.24, 0.26, 4.0, 6.0, 3.0, 2.0, 1.0, 0.5, 0.0, 5.01, 4.99, 1.76, 1.74, 0.1,
                              -0.0])
    b = _spread((3, 4096), 1)
    b[1, 1024:1056] = 0.0
    return [a, b]


@pytest.mark.parametrize("idx", [0, 1])
def test_quantizer_exponent_and_nearest(idx):
    ops = _ops()
    w = _weights()[idx]
    packed, scale = ops.quantize_mxfp4(w)
    out, K = w.shape
    assert packed.shape == (out, K // 2) and scale.shape == (out, K // 32)
    assert packed.dtype == torch.uint8 and scale.dtype == torch.uint8
    assert int(scale.min()) >= 1 and int(scale.max()) <= 254
    blocks = w.double().reshape(out, K // 32, 32)
    amax = blocks.abs().amax(-1)
    X = scale.double() - 127.0
    nz = amax > 0
    # exponent: 2^(X+2) <= amax < 2^(X+3)
    assert bool((torch.exp2(X + 2)[nz] <= amax[nz]).all()) and bool((amax[nz] < torch.exp2(X + 3)[nz]).all())
    codes = _codes(packed).reshape(out, K // 32, 32)
    # all-zero blocks: e = 127 and zero codes
    assert bool((scale[~nz] == 127).all()) and int(codes[~nz].sum()) == 0
    # nearest of the 15 grid values by brute force, ties to the even code, saturation at +-6
    a = blocks / torch.exp2(X).unsqueeze(-1)
    grid = torch.tensor(GRID, dtype=torch.float64)
    dist = (a.abs().unsqueeze(-1) - grid).abs()                 # [out, nb, 32, 8]
    best = dist.min(-1, keepdim=True).values
    cand = dist == best
    assert int(cand.sum(-1).max()) <= 2
    even = torch.tensor([i % 2 == 0 for i in range(8)])
    idx_all = torch.arange(8).expand_as(cand)
    want = torch.where(cand.sum(-1) == 1, (idx_all * cand).sum(-1), (idx_all * (cand & even)).sum(-1))
    got = (codes & 7).long()
    assert torch.equal(got, want), (got[got != want][:8], want[got != want][:8])
    # the sign bit is the input's sign (a magnitude rounded to zero keeps it)
    assert torch.equal((codes >> 3).bool(), torch.signbit(blocks))
    # values above 6 * 2^X saturate
    sat = a.abs() > 6
    assert bool(((codes & 7)[sat] == 7).all())
    if idx == 0:
        assert int(sat.sum()) >= 3 and int((cand.sum(-1) == 2).sum()) >= 14   # the hand-made ties are there


def test_quantizer_idempotent_on_its_own_output():
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    out, nb = 9, 12
    codes = torch.randint(0, 16, (out, nb, 32), generator=g, dtype=torch.uint8)
    # every block holds a magnitude of 4 or 6, so its amax pins the block exponent
    pos = torch.randint(0, 32, (out, nb, 1), generator=g)
    top = torch.randint(6, 8, (out, nb, 1), generator=g, dtype=torch.uint8) | \
        (torch.randint(0, 2, (out, nb, 1), generator=g, dtype=torch.uint8) << 3)
    codes.scatter_(2, pos, top)
    codes = codes.reshape(out, nb * 16, 2)
    packed = codes[..., 0] | (codes[..., 1] << 4)
    scale = torch.randint(97, 138, (out, nb), generator=g, dtype=torch.uint8)
    for dtype in (torch.float32, torch.bfloat16):
        w = ops.dequantize_mxfp4(packed, scale, dtype)
        p2, s2 = ops.quantize_mxfp4(w)
        assert torch.equal(p2, packed) and torch.equal(s2, scale)
    # bf16 dequantisation is exact
    assert torch.equal(ops.dequantize_mxfp4(packed, scale, torch.bfloat16).float(),
                       ops.dequantize_mxfp4(packed, scale, torch.float32))


def test_packing_and_literal_block():
    ops = _ops()
    # byte j: element 2j in the low nibble, 2j + 1 in the high nibble; codes 0..15 twice
    packed = torch.tensor([[0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE] * 2], dtype=torch.uint8)
    scale = torch.tensor([[128]], dtype=torch.uint8)              # 2^1
    want = [0.0, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, -0.0, -1.0, -2.0, -3.0, -4.0, -6.0, -8.0, -12.0] * 2
    got = ops.dequantize_mxfp4(packed, scale, torch.float32)
    assert got.shape == (1, 32) and got[0].tolist() == want
    assert torch.equal(ops.dequantize_mxfp4(packed, scale), torch.tensor([want]).to(torch.bfloat16))
    w = torch.zeros(1, 32)
    w[0, 0], w[0, 1], w[0, 31] = 6.0, -0.5, 1.0
    p, s = ops.quantize_mxfp4(w)
    assert int(s[0, 0]) == 127 and int(p[0, 0]) == (0x9 << 4 | 0x7) and int(p[0, 15]) == 0x2 << 4
    assert int(p[0, 1:15].sum()) == 0
    # E8M0 edge bytes in the CPU dequantizer: 0 is 2^-127, 255 is NaN
    one = torch.tensor([[0x02] + [0] * 15], dtype=torch.uint8)    # element 0 = 1.0
    assert float(ops.dequantize_mxfp4(one, torch.tensor([[0]], dtype=torch.uint8), torch.float32)[0, 0]) == 2.0 ** -127
    assert bool(torch.isnan(ops.dequantize_mxfp4(one, torch.tensor([[255]], dtype=torch.uint8), torch.float32)).all())


def test_error_handling():
    ops = _ops()
    with pytest.raises(ValueError):
        ops.quantize_mxfp4(torch.randn(4, 48))
    w = torch.randn(4, 64)
    w[2, 5] = float("nan")
    with pytest.raises(ValueError):
        ops.quantize_mxfp4(w)
    w[2, 5] = float("inf")
    with pytest.raises(ValueError):
        ops.quantize_mxfp4(w)


def test_mx_linear_cpu_is_dequantize_plus_linear():
    ops = _ops()
    torch.manual_seed(3)
    w = torch.randn(24, 64)
    p, s = ops.quantize_mxfp4(w)
    wd = ops.dequantize_mxfp4(p, s, torch.float32)
    x, b = torch.randn(2, 3, 64), torch.randn(24)
    assert torch.equal(ops.mx_linear(x, p, s, b), torch.nn.functional.linear(x, wd, b))
    y = torch.nn.functional.linear(x, wd, b)
    torch.testing.assert_close(ops.mx_linear(x, p, s, b, glu=True), torch.nn.functional.silu(y[..., :12]) * y[..., 12:])


def test_quantize_commutes_with_tp_sharding():
    from neuronx_distributed_llama3_2_amd.parallel_layers.sharding import shard_tensor
    from neuronx_distributed_llama3_2_amd.quantization import MXFP4RowParallel

    ops = _ops()
    w = _spread((64, 256), 4)
    p, s = ops.quantize_mxfp4(w)
    for dim in (0, 1):   # column split (out), row split (in)
        attrs = {"tp": True, "dim": dim, "stride": 1, "qkv": None}
        for r in range(2):
            pl, sl = ops.quantize_mxfp4(shard_tensor(w, attrs, 2, r).contiguous())
            assert torch.equal(pl, shard_tensor(p, attrs, 2, r)) and torch.equal(sl, shard_tensor(s, attrs, 2, r))
    with pytest.raises(ValueError):
        MXFP4RowParallel(48, 16, bias=False)   # local in-features must be whole blocks


def test_mxfp4_layers_state_dict():
    from neuronx_distributed_llama3_2_amd.parallel_layers.layers import ColumnParallelLinear, RowParallelLinear
    from neuronx_distributed_llama3_2_amd.quantization import (MXFP4ColumnParallel, MXFP4RowParallel, QuantizationType,
                                                               QuantizedDtype, convert, get_default_mxfp4_qconfig_dict)

    from neuronx_distributed_llama3_2_amd.inference.generation import _init_single_process
    from neuronx_distributed_llama3_2_amd.parallel_layers import parallel_state as ps

    _init_single_process()
    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    ops = _ops()
    torch.manual_seed(5)
    qc = get_default_mxfp4_qconfig_dict()
    assert qc["quantized_dtype"] == QuantizedDtype.MXFP4 and qc["quantization_type"] == QuantizationType.MX_BLOCK
    assert QuantizationType("mxfp4") == QuantizationType.MX_BLOCK
    for fcls, qcls in ((ColumnParallelLinear, MXFP4ColumnParallel), (RowParallelLinear, MXFP4RowParallel)):
        f = fcls(64, 40, bias=True)
        with torch.no_grad():
            f.weight.normal_()
            f.bias.normal_()
        a = qcls.from_float(f, q_config=qc)
        assert a.weight.dtype == torch.uint8 and a.scale.dtype == torch.uint8
        assert a.weight.shape == (40, 32) and a.scale.shape == (40, 2)
        for t in (a.weight, a.scale):
            assert t.tensor_model_parallel and t.partition_dim == (0 if qcls is MXFP4ColumnParallel else 1)
        p, s = ops.quantize_mxfp4(f.weight)
        assert torch.equal(a.weight, p) and torch.equal(a.scale, s) and torch.equal(a.bias, f.bias)
        # a float weight in the state dict is quantized on load: the same packed bits
        b = qcls(64, 40, bias=True, dtype=torch.float32)
        b.load_state_dict({"weight": f.weight.detach().clone(), "bias": f.bias.detach().clone()})
        assert torch.equal(b.weight, a.weight) and torch.equal(b.scale, a.scale)
        # a packed state dict round-trips as it is
        c = qcls(64, 40, bias=True, dtype=torch.float32)
        c.load_state_dict(a.state_dict())
        assert torch.equal(c.weight, a.weight) and torch.equal(c.scale, a.scale) and torch.equal(c.bias, a.bias)
        x = torch.randn(3, 64)
        want = torch.nn.functional.linear(x, ops.dequantize_mxfp4(p, s, torch.float32)) + f.bias
        assert torch.equal(a(x), want) and torch.equal(c(x), want)
    # convert() picks the MXFP4 layers from the q_config alone
    m = convert(torch.nn.Sequential(ColumnParallelLinear(64, 32, bias=False)), qc)
    assert isinstance(m[0], MXFP4ColumnParallel)


def test_mxfp4_refuses_moe_experts():
    from neuronx_distributed_llama3_2_amd.quantization import get_default_mxfp4_qconfig_dict
    from neuronx_distributed_llama3_2_amd.quantization.quantization_mappings import get_mxfp4_quant_module_mappings
    from neuronx_distributed_llama3_2_amd.modules.moe import moe_parallel_layers as mp

    mapping = get_mxfp4_quant_module_mappings()
    for cls in (mp.ExpertFusedColumnParallelLinear, mp.ExpertFusedRowParallelLinear):
        with pytest.raises(NotImplementedError):
            mapping[cls].from_float(None, q_config=get_default_mxfp4_qconfig_dict())


def _fake_quantized_sd(hf_sd):
    """HF state dict whose decoder linears (and the tied table the lm_head copies) went through
    quantize -> dequantize; the fused QKV projection stays float, as in the quantized model."""
    ops = _ops()
    out = {}
    for k, v in hf_sd.items():
        if any(t in k for t in ("o_proj", "gate_proj", "up_proj", "down_proj")) and k.endswith("weight"):
            out[k] = ops.dequantize_mxfp4(*ops.quantize_mxfp4(v), v.dtype)
        else:
            out[k] = v.detach().clone()
    return out


def test_mxfp4_inference_end_to_end():
    from neuronx_distributed_llama3_2_amd.inference import LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.quantization import MXFP4ColumnParallel, MXFP4RowParallel

    ops = _ops()
    cfg = _tiny_cfg()
    hf = _hf_model(cfg, seed=4)
    sd = hf.state_dict()
    q = _inf_model(cfg, sd, quantized=True, quantization_type="mxfp4")
    layer = q.model.model.layers[0]
    assert isinstance(layer.mlp.down_proj, MXFP4RowParallel) and isinstance(q.model.lm_head, MXFP4ColumnParallel)
    assert layer.mlp.gate_up_proj.weight.dtype == torch.uint8 and layer.mlp.gate_up_proj.scale.dtype == torch.uint8
    # parameter bytes of the converted linears: out * in * (1/2 + 1/32)
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    for mod, o, i in ((layer.self_attn.o_proj, H, H), (layer.mlp.gate_up_proj, 2 * I, H), (layer.mlp.down_proj, H, I),
                      (q.model.lm_head, V, H)):
        nbytes = sum(p.numel() * p.element_size() for p in mod.parameters())
        assert nbytes * 32 == o * i * 17, (type(mod), nbytes)
    # float model with the same fake-quantized weights; its lm_head is the float tied table, so
    # fake-quantize that head (not the embedding lookup) by hand
    f = _inf_model(cfg, _fake_quantized_sd(sd))
    emb = f.model.model.embed_tokens.weight
    f.model.lm_head.weight = torch.nn.Parameter(ops.dequantize_mxfp4(*ops.quantize_mxfp4(emb), emb.dtype),
                                                requires_grad=False)
    torch.manual_seed(6)
    ids = torch.randint(3, cfg.vocab_size, (1, 10))
    lq, lf = q._context_encode(ids), f._context_encode(ids)
    assert torch.equal(lq, lf)
    tq = q.generate(ids, max_new_tokens=8, eos_token_id=-1)
    tf = f.generate(ids, max_new_tokens=8, eos_token_id=-1)
    assert tq.shape == (1, 18) and torch.equal(tq, tf)
    # trace -> load round trip keeps the packed shards
    d = tempfile.mkdtemp()
    q.compile(d)
    q2 = LlamaForCausalLMInference.load(d, dtype=torch.float32)
    o2 = q2.model.model.layers[1].self_attn.o_proj
    assert o2.weight.dtype == torch.uint8 and o2.scale.dtype == torch.uint8
    assert torch.equal(o2.weight, q.model.model.layers[1].self_attn.o_proj.weight)
    assert torch.equal(q2.model.lm_head.weight, q.model.lm_head.weight)
    assert torch.equal(q2._context_encode(ids), lq)

    # recorded, not gated: the quantization error against the unquantized float model
    m = _inf_model(cfg, sd)
    lm = m._context_encode(ids)
    rel = float((lq - lm).norm() / lm.norm())
    zero_sd = {k: (torch.zeros_like(v) if any(t in k for t in ("o_proj", "gate_proj", "up_proj", "down_proj")) else v)
               for k, v in sd.items()}
    lz = _inf_model(cfg, zero_sd)._context_encode(ids)
    rel_zero = float((lz - lm).norm() / lm.norm())
    print(f"mxfp4 tiny-llama logits: relative L2 vs float {rel:.4f}; zeroed linears {rel_zero:.4f}")
    assert math.isfinite(rel)
    assert rel < rel_zero   # a sanity floor, not a quality claim


def test_quantized_example_cli_mxfp4(tmp_path):
    """examples/inference/run_llama_quantized.py --quantization_type mxfp4: trace, reload, generate."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "inference"))
    import run_llama_quantized
    from safetensors.torch import load_file
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    llama = LlamaForCausalLM(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                         num_attention_heads=4, num_key_value_heads=2, vocab_size=128,
                                         max_position_embeddings=128))
    src = str(tmp_path / "llama")
    llama.save_pretrained(src)
    out = run_llama_quantized.main(["--model_path", src, "--traced_path", str(tmp_path / "q"), "--max_prompt_length",
                                    "16", "--sequence_length", "24", "--prompt_ids", "7,8,9",
                                    "--quantization_type", "mxfp4"])
    assert out.shape == (1, 24)
    shard = load_file(str(tmp_path / "q" / "tp0_sharded_checkpoint.safetensors"))
    w = shard["model.layers.0.mlp.down_proj.weight"]
    assert w.dtype == torch.uint8 and w.shape == (64, 64)
    assert shard["model.layers.0.mlp.down_proj.scale"].dtype == torch.uint8
