"""MXFP4 MoE experts on the CPU: the two expert ops against bmm on the dequantized stack, the
expert-fused MXFP4 layers (bits, state dicts, sharding), and the quantized Mixtral / DBRX
applications against float twins whose o_proj / lm_head / expert weights went through
quantize -> dequantize (the CPU path dequantizes, so the two agree up to fp32 summation order)."""

import os
import tempfile

import pytest
import torch

from dist_utils import run_distributed
from neuronx_distributed_llama3_2_amd.parallel_layers import parallel_state as ps
from test_inference_moe import _app, _dbrx_hf, _mixtral_cfg, _mixtral_hf


def _ops():
    from neuronx_distributed_llama3_2_amd.ops import gemv

    return gemv


def _stack(E, Nw, K, seed):
    torch.manual_seed(seed)
    ops = _ops()
    p, s = ops.quantize_mxfp4(torch.randn(E, Nw, K) * torch.exp2(torch.randint(-3, 4, (E, Nw, 1)).float()))
    return p, s, ops.dequantize_mxfp4(p, s, torch.float32)


def _single_process_tp1():
    from neuronx_distributed_llama3_2_amd.inference.generation import _init_single_process

    _init_single_process()
    ps.initialize_model_parallel(tensor_model_parallel_size=1)


# ---------------------------------------------------------------------------------------- ops
def test_dequantize_accepts_the_3d_stack():
    ops = _ops()
    p, s, wd = _stack(3, 6, 64, 0)
    assert wd.shape == (3, 6, 64)
    for e in range(3):
        assert torch.equal(wd[e], ops.dequantize_mxfp4(p[e], s[e], torch.float32))
    out = torch.empty(3, 6, 64)
    assert ops.dequantize_mxfp4_into(p, s, out) is out and torch.equal(out, wd)
    with pytest.raises(ValueError):
        ops.dequantize_mxfp4_into(p, s, torch.empty(3, 6, 32))


@pytest.mark.parametrize("eidx,xdiv", [([2], 1), ([0, 1, 2, 3], 1), ([3, 3, 0, 3], 2), ([1, 0, 1, 0, 2, 2], 3)])
def test_mx_expert_linear_is_bmm_on_the_dequantized_stack(eidx, xdiv):
    ops = _ops()
    E, N, K = 4, 10, 64
    p, s, wd = _stack(E, 2 * N, K, 1)
    P = len(eidx)
    torch.manual_seed(2)
    x = torch.randn((P + xdiv - 1) // xdiv, K)
    idx = torch.tensor(eidx, dtype=torch.int32)
    rows = x[torch.arange(P) // xdiv]
    want = torch.bmm(rows.unsqueeze(1), wd[idx.long()].transpose(1, 2)).squeeze(1)
    got = ops.mx_expert_linear(x, p, s, idx, xdiv=xdiv)
    assert got.shape == (P, 2 * N)
    torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-6)
    glu = ops.mx_expert_linear(x, p, s, idx.long(), xdiv=xdiv, glu=True)
    torch.testing.assert_close(glu, torch.nn.functional.silu(want[:, :N]) * want[:, N:], atol=1e-6, rtol=1e-6)


def test_mx_experts_linear_is_bmm_on_the_dequantized_stack():
    ops = _ops()
    E, N, K = 4, 6, 96
    p, s, wd = _stack(E, 2 * N, K, 3)
    torch.manual_seed(4)
    for M in (1, 3, 9):
        shared, per = torch.randn(M, K), torch.randn(E, M, K)
        want_s = torch.bmm(shared.expand(E, M, K), wd.transpose(1, 2))
        want_p = torch.bmm(per, wd.transpose(1, 2))
        torch.testing.assert_close(ops.mx_experts_linear(shared, p, s), want_s, atol=1e-6, rtol=1e-6)
        torch.testing.assert_close(ops.mx_experts_linear(per, p, s), want_p, atol=1e-6, rtol=1e-6)
        torch.testing.assert_close(ops.mx_experts_linear(per, p, s, glu=True),
                                   torch.nn.functional.silu(want_p[..., :N]) * want_p[..., N:], atol=1e-6, rtol=1e-6)


def test_expert_ops_shape_and_dtype_errors():
    ops = _ops()
    p, s, _ = _stack(4, 6, 64, 5)
    x, idx = torch.randn(2, 64), torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.mx_expert_linear(x, p.to(torch.int8), s, idx)
    with pytest.raises(TypeError):
        ops.mx_expert_linear(x, p, s, idx.float())
    with pytest.raises(TypeError):
        ops.mx_experts_linear(x, p, s.float())
    with pytest.raises(ValueError):
        ops.mx_expert_linear(x, p[0], s[0], idx)            # a 2-D weight is mx_linear's
    with pytest.raises(ValueError):
        ops.mx_expert_linear(torch.randn(2, 32), p, s, idx)  # K mismatch
    with pytest.raises(ValueError):
        ops.mx_expert_linear(x, p, s[:, :, :1], idx)        # scale blocks
    with pytest.raises(ValueError):
        ops.mx_expert_linear(x, p, s, torch.tensor([0, 1, 2], dtype=torch.int32))   # 3 pairs, 2 rows
    with pytest.raises(ValueError):
        ops.mx_expert_linear(x, p, s, idx, xdiv=0)
    with pytest.raises(ValueError):
        ops.mx_expert_linear(x, p[:, :5], s[:, :5], idx, glu=True)    # odd [gate; up] rows
    with pytest.raises(ValueError):
        ops.mx_experts_linear(torch.randn(3, 2, 64), p, s)  # 3 != E
    with pytest.raises(ValueError):
        ops.mx_experts_linear(torch.randn(64), p, s)


# ---------------------------------------------------------------------------------------- layers
def test_mxfp4_expert_layers_bits_and_state_dicts():
    from neuronx_distributed_llama3_2_amd.modules.moe.moe_parallel_layers import (ExpertFusedColumnParallelLinear,
                                                                                  ExpertFusedRowParallelLinear)
    from neuronx_distributed_llama3_2_amd.quantization import (MXFP4ExpertFusedColumnParallel, MXFP4ExpertFusedRowParallel,
                                                               convert, get_default_mxfp4_qconfig_dict,
                                                               get_mxfp4_moe_quant_module_mappings)

    _single_process_tp1()
    ops = _ops()
    torch.manual_seed(7)
    E, H, I = 3, 64, 96
    qc = get_default_mxfp4_qconfig_dict()
    cases = ((ExpertFusedColumnParallelLinear(E, H, 2 * I, stride=2), MXFP4ExpertFusedColumnParallel, 1, 2),
             (ExpertFusedRowParallelLinear(E, I, H, reduce_output=False), MXFP4ExpertFusedRowParallel, 2, 1))
    for f, qcls, pdim, stride in cases:
        with torch.no_grad():
            f.weight.normal_()
        i, o = f.weight.shape[1], f.weight.shape[2]
        a = qcls.from_float(f, q_config=qc)
        assert isinstance(a, qcls) and a.weight.dtype == torch.uint8 and a.scale.dtype == torch.uint8
        assert a.weight.shape == (E, o, i // 2) and a.scale.shape == (E, o, i // 32)
        for t in (a.weight, a.scale):
            assert t.tensor_model_parallel and t.partition_dim == pdim and t.partition_stride == stride
        p, s = ops.quantize_mxfp4(f.weight.detach().transpose(1, 2).contiguous())
        assert torch.equal(a.weight, p) and torch.equal(a.scale, s)
        # an unloaded layer dequantises to zeros
        kw = {"reduce_output": False} if qcls is MXFP4ExpertFusedRowParallel else {}
        b = qcls(E, f.input_size, f.output_size, dtype=torch.float32, stride=stride, **kw)
        assert bool((b.scale == 127).all()) and not bool(ops.dequantize_mxfp4(b.weight, b.scale, torch.float32).any())
        # a float weight in the logical [E, in, out] shape is quantized on load: the same bits
        b.load_state_dict({"weight": f.weight.detach().clone()})
        assert torch.equal(b.weight, a.weight) and torch.equal(b.scale, a.scale)
        with pytest.raises(RuntimeError):
            qcls(E, f.input_size, f.output_size, dtype=torch.float32, stride=stride, **kw).load_state_dict(
                {"weight": torch.zeros(E, i + 32, o)})
        # a packed state dict round-trips as it is
        c = qcls(E, f.input_size, f.output_size, dtype=torch.float32, stride=stride, **kw)
        c.load_state_dict(a.state_dict())
        assert torch.equal(c.weight, a.weight) and torch.equal(c.scale, a.scale)
        # forward: every expert on its own rows, or one shared row block
        wd = ops.dequantize_mxfp4(p, s, torch.float32)
        x = torch.randn(E, 5, i)
        torch.testing.assert_close(c(x), torch.bmm(x, wd.transpose(1, 2)), atol=1e-6, rtol=1e-6)
        torch.testing.assert_close(c(x[:1]), torch.bmm(x[:1].expand(E, 5, i), wd.transpose(1, 2)), atol=1e-6, rtol=1e-6)
        m = convert(torch.nn.Sequential(f), qc, mapping=get_mxfp4_moe_quant_module_mappings())
        assert isinstance(m[0], qcls) and torch.equal(m[0].weight, a.weight)
    # blocks run along `in`: a row shard whose local in-features are not whole blocks is refused
    with pytest.raises(ValueError):
        MXFP4ExpertFusedRowParallel(E, 48, H)
    with pytest.raises(ValueError):
        MXFP4ExpertFusedRowParallel.from_float(ExpertFusedRowParallelLinear(E, 48, H), q_config=qc)


def test_default_mxfp4_mapping_still_refuses_experts():
    from neuronx_distributed_llama3_2_amd.modules.moe.moe_parallel_layers import ExpertFusedColumnParallelLinear
    from neuronx_distributed_llama3_2_amd.quantization import convert, get_default_mxfp4_qconfig_dict

    _single_process_tp1()
    with pytest.raises(NotImplementedError):
        convert(torch.nn.Sequential(ExpertFusedColumnParallelLinear(2, 32, 32)), get_default_mxfp4_qconfig_dict())


# ---------------------------------------------------------------------------------------- model
def _fq(w):
    ops = _ops()
    return ops.dequantize_mxfp4(*ops.quantize_mxfp4(w.contiguous()), w.dtype)


def _fake_quantized_full_sd(full):
    """Framework-named full state dict whose o_proj / lm_head / expert weights went through
    quantize -> dequantize (experts along their in-features, i.e. on the transposed weight);
    router, fused QKV, norms and the embedding stay as they are."""
    out = {}
    for k, v in full.items():
        if "expert_mlps" in k and k.endswith("proj.weight"):
            out[k] = _fq(v.transpose(1, 2)).transpose(1, 2).contiguous()
        elif k.endswith("o_proj.weight") or k == "lm_head.weight":
            out[k] = _fq(v)
        else:
            out[k] = v.detach().clone()
    return out


def _mixtral_full(seed, **kw):
    from neuronx_distributed_llama3_2_amd.models.mixtral.convert import mixtral_hf_to_nxd

    cfg = _mixtral_cfg(intermediate_size=128, **kw)   # TP=2 shards of 64 in-features: whole blocks
    return cfg, mixtral_hf_to_nxd(_mixtral_hf(cfg, seed=seed).state_dict(), cfg)


def test_mixtral_mxfp4_matches_fake_quantized_float_twin_and_reloads():
    from neuronx_distributed_llama3_2_amd.inference import MixtralForCausalLMInference
    from neuronx_distributed_llama3_2_amd.quantization import (MXFP4ColumnParallel, MXFP4ExpertFusedColumnParallel,
                                                               MXFP4ExpertFusedRowParallel, MXFP4RowParallel)

    cfg, full = _mixtral_full(1)
    q = _app(MixtralForCausalLMInference, cfg, full, quantized=True, quantization_type="mxfp4")
    layer = q.model.model.layers[0]
    mo = layer.block_sparse_moe.expert_mlps.mlp_op
    assert isinstance(mo.gate_up_proj, MXFP4ExpertFusedColumnParallel) and isinstance(mo.down_proj, MXFP4ExpertFusedRowParallel)
    assert isinstance(layer.self_attn.o_proj, MXFP4RowParallel) and isinstance(q.model.lm_head, MXFP4ColumnParallel)
    assert layer.block_sparse_moe.router.linear_router.weight.is_floating_point()
    assert all(p.is_floating_point() for p in layer.self_attn.qkv_proj.parameters())
    E, H, I = 4, cfg.hidden_size, cfg.intermediate_size
    assert mo.gate_up_proj.weight.shape == (E, 2 * I, H // 2) and mo.down_proj.weight.shape == (E, H, I // 2)
    nbytes = sum(p.numel() * p.element_size() for m in (mo.gate_up_proj, mo.down_proj) for p in m.parameters())
    assert nbytes * 32 == E * 3 * H * I * 17   # 4.25 bits per expert weight
    assert [tuple(t.shape) for t in q.model._expert_scratch] == [(E, 2 * I, H), (E, H, I)]

    f = _app(MixtralForCausalLMInference, cfg, _fake_quantized_full_sd(full))
    torch.manual_seed(6)
    ids = torch.randint(3, cfg.vocab_size, (2, 12))
    mask = torch.ones_like(ids)
    mask[1, 9:] = 0
    lq, lf = q._context_encode(ids, mask), f._context_encode(ids, mask)
    torch.testing.assert_close(lq, lf, atol=1e-4, rtol=1e-4)
    tq = q.generate(ids[:1], max_new_tokens=8, eos_token_id=-1)
    tf = f.generate(ids[:1], max_new_tokens=8, eos_token_id=-1)
    assert tq.shape == (1, 20) and torch.equal(tq, tf)
    # compile -> load keeps the packed expert shards and the setting
    d = tempfile.mkdtemp()
    q.compile(d)
    q2 = MixtralForCausalLMInference.load(d, dtype=torch.float32)
    assert q2.config.quantized and str(q2.config.quantization_type) == "mxfp4"
    mo2 = q2.model.model.layers[1].block_sparse_moe.expert_mlps.mlp_op
    mo1 = q.model.model.layers[1].block_sparse_moe.expert_mlps.mlp_op
    for a, b in ((mo2.gate_up_proj, mo1.gate_up_proj), (mo2.down_proj, mo1.down_proj)):
        assert a.weight.dtype == torch.uint8 and torch.equal(a.weight, b.weight) and torch.equal(a.scale, b.scale)
    assert torch.equal(q2._context_encode(ids, mask), lq)
    assert torch.equal(q2.generate(ids[:1], max_new_tokens=8, eos_token_id=-1), tq)


def test_mxfp4_dispatch_regimes_agree():
    """One block, three regimes: 1 token (selective: n * k <= E), 3 tokens with E = 4 (all-experts
    form) and 40 tokens (scratch + the float grouped code), each against the float twin's block."""
    from neuronx_distributed_llama3_2_amd.inference import MixtralForCausalLMInference

    cfg, full = _mixtral_full(2)
    q = _app(MixtralForCausalLMInference, cfg, full, quantized=True, quantization_type="mxfp4").model
    f = _app(MixtralForCausalLMInference, cfg, _fake_quantized_full_sd(full)).model
    lq, lf = q.model.layers[0], f.model.layers[0]
    gu, d = q._expert_weights(lq)
    assert isinstance(gu, tuple) and gu[0].dtype == torch.uint8
    called = []
    for name in ("_selective_mx", "_all_experts_mx", "_dequantized_experts", "_all_experts", "_grouped"):
        def spy(*a, _n=name, _f=getattr(q, name), **kw):
            called.append(_n)
            return _f(*a, **kw)
        setattr(q, name, spy)
    torch.manual_seed(8)
    x40 = torch.randn(72, 64)
    ref = f._ffn(lf, x40)
    # the float code picks all-experts up to 64 tokens and the grouped GEMMs above; both read the scratch
    want = {1: ["_selective_mx"], 3: ["_all_experts_mx"], 40: ["_dequantized_experts", "_all_experts"],
            72: ["_dequantized_experts", "_grouped"]}
    for n in (1, 3, 40, 72):
        del called[:]
        torch.testing.assert_close(q._ffn(lq, x40[:n]), ref[:n], atol=1e-5, rtol=1e-5)
        assert called == want[n], (n, called)
    # the same tokens through every regime of the packed block, routing held fixed
    x = x40[:3]
    top_w, top_i = q._route(lq, x)
    a = torch.cat([q._selective_mx(x[i:i + 1], top_w[i:i + 1], top_i[i:i + 1], gu, d) for i in range(3)])
    b = q._all_experts_mx(x, top_w, top_i, gu, d)
    c = q._grouped(x, top_w, top_i, *q._dequantized_experts(gu, d))
    torch.testing.assert_close(a, b, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(b, c, atol=1e-5, rtol=1e-5)


def test_dbrx_mxfp4_matches_fake_quantized_float_twin():
    from neuronx_distributed_llama3_2_amd.inference import DbrxForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.mixtral.convert import dbrx_hf_to_nxd, dbrx_to_mixtral_config

    c, hf = _dbrx_hf()
    cfg = dbrx_to_mixtral_config(c)
    full = dbrx_hf_to_nxd(hf.state_dict(), cfg)
    q = _app(DbrxForCausalLMInference, cfg, full, quantized=True, quantization_type="mxfp4")
    f = _app(DbrxForCausalLMInference, cfg, _fake_quantized_full_sd(full))
    assert q.model.model.layers[0].block_sparse_moe.expert_mlps.mlp_op.down_proj.weight.dtype == torch.uint8
    torch.manual_seed(9)
    ids = torch.randint(3, 256, (1, 11))
    torch.testing.assert_close(q._context_encode(ids), f._context_encode(ids), atol=1e-4, rtol=1e-4)
    assert torch.equal(q.generate(ids, max_new_tokens=8, eos_token_id=-1), f.generate(ids, max_new_tokens=8, eos_token_id=-1))


def test_moe_int8_types_still_raise():
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, MixtralForCausalLMInference

    cfg = _mixtral_cfg()
    for qt in ("per_channel_symmetric", "per_tensor_symmetric"):
        icfg = InferenceConfig(tp_degree=1, batch_size=1, seq_len=32, max_context_length=16, quantized=True,
                               quantization_type=qt)
        with pytest.raises(NotImplementedError, match="int8"):
            MixtralForCausalLMInference(cfg, icfg, dtype=torch.float32, init_weights=False)


def _w_mx_moe_tp(rank, world, out_dir):
    from neuronx_distributed_llama3_2_amd.inference import MixtralForCausalLMInference

    cfg, full = _mixtral_full(3)
    ps.initialize_model_parallel(tensor_model_parallel_size=world)
    m = _app(MixtralForCausalLMInference, cfg, full, tp=world, quantized=True, quantization_type="mxfp4")
    torch.manual_seed(5)
    ids = torch.randint(3, cfg.vocab_size, (2, 9))
    logits = m._context_encode(ids)
    greedy = m.generate(ids, max_new_tokens=6, eos_token_id=-1)
    mo = m.model.model.layers[1].block_sparse_moe.expert_mlps.mlp_op
    shard = {f"{name}.{part}": getattr(getattr(mo, name), part).detach().clone()
             for name in ("gate_up_proj", "down_proj") for part in ("weight", "scale")}
    torch.save({"logits": logits, "greedy": greedy, "shard": shard}, os.path.join(out_dir, f"tp{world}_r{rank}.pt"))


def test_mixtral_mxfp4_tp2_shards_and_logits_match_tp1():
    from neuronx_distributed_llama3_2_amd.parallel_layers.sharding import shard_tensor

    d = tempfile.mkdtemp()
    run_distributed(_w_mx_moe_tp, 1, d)
    run_distributed(_w_mx_moe_tp, 2, d)
    one = torch.load(os.path.join(d, "tp1_r0.pt"))
    two = [torch.load(os.path.join(d, f"tp2_r{r}.pt")) for r in range(2)]
    # packed [E, out, in/2] / scale [E, out, in/32]: gate_up shards `out` (dim 1) with stride 2 for
    # [gate; up], down shards `in` (dim 2); whole blocks, so quantizing commutes with the slicing
    for name, dim, stride in (("gate_up_proj", 1, 2), ("down_proj", 2, 1)):
        attrs = {"tp": True, "dim": dim, "stride": stride, "qkv": None}
        for part in ("weight", "scale"):
            t = one["shard"][f"{name}.{part}"]
            for r in range(2):
                got = two[r]["shard"][f"{name}.{part}"]
                assert got.dtype == torch.uint8 and got.shape[dim] * 2 == t.shape[dim]
                assert torch.equal(got, shard_tensor(t, attrs, 2, r)), (name, part, r)
    I = 128
    gu1, gu2 = one["shard"]["gate_up_proj.weight"], two[1]["shard"]["gate_up_proj.weight"]
    assert torch.equal(gu2[:, :I // 2], gu1[:, I // 2:I]) and torch.equal(gu2[:, I // 2:], gu1[:, I + I // 2:])
    for r in range(2):
        torch.testing.assert_close(two[r]["logits"], one["logits"], atol=1e-4, rtol=1e-4)
        assert torch.equal(two[r]["greedy"], one["greedy"])


def test_mixtral_and_dbrx_example_cli_mxfp4(tmp_path):
    """examples/inference/run_mixtral.py / run_dbrx.py with --quantized --quantization_type mxfp4:
    trace an HF directory, reload the packed shards, generate."""
    import sys

    from safetensors.torch import load_file
    from transformers import DbrxConfig, DbrxForCausalLM

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples", "inference"))
    import run_dbrx  # noqa: F401  (module import = the CLI wiring is valid)
    import run_mixtral  # noqa: F401
    from llama3_2_runner import main as runner_main

    from neuronx_distributed_llama3_2_amd.inference.moe import DbrxRunner, MixtralRunner

    cfg = _mixtral_cfg(intermediate_size=128, num_hidden_layers=1)
    src = str(tmp_path / "mixtral")
    _mixtral_hf(cfg, seed=4).save_pretrained(src)
    torch.manual_seed(0)
    dsrc = str(tmp_path / "dbrx")
    DbrxForCausalLM(DbrxConfig(d_model=64, n_heads=4, n_layers=1, max_seq_len=128, vocab_size=128,
                               attn_config=dict(kv_n_heads=2, clip_qkv=8.0, rope_theta=10000.0),
                               ffn_config=dict(ffn_hidden_size=64, moe_num_experts=4, moe_top_k=2))).save_pretrained(dsrc)
    for model_dir, runner, name in ((src, MixtralRunner, "m"), (dsrc, DbrxRunner, "d")):
        traced = str(tmp_path / f"traced_{name}")
        runner_main(["trace", "--model_path", model_dir, "--traced_path", traced, "--max_prompt_length", "16",
                     "--sequence_length", "24", "--quantized", "--quantization_type", "mxfp4"], runner_cls=runner)
        shard = load_file(os.path.join(traced, "tp0_sharded_checkpoint.safetensors"))
        key = "model.layers.0.block_sparse_moe.expert_mlps.mlp_op.down_proj."
        assert shard[key + "weight"].dtype == torch.uint8 and shard[key + "scale"].dtype == torch.uint8
        assert shard[key + "weight"].shape[1:] == (64, shard[key + "scale"].shape[2] * 16)
        out = runner_main(["generate", "--traced_path", traced, "--prompt_ids", "3,4,5"], runner_cls=runner)
        assert out.shape == (1, 24)
