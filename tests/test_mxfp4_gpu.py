"""MXFP4 weight-only kernels on MI355X (csrc/gemv_mx.hip): mx_dequant bit-exact against the CPU
dequantizer, mx_gemv per element against fp64 of the dequantized weights, and a quantized tiny
Llama decoding eagerly and from a hipGraph."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    from neuronx_distributed_llama3_2_amd.ops import gemv

    return gemv


def _random_mx(N, K, seed, e_lo, e_hi):
    """Random packed codes + scales (CPU): every one of the 16 codes present, some blocks all zero,
    some saturated at +6 / -6."""
    g = torch.Generator().manual_seed(seed)
    nb = K // 32
    codes = torch.randint(0, 16, (N, nb, 32), generator=g, dtype=torch.uint8)
    codes[0, 0, :16] = torch.arange(16, dtype=torch.uint8)
    kind = torch.randint(0, 8, (N, nb), generator=g)
    if N * nb > 1:
        codes[kind == 1] = 0
        codes[kind == 2] = 7
        codes[kind == 3] = 15
        codes[0, 0, :16] = torch.arange(16, dtype=torch.uint8)
        codes[0, 0, 16:] = 7
    codes = codes.reshape(N, K // 2, 2)
    packed = (codes[..., 0] | (codes[..., 1] << 4)).contiguous()
    scale = torch.randint(e_lo, e_hi + 1, (N, nb), generator=g, dtype=torch.uint8)
    return packed, scale


@pytest.mark.parametrize("N,K", [(1, 32), (5, 96), (130, 2080), (64, 4096)])
def test_mx_dequant_bit_exact(N, K):
    ops = _ops()
    from neuronx_distributed_llama3_2_amd.ops import ext

    ext()   # the native kernel must be present on a GPU box
    packed, scale = _random_mx(N, K, 10 + N, 97, 137)
    assert len(torch.unique(torch.cat([packed & 0xF, packed >> 4]))) == 16
    want = ops.dequantize_mxfp4(packed, scale, torch.bfloat16)           # CPU: pure torch
    got = ops.dequantize_mxfp4(packed.cuda(), scale.cuda(), torch.bfloat16)
    assert got.dtype == torch.bfloat16 and got.shape == (N, K)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got.cpu().float(), ops.dequantize_mxfp4(packed, scale, torch.float32))   # bf16 is exact


_WIDE = 8192 + 3   # takes the several-rows-per-wave launch, with a ragged last wave
_CASES = {}


def _case(K, N, glu=False):
    """(packed, scale, x wide, bias) on the GPU and the fp64 CPU operands, built once per shape."""
    key = (K, N, glu)
    if key not in _CASES:
        ops = _ops()
        Nw = 2 * N if glu else N
        packed, scale = _random_mx(Nw, K, K + N, 121, 127)
        g = torch.Generator().manual_seed(K * 7 + N)
        xw = torch.randn(8, K + 64, generator=g).to(torch.bfloat16)
        bias = torch.randn(Nw, generator=g).to(torch.bfloat16)
        wd = ops.dequantize_mxfp4(packed, scale, torch.float32).double()
        _CASES[key] = dict(packed=packed.cuda(), scale=scale.cuda(), xw=xw.cuda(), bias=bias.cuda(), wd=wd,
                           x64=xw[:, 32:32 + K].double(), b64=bias.double())
    return _CASES[key]


@pytest.mark.parametrize("N", [1, 5, 1536, _WIDE])
@pytest.mark.parametrize("K", [32, 2080, 4096])
def test_mx_gemv_matches_fp64(K, N):
    """Per element: exact bf16 x bf16 products, fp32 summation in any order and one bf16 rounding give
    |y - ref| <= 2^-8 |ref| + K 2^-24 sum_k |x_k w_k| (the bias counts as one more addend)."""
    ops = _ops()
    from neuronx_distributed_llama3_2_amd.ops import ext

    c = _case(K, N)
    if N == _WIDE:
        assert ext().mx_gemv_rows_per_wave(N, K) >= 2
    else:
        assert ext().mx_gemv_rows_per_wave(N, K) == 1
    ref_all = c["x64"] @ c["wd"].t()
    mag_all = c["x64"].abs() @ c["wd"].abs().t()
    for M in (1, 2, 3, 4, 8):
        x = c["xw"][:M, 32:32 + K]           # a column slice of a wider tensor: ldx != K
        assert x.stride(0) != K
        for with_bias in (False, True):
            y = ops.mx_linear(x, c["packed"], c["scale"], c["bias"] if with_bias else None)
            assert y.shape == (M, N) and y.dtype == torch.bfloat16
            y2 = ops.mx_linear(x, c["packed"], c["scale"], c["bias"] if with_bias else None)
            assert torch.equal(y, y2)        # no atomics: two calls give the same bits
            ref, mag = ref_all[:M], mag_all[:M]
            if with_bias:
                ref, mag = ref + c["b64"], mag + c["b64"].abs()
            err = (y.cpu().double() - ref).abs()
            bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * mag
            worst = float((err - bound).max())
            print(f"K={K} N={N} M={M} bias={with_bias}: max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
            assert worst <= 0, (K, N, M, with_bias, worst)


@pytest.mark.parametrize("K,N", [(32, _WIDE), (2080, 5), (4096, 1536)])
def test_mx_gemv_glu(K, N):
    """Fused SwiGLU ([gate; up] rows): through __expf, so the tolerance of test_gemv_skinny."""
    ops = _ops()
    c = _case(K, N, glu=True)
    full = c["x64"] @ c["wd"].t()
    for M in (1, 3, 8):
        x = c["xw"][:M, 32:32 + K]
        for with_bias in (False, True):
            y = ops.mx_linear(x, c["packed"], c["scale"], c["bias"] if with_bias else None, glu=True)
            assert y.shape == (M, N)
            assert torch.equal(y, ops.mx_linear(x, c["packed"], c["scale"], c["bias"] if with_bias else None, glu=True))
            f = full[:M] + (c["b64"] if with_bias else 0.0)
            ref = (torch.nn.functional.silu(f[:, :N]) * f[:, N:]).float()
            torch.testing.assert_close(y.cpu().float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)


def test_mx_linear_fallbacks_on_gpu(monkeypatch):
    """M > 8 (mx_dequant + GEMM), a misaligned weight view and NXD_FORCE_REFERENCE=1 all agree with
    the decode kernel's result."""
    ops = _ops()
    c = _case(4096, 1536)
    x9 = torch.cat([c["xw"][:, 32:32 + 4096], c["xw"][:1, 32:32 + 4096]]).contiguous()
    ref = (x9.cpu().double() @ c["wd"].t()).float()
    tol = dict(atol=2e-2 * float(ref.abs().max()), rtol=2e-2)
    torch.testing.assert_close(ops.mx_linear(x9, c["packed"], c["scale"]).cpu().float(), ref, **tol)
    shifted = torch.empty(c["packed"].numel() + 1, dtype=torch.uint8, device="cuda")[1:].view_as(c["packed"])
    shifted.copy_(c["packed"])
    assert shifted.data_ptr() % 16 != 0
    torch.testing.assert_close(ops.mx_linear(x9[:3], shifted, c["scale"]).cpu().float(), ref[:3], **tol)
    monkeypatch.setenv("NXD_FORCE_REFERENCE", "1")
    torch.testing.assert_close(ops.mx_linear(x9[:3], c["packed"], c["scale"]).cpu().float(), ref[:3], **tol)


def test_mxfp4_model_decode_on_gpu():
    """A tiny Llama with quantization_type="mxfp4": eager and hipGraph decode give the same 8 greedy
    tokens, prefill and one decode step stay within the int8 GPU inference test's tolerance
    (max-abs difference / max-abs logit < 0.05) of the bf16 model holding the dequantized weights.
    Measured on MI355X: prefill 0.0000, decode step 0.0000, to the four decimals printed
    (profiles/mxfp4_accuracy.txt)."""
    from test_inference_gpu import _cfg
    from test_mxfp4 import _fake_quantized_sd
    from transformers import LlamaForCausalLM as HF

    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd
    from neuronx_distributed_llama3_2_amd.quantization import MXFP4ColumnParallel

    ops = _ops()
    cfg = _cfg()
    torch.manual_seed(0)
    # bf16 up front: the loader casts to the activation dtype before it quantizes, and the
    # fake-quantized twin below must quantize the very same values
    sd = {k: v.detach().to(torch.bfloat16) for k, v in HF(cfg).state_dict().items()}
    dev = torch.device("cuda")

    def model(sd_, graphs, steps, **kw):
        icfg = InferenceConfig(batch_size=2, seq_len=256, max_context_length=128, use_hip_graphs=graphs,
                               decode_graph_steps=steps, **kw)
        m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, device=dev, init_weights=False)
        m._load_full(hf_to_nxd(sd_, cfg))
        return m

    g = model(sd, True, 8, quantized=True, quantization_type="mxfp4")
    e = model(sd, False, 1, quantized=True, quantization_type="mxfp4")
    assert isinstance(g.model.lm_head, MXFP4ColumnParallel)
    assert g.model.model.layers[0].mlp.gate_up_proj.weight.dtype == torch.uint8
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (2, 40))
    a = g.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    assert a.shape == (2, 48) and torch.equal(a, b), (a[:, 40:], b[:, 40:])
    assert e.model._check_decode_fusable() is False   # packed weights stay on the unfused decode path

    # the bf16 model holding the same (exactly dequantized) weights; its tied head fake-quantized by hand
    f = model(_fake_quantized_sd(sd), False, 1)
    emb = f.model.model.embed_tokens.weight
    f.model.lm_head.weight = torch.nn.Parameter(ops.dequantize_mxfp4(*ops.quantize_mxfp4(emb), torch.bfloat16),
                                                requires_grad=False)
    f.model._decode_fused_ok = False
    lq, lf = e._context_encode(ids).float(), f._context_encode(ids).float()
    pre = float((lq - lf).abs().max() / lf.abs().max())
    f.generate(ids, max_new_tokens=8, eos_token_id=-1)
    f.model.kv_cache.copy_(e.model.kv_cache)
    last = b[:, -1:].cuda()
    pos = torch.full((2, 1), b.shape[1] - 1, dtype=torch.int64, device="cuda")
    sid = torch.arange(2, device="cuda")
    clen = torch.full((2,), b.shape[1], dtype=torch.int32, device="cuda")
    dq = e.model.forward_tokens(last, pos, sid, clen).float()
    df = f.model.forward_tokens(last, pos, sid, clen).float()
    dec = float((dq - df).abs().max() / df.abs().max())
    print(f"mxfp4 vs fake-quantized bf16 model: prefill {pre:.4f}, decode step {dec:.4f}")
    assert pre < 0.05 and dec < 0.05, (pre, dec)
