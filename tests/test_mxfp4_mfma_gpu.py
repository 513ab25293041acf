"""MXFP4 decode on MFMA weight tiles on MI355X (csrc/gemv_mx_mfma.hip): mx_gemm and mx_experts_gemm
per element against fp64 of the dequantized weights for 1..16 rows, the guards of the K tail and of
the rows past M, the fused SwiGLU, the VALU kernels they leave in place, and a quantized tiny Llama
decoding at batch 12 eagerly and from a hipGraph.  The kernels are called through
ext() directly, so these tests do not depend on the routing default (NXD_MX_MFMA)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

_WIDE = 8192 + 3     # several tiles per wave, and a ragged last tile
_SENTINEL = 0x7B5A   # bf16 bit pattern the kernels are not going to produce by accident


def _ext():
    from neuronx_distributed_llama3_2_amd.ops import ext

    return ext()


def _x16(K, seed):
    """16 rows as a column slice of a wider tensor (ldx != K): GPU bf16 and CPU fp64."""
    from test_mxfp4_moe_gpu import _x

    x = _x(16, K, seed)
    return x, x.cpu().double()


def _gemm(x, packed, scale, bias, N, glu=False, cfg=0):
    y = torch.empty((x.shape[0], N), dtype=torch.bfloat16, device="cuda")
    _ext().mx_gemm(x, packed, scale, bias, y, glu, cfg)
    return y


def _cfgs(glu=False):
    """Every (tiles per wave, K split) instantiation, as the cfg argument that forces it: the launcher's
    own choice depends on the shape, and the small shapes here would only ever reach a few."""
    return [16 * T + KS for T in ((1, 2) if glu else (1, 2, 4)) for KS in (1, 2, 4)]


def _bound_ratio(y, ref, mag, K):
    """max over elements of |y - ref| / (2^-8 |ref| + K 2^-24 sum_k |x_k w_k|): exact bf16 x bf16
    products, fp32 summation in any order and one bf16 rounding keep it <= 1."""
    assert bool(torch.isfinite(y).all())
    err = (y.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * mag
    over = float((err - bound).max())
    return float((err / bound.clamp(min=1e-300)).max()), over


@pytest.mark.parametrize("N", [1, 5, 17, 40, _WIDE])
@pytest.mark.parametrize("K", [32, 96, 2080, 4096])
def test_mx_gemm_matches_fp64(K, N):
    """Per element against fp64.  K = 32 leaves three of the four lane groups idle, 96 one; 2080 is 65
    blocks (no multiple of 4 or of a K split).  Worst err/bound ratios measured on MI355X are in
    profiles/LOG.md (MXFP4 on MFMA weight tiles)."""
    from test_mxfp4_gpu import _case

    c = _case(K, N)
    x16, x64 = _x16(K, 3 * K + N)
    ref_all = x64 @ c["wd"].t()
    mag_all = x64.abs() @ c["wd"].abs().t()
    worst = 0.0
    for M in (1, 3, 4, 8, 9, 13, 16):
        x = x16[:M]
        assert x.stride(0) != K
        for with_bias in (False, True):
            bias = c["bias"] if with_bias else None
            y = _gemm(x, c["packed"], c["scale"], bias, N)
            assert torch.equal(y, _gemm(x, c["packed"], c["scale"], bias, N))   # no atomics: the same bits
            ref, mag = ref_all[:M], mag_all[:M]
            if with_bias:
                ref, mag = ref + c["b64"], mag + c["b64"].abs()
            ratio, over = _bound_ratio(y.cpu(), ref, mag, K)
            worst = max(worst, ratio)
            assert over <= 0, (K, N, M, with_bias, ratio)
    for cfg in _cfgs():   # every instantiation, at 13 rows with the bias
        y = _gemm(x16[:13], c["packed"], c["scale"], c["bias"], N, cfg=cfg)
        assert torch.equal(y, _gemm(x16[:13], c["packed"], c["scale"], c["bias"], N, cfg=cfg))
        ratio, over = _bound_ratio(y.cpu(), ref_all[:13] + c["b64"], mag_all[:13] + c["b64"].abs(), K)
        worst = max(worst, ratio)
        assert over <= 0, (K, N, cfg, ratio)
    print(f"mx_gemm K={K} N={N}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("K", [32, 96])
def test_mx_gemm_guards(K):
    """x is the first M rows of a taller tensor whose other rows are NaN, y the first M rows of a
    16-row tensor holding a sentinel: idle lane groups and rows past M must neither read garbage into
    the tile nor store."""
    from test_mxfp4_gpu import _case

    N = 40
    c = _case(K, N)
    x16, x64 = _x16(K, 5 * K)
    for M in (1, 3, 8, 13):
        tall = torch.full((20, K + 64), float("nan"), dtype=torch.bfloat16, device="cuda")
        tall[:M, 32:32 + K] = x16[:M]
        x = tall[:M, 32:32 + K]
        ybuf = torch.full((16, N), _SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        _ext().mx_gemm(x, c["packed"], c["scale"], None, ybuf[:M], False)
        assert bool(torch.isfinite(ybuf[:M]).all()), (K, M)
        assert bool((ybuf[M:].view(torch.int16) == _SENTINEL).all()), (K, M)
        ref = x64[:M] @ c["wd"].t()
        mag = x64[:M].abs() @ c["wd"].abs().t()
        ratio, over = _bound_ratio(ybuf[:M].cpu(), ref, mag, K)
        assert over <= 0, (K, M, ratio)


@pytest.mark.parametrize("K,N", [(32, _WIDE), (2080, 5), (4096, 1536)])
def test_mx_gemm_glu(K, N):
    """Fused SwiGLU ([gate; up] rows): through __expf, so the tolerance of test_mx_gemv_glu."""
    from test_mxfp4_gpu import _case

    c = _case(K, N, glu=True)
    x16, x64 = _x16(K, 7 * K + N)
    full = x64 @ c["wd"].t()
    for M in (3, 8, 16):
        for with_bias in (False, True):
            bias = c["bias"] if with_bias else None
            y = _gemm(x16[:M], c["packed"], c["scale"], bias, N, glu=True)
            assert torch.equal(y, _gemm(x16[:M], c["packed"], c["scale"], bias, N, glu=True))
            f = full[:M] + (c["b64"] if with_bias else 0.0)
            ref = (torch.nn.functional.silu(f[:, :N]) * f[:, N:]).float()
            torch.testing.assert_close(y.cpu().float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)
    f = full[:13] + c["b64"]
    ref = (torch.nn.functional.silu(f[:, :N]) * f[:, N:]).float()
    for cfg in _cfgs(glu=True):
        y = _gemm(x16[:13], c["packed"], c["scale"], c["bias"], N, glu=True, cfg=cfg)
        torch.testing.assert_close(y.cpu().float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)


def _experts_gemm(x, packed, scale, M, N, glu=False, cfg=0):
    y = torch.empty((packed.shape[0], M, N), dtype=torch.bfloat16, device="cuda")
    _ext().mx_experts_gemm(x, packed, scale, y, glu, cfg)
    return y


@pytest.mark.parametrize("K,N", [(32, _WIDE), (2080, 5), (4096, 40)])
def test_mx_experts_gemm_matches_fp64(K, N):
    """All experts of a strided stack, x shared or per expert."""
    from test_mxfp4_moe_gpu import _check_bound, _stack, _x

    E = 4
    packed, scale, wd = _stack(E, N, K, 7 * K + N)
    for M in (3, 8, 16):
        xs = _x(M, K, 17 * M)
        xp = _x(E * M, K, 19 * M).unflatten(0, (E, M))
        assert not xp.is_contiguous()
        for x, x64 in ((xs, xs.double().expand(E, M, K)), (xp, xp.double())):
            y = _experts_gemm(x, packed, scale, M, N)
            assert torch.equal(y, _experts_gemm(x, packed, scale, M, N))
            ref = torch.einsum("emk,enk->emn", x64, wd)
            mag = torch.einsum("emk,enk->emn", x64.abs(), wd.abs())
            _check_bound(y, ref, mag, K, f"mfma all experts K={K} N={N} M={M} {'shared' if x is xs else 'per expert'}")
    for cfg in _cfgs():   # x, ref, mag: 16 rows per expert
        _check_bound(_experts_gemm(x, packed, scale, 16, N, cfg=cfg), ref, mag, K, f"mfma all experts K={K} N={N} cfg={cfg}")


def test_mx_experts_gemm_glu():
    from test_mxfp4_moe_gpu import _stack, _x

    E, K, N, M = 4, 2080, 5, 13
    packed, scale, wd = _stack(E, 2 * N, K, 23)
    x = _x(E * M, K, 29).unflatten(0, (E, M))
    y = _experts_gemm(x, packed, scale, M, N, glu=True)
    full = torch.einsum("emk,enk->emn", x.double(), wd)
    ref = (torch.nn.functional.silu(full[..., :N]) * full[..., N:]).float()
    torch.testing.assert_close(y.float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)


@pytest.mark.parametrize("N", [5, _WIDE])
def test_valu_mx_gemv_still_covered(N):
    """The VALU bodies at 4 and 8 rows, called directly: covered whatever the routing default is."""
    from test_mxfp4_gpu import _case

    K = 2080
    c = _case(K, N)
    x16, x64 = _x16(K, 11 * K + N)
    for M in (4, 8):
        y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        _ext().mx_gemv(x16[:M], c["packed"], c["scale"], None, y, False)
        ref = x64[:M] @ c["wd"].t()
        mag = x64[:M].abs() @ c["wd"].abs().t()
        ratio, over = _bound_ratio(y.cpu(), ref, mag, K)
        print(f"valu mx_gemv K={K} N={N} M={M}: err/bound {ratio:.3f}")
        assert over <= 0, (N, M, ratio)


def test_mx_linear_routes_to_the_mfma_form(monkeypatch):
    """mx_linear at 12 rows gives the bits of mx_gemm, at 4 rows those of the kernel the knob names;
    mx_experts_linear keeps the VALU expert kernel whatever the knob says."""
    from test_mxfp4_gpu import _case
    from test_mxfp4_moe_gpu import _stack

    from neuronx_distributed_llama3_2_amd.ops import gemv

    K, N = 2080, 40
    c = _case(K, N)
    x16, _ = _x16(K, 13)
    monkeypatch.setattr(gemv, "_MX_MFMA", 9)
    assert torch.equal(gemv.mx_linear(x16[:12], c["packed"], c["scale"], c["bias"]),
                       _gemm(x16[:12], c["packed"], c["scale"], c["bias"], N))
    # the all-experts op is not routed to the MFMA form: 4 rows stay on the VALU expert kernel
    packed, scale, _ = _stack(4, N, K, 43)
    y4e = torch.empty((4, 4, N), dtype=torch.bfloat16, device="cuda")
    _ext().mx_experts_gemv(x16[:4], packed, scale, y4e, False)
    assert torch.equal(gemv.mx_experts_linear(x16[:4], packed, scale), y4e)
    y4 = torch.empty((4, N), dtype=torch.bfloat16, device="cuda")
    _ext().mx_gemv(x16[:4], c["packed"], c["scale"], None, y4, False)
    assert torch.equal(gemv.mx_linear(x16[:4], c["packed"], c["scale"]), y4)
    monkeypatch.setattr(gemv, "_MX_MFMA", 2)
    assert torch.equal(gemv.mx_linear(x16[:4], c["packed"], c["scale"]), _gemm(x16[:4], c["packed"], c["scale"], None, N))


# ------------------------------------------------------------------------------------------ models
def test_mxfp4_llama_batch12_decode_on_gpu():
    """The tiny Llama of test_mxfp4_model_decode_on_gpu at batch 12 (every projection on mx_gemm):
    hipGraph and eager decode give the same 8 greedy tokens, one decode step stays within 0.05
    (max-abs difference / max-abs logit) of the bf16 model holding the dequantized weights."""
    from test_inference_gpu import _cfg
    from test_mxfp4 import _fake_quantized_sd
    from transformers import LlamaForCausalLM as HF

    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd
    from neuronx_distributed_llama3_2_amd.ops import gemv

    B = 12
    assert gemv.mx_route(B) == "gemm"
    cfg = _cfg()
    torch.manual_seed(0)
    sd = {k: v.detach().to(torch.bfloat16) for k, v in HF(cfg).state_dict().items()}
    dev = torch.device("cuda")

    def model(sd_, graphs, steps, **kw):
        icfg = InferenceConfig(batch_size=B, seq_len=256, max_context_length=128, use_hip_graphs=graphs,
                               decode_graph_steps=steps, **kw)
        m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, device=dev, init_weights=False)
        m._load_full(hf_to_nxd(sd_, cfg))
        return m

    g = model(sd, True, 8, quantized=True, quantization_type="mxfp4")
    e = model(sd, False, 1, quantized=True, quantization_type="mxfp4")
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (B, 40))
    a = g.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    assert a.shape == (B, 48) and torch.equal(a, b), (a[:, 40:], b[:, 40:])

    f = model(_fake_quantized_sd(sd), False, 1)
    emb = f.model.model.embed_tokens.weight
    f.model.lm_head.weight = torch.nn.Parameter(gemv.dequantize_mxfp4(*gemv.quantize_mxfp4(emb), torch.bfloat16),
                                                requires_grad=False)
    f.model._decode_fused_ok = False
    f.generate(ids, max_new_tokens=8, eos_token_id=-1)
    f.model.kv_cache.copy_(e.model.kv_cache)
    last = b[:, -1:].cuda()
    pos = torch.full((B, 1), b.shape[1] - 1, dtype=torch.int64, device="cuda")
    sid = torch.arange(B, device="cuda")
    clen = torch.full((B,), b.shape[1], dtype=torch.int32, device="cuda")
    dq = e.model.forward_tokens(last, pos, sid, clen).float()
    df = f.model.forward_tokens(last, pos, sid, clen).float()
    dec = float((dq - df).abs().max() / df.abs().max())
    print(f"mxfp4 batch {B} vs fake-quantized bf16 model: decode step {dec:.4f}")
    assert dec < 0.05, dec
