"""MXFP4 projections at 17..512 rows on MI355X (csrc/gemm_mx.hip): mx_gemm_wide per element against
fp64 of the dequantized weights across the row-chunk boundaries, the guards of the K tail and of the
rows past M, the fused SwiGLU, the routing of mx_linear and a quantized tiny Llama decoding at batch
24 eagerly and from a hipGraph.  The kernel is called through ext() directly, so only the routing and
model tests depend on the knob (NXD_MX_WIDE), which they set themselves."""

import pytest
import torch

pytestmark = pytest.mark.gpu

_WIDE = 8192 + 3
_SENTINEL = 0x7B5A
_ROWS = (17, 32, 47, 64, 65, 128, 129, 200)   # one tile + one row; both sides of the 64- and 128-row chunks
# every instantiation as cfg = 256 MT + 16 T + KS (row tiles per workgroup, output tiles per wave, K split)
_CFGS = [256 * 4 + 16 * T + KS for T in (1, 2) for KS in (1, 2)] + [256 * 8 + 16 * T + 1 for T in (1, 2)]


def _wide(x, packed, scale, bias, N, glu=False, cfg=0):
    from neuronx_distributed_llama3_2_amd.ops import ext

    y = torch.empty((x.shape[0], N), dtype=torch.bfloat16, device="cuda")
    ext().mx_gemm_wide(x, packed, scale, bias, y, glu, cfg)
    return y


@pytest.mark.parametrize("K,N", [(32, 1), (32, _WIDE), (96, 17), (2080, 40), (2080, _WIDE), (4096, 1536)])
def test_mx_gemm_wide_matches_fp64(K, N):
    """Per element: |y - ref| <= 2^-8 |ref| + K 2^-24 sum_k |x_k w_k| (exact bf16 products, fp32 sums in
    any order, one bf16 rounding).  K = 32 and 96 leave lane groups idle, 2080 is 65 blocks."""
    from test_mxfp4_gpu import _case
    from test_mxfp4_mfma_gpu import _bound_ratio
    from test_mxfp4_moe_gpu import _x

    c = _case(K, N)
    xg = _x(max(_ROWS), K, 3 * K + N)
    x64 = xg.cpu().double()
    ref_all = x64 @ c["wd"].t()
    mag_all = x64.abs() @ c["wd"].abs().t()
    worst = 0.0

    def check(M, bias, cfg):
        nonlocal worst
        y = _wide(xg[:M], c["packed"], c["scale"], bias, N, cfg=cfg)
        assert torch.equal(y, _wide(xg[:M], c["packed"], c["scale"], bias, N, cfg=cfg))   # no atomics: the same bits
        ref, mag = ref_all[:M], mag_all[:M]
        if bias is not None:
            ref, mag = ref + c["b64"], mag + c["b64"].abs()
        ratio, over = _bound_ratio(y.cpu(), ref, mag, K)
        worst = max(worst, ratio)
        assert over <= 0, (K, N, M, bias is not None, cfg, ratio)

    for M in _ROWS:
        check(M, None, 0)
        check(M, c["bias"], 0)
    for cfg in _CFGS:
        check(47, c["bias"], cfg)
    print(f"mx_gemm_wide K={K} N={N}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("K", [32, 96])
def test_mx_gemm_wide_guards(K):
    """x is the first M rows of a taller tensor whose other rows and side columns are NaN, y the first M
    rows of a taller tensor holding a sentinel: neither the K tail nor the rows past M may read garbage
    into the tile or store."""
    from test_mxfp4_gpu import _case
    from test_mxfp4_mfma_gpu import _bound_ratio
    from test_mxfp4_moe_gpu import _x

    N = 40
    c = _case(K, N)
    xg = _x(70, K, 5 * K)
    x64 = xg.cpu().double()
    for M in (17, 33, 70):
        tall = torch.full((M + 20, K + 64), float("nan"), dtype=torch.bfloat16, device="cuda")
        tall[:M, 32:32 + K] = xg[:M]
        ybuf = torch.full((M + 20, N), _SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        from neuronx_distributed_llama3_2_amd.ops import ext

        ext().mx_gemm_wide(tall[:M, 32:32 + K], c["packed"], c["scale"], None, ybuf[:M], False)
        assert bool((ybuf[M:].view(torch.int16) == _SENTINEL).all()), (K, M)
        ratio, over = _bound_ratio(ybuf[:M].cpu(), x64[:M] @ c["wd"].t(), x64[:M].abs() @ c["wd"].abs().t(), K)
        assert over <= 0, (K, M, ratio)


@pytest.mark.parametrize("K,N", [(32, _WIDE), (2080, 5), (4096, 1536)])
def test_mx_gemm_wide_glu(K, N):
    """Fused SwiGLU ([gate; up] rows): through __expf, so the tolerance of test_mx_gemm_glu."""
    from test_mxfp4_gpu import _case
    from test_mxfp4_moe_gpu import _x

    c = _case(K, N, glu=True)
    xg = _x(129, K, 7 * K + N)
    full = xg.cpu().double() @ c["wd"].t()
    for M in (17, 64, 129):
        for bias in (None, c["bias"]):
            f = full[:M] + (c["b64"] if bias is not None else 0.0)
            ref = (torch.nn.functional.silu(f[:, :N]) * f[:, N:]).float()
            for cfg in [0] + (_CFGS if M == 17 and bias is not None else []):
                y = _wide(xg[:M], c["packed"], c["scale"], bias, N, glu=True, cfg=cfg)
                assert torch.equal(y, _wide(xg[:M], c["packed"], c["scale"], bias, N, glu=True, cfg=cfg))
                torch.testing.assert_close(y.cpu().float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)


def test_mx_linear_routes_to_the_wide_kernel(monkeypatch):
    """Up to the knob mx_linear gives the bits of mx_gemm_wide; past it, or with the knob at 0, those
    of dequantise + GEMM."""
    from test_mxfp4_gpu import _case
    from test_mxfp4_moe_gpu import _x

    from neuronx_distributed_llama3_2_amd.ops import gemv
    from neuronx_distributed_llama3_2_amd.ops.gemm import linear

    K, N = 2080, 40
    c = _case(K, N)
    x = _x(65, K, 13)
    wd = gemv.dequantize_mxfp4(c["packed"], c["scale"], torch.bfloat16)
    monkeypatch.setattr(gemv, "_MX_WIDE", 64)
    assert torch.equal(gemv.mx_linear(x[:24], c["packed"], c["scale"], c["bias"]),
                       _wide(x[:24], c["packed"], c["scale"], c["bias"], N))
    assert torch.equal(gemv.mx_linear(x, c["packed"], c["scale"], c["bias"]), linear(x, wd, c["bias"]))
    monkeypatch.setattr(gemv, "_MX_WIDE", 0)
    assert torch.equal(gemv.mx_linear(x[:24], c["packed"], c["scale"], c["bias"]), linear(x[:24], wd, c["bias"]))


def test_mxfp4_llama_batch24_decode_on_gpu(monkeypatch):
    """The tiny Llama of test_mxfp4_llama_batch12_decode_on_gpu at batch 24 with every decode projection
    on mx_gemm_wide: hipGraph and eager decode give the same 8 greedy tokens, one decode step stays
    within 0.05 (max-abs difference / max-abs logit) of the bf16 model holding the dequantized weights."""
    from test_inference_gpu import _cfg
    from test_mxfp4 import _fake_quantized_sd
    from transformers import LlamaForCausalLM as HF

    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd
    from neuronx_distributed_llama3_2_amd.ops import gemv

    B = 24
    monkeypatch.setattr(gemv, "_MX_WIDE", 64)
    assert gemv.mx_route(B) == "dequant" and gemv.mx_wide_ok(B)
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
