"""Fused decode GEMVs over MXFP4 weights on MI355X (csrc/decode_fused_mx.hip: _C.dgemv_mx, ops.gemv.mx_decode_linear)
against fp64 of the dequantized weights, rounded where tests/decode_refs.py says dgemv rounds, and a quantized tiny
Llama decoding on them.  Integer cases are exact: x = +-2^r per row normalises to exactly +-w_norm (decode_refs.py,
kind "int"), codes times scales 2^-2..2^2 are multiples of 2^-3 up to 24, so every term is a multiple of 2^-4 and
sum |a w| <= 72 K < 2^20 for K <= 4128: every fp32 partial sum is exact in any order.  GLU goes through __expf and
takes test_mx_gemv_glu's tolerance.  Every output is a view (one more row, ld = N + 3) of a buffer of NaN sentinels."""

import pytest
import torch

from test_mxfp4_gpu import _random_mx

pytestmark = pytest.mark.gpu

PLAIN, RESID, GLU = 0, 1, 2
SENT = 0x7FA5          # a quiet-NaN bf16 bit pattern
N_BIG = 259            # 64 four-row waves and a ragged 65th, 17 workgroups
_REFS = {}


def _gemv():
    from neuronx_distributed_llama3_2_amd.ops import ext, gemv

    ext()
    return gemv


def _case(kind, epi, K, N):
    """GPU operands for three rows and the fp64 accumulators [3, Nw], built once per shape."""
    key = (kind, epi, K, N)
    if key in _REFS:
        return _REFS[key]
    ops = _gemv()
    Nw = 2 * N if epi == GLU else N
    g = torch.Generator().manual_seed(K * 31 + N * 7 + epi + (kind == "int") * 1000)
    if kind == "int":
        codes = torch.randint(0, 16, (Nw, K // 2, 2), generator=g, dtype=torch.uint8)
        packed = (codes[..., 0] | (codes[..., 1] << 4)).contiguous()
        scale = torch.randint(125, 130, (Nw, K // 32), generator=g, dtype=torch.uint8)
        sign = 2.0 * torch.randint(0, 2, (3, K), generator=g) - 1
        nw = torch.randint(1, 4, (K,), generator=g).float()
        if epi == RESID:
            x, a = torch.randint(-2, 3, (3, K), generator=g).float(), None
        else:
            x = sign * 2.0 ** torch.tensor([[-2.0], [1.0], [3.0]])
            a = sign.double() * nw.double()              # the normalised row, exactly
        y0 = torch.randint(-8, 9, (3, N), generator=g).float()
        eps = 2.0 ** -20
    else:
        packed, scale = _random_mx(Nw, K, K + N, 121, 127)
        x = torch.randn(3, K, generator=g)
        nw = 1 + 0.1 * torch.randn(K, generator=g)
        y0 = torch.randn(3, N, generator=g)
        eps, a = 1e-5, None
    xw = torch.zeros(3, K + 64)
    xw[:, 32:32 + K] = x
    xw, nw, y0 = xw.to(torch.bfloat16), nw.to(torch.bfloat16), y0.to(torch.bfloat16)
    if a is None:
        a = xw[:, 32:32 + K].double()
        if epi != RESID:
            n64 = a * torch.rsqrt(a.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
            a = (n64 * nw.double()).float().to(torch.bfloat16).double()
    acc = a @ ops.dequantize_mxfp4(packed, scale, torch.float32).double().t()
    _REFS[key] = dict(packed=packed.cuda(), scale=scale.cuda(), xw=xw.cuda(), nw=nw.cuda(), y0=y0, eps=eps, acc=acc)
    return _REFS[key]


def _run(c, epi, K, N, M, cfg):
    """One dgemv_mx call into a sentinel-framed view; returns y [M, N] on the CPU after checking the frame."""
    from neuronx_distributed_llama3_2_amd.ops import ext

    buf = torch.full((M + 1, N + 3), SENT, dtype=torch.int16).view(torch.bfloat16)
    if epi == RESID:
        buf[:M, :N] = c["y0"][:M]
    frame = buf.clone()
    buf = buf.cuda()
    x = c["xw"][:M, 32:32 + K]
    assert x.stride(0) != K
    ext().dgemv_mx(epi, x, None if epi == RESID else c["nw"], c["eps"], c["packed"], c["scale"], buf[:M, :N], cfg)
    got = buf.cpu()
    frame[:M, :N] = got[:M, :N]
    assert torch.equal(got.view(torch.int16), frame.view(torch.int16)), "sentinel around the output changed"
    return got[:M, :N]


def _check(c, epi, N, M, y, exact, what):
    acc = c["acc"][:M]
    if epi == GLU:
        ref = (torch.nn.functional.silu(acc[:, :N]) * acc[:, N:]).float()
    elif epi == RESID:
        ref = c["y0"][:M].float() + (acc.float().to(torch.bfloat16).float() if exact else acc.float())
    else:
        ref = acc.float()
    if exact and epi != GLU:
        assert torch.equal(y, ref.to(torch.bfloat16)), what
    else:
        torch.testing.assert_close(y.float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("K", [32, 2080, 4128])
@pytest.mark.parametrize("epi", [PLAIN, RESID, GLU], ids=["plain_norm", "resid", "glu_norm"])
def test_dgemv_mx_integer_cases(epi, K, M):
    """Every R x KS instantiation (cfg = 16 R + KS) and the launcher's choice (cfg = 0).  K = 32: one block, 63 idle
    lanes, empty k-slices; 2080: one block past a 64-block step; 4128: a third prologue trip, a second load round."""
    cfgs = [0] + [16 * r + ks for r in ((1, 2) if epi == GLU else (1, 2, 4)) for ks in (1, 2, 4)]
    for N in ((1, 5, 12) if epi == GLU else (1, 5, 17)) + (N_BIG,):
        c = _case("int", epi, K, N)
        for cfg in cfgs:
            _check(c, epi, N, M, _run(c, epi, K, N, M, cfg), True, f"N={N} cfg={cfg}")


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("K", [2080, 4128])
@pytest.mark.parametrize("epi", [PLAIN, RESID, GLU], ids=["plain_norm", "resid", "glu_norm"])
def test_dgemv_mx_random_cases(epi, K, M):
    """Random codes and scales 2^-6..1: test_mx_gemv_glu's tolerance against fp64; two calls give the same bits."""
    N = 130
    c = _case("rand", epi, K, N)
    y = _run(c, epi, K, N, M, 0)
    _check(c, epi, N, M, y, False, f"random K={K} M={M}")
    assert torch.equal(y, _run(c, epi, K, N, M, 0))


def test_mx_decode_linear_on_gpu():
    """The op's three forms give the direct call's bits; the residual is updated in place and returned."""
    ops = _gemv()
    K, N, M = 2080, 17, 2
    c = _case("int", RESID, K, N)
    x = c["xw"][:M, 32:32 + K]
    res = c["y0"][:M].cuda()
    out = ops.mx_decode_linear(x, c["packed"], c["scale"], residual=res)
    assert out is res and torch.equal(res.cpu(), _run(c, RESID, K, N, M, 0))
    for epi, glu in ((PLAIN, False), (GLU, True)):
        c = _case("int", epi, K, N)
        y = ops.mx_decode_linear(c["xw"][:M, 32:32 + K], c["packed"], c["scale"], norm_weight=c["nw"], eps=c["eps"], glu=glu)
        assert y.shape == (M, N) and torch.equal(y.cpu(), _run(c, epi, K, N, M, 0))


def test_mxfp4_model_decodes_on_fused_launches(monkeypatch):
    """The tiny Llama of test_mxfp4_model_decode_on_gpu with the knob on: the MXFP4 gate opens, _check_decode_fusable
    stays False, eager and hipGraph decode agree, a step is within that test's 0.05 of the bf16 model holding the
    dequantized weights; with the knob at 0 the step is the unfused one bit for bit."""
    from test_inference_gpu import _cfg
    from test_mxfp4 import _fake_quantized_sd
    from transformers import LlamaForCausalLM as HF

    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    ops = _gemv()
    monkeypatch.setenv("NXD_DECODE_FUSED_MX", "1")
    cfg = _cfg()
    torch.manual_seed(0)
    sd = {k: v.detach().to(torch.bfloat16) for k, v in HF(cfg).state_dict().items()}

    def model(sd_, graphs, steps, **kw):
        icfg = InferenceConfig(batch_size=2, seq_len=256, max_context_length=128, use_hip_graphs=graphs,
                               decode_graph_steps=steps, **kw)
        m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, device=torch.device("cuda"), init_weights=False)
        m._load_full(hf_to_nxd(sd_, cfg))
        return m

    g = model(sd, True, 8, quantized=True, quantization_type="mxfp4")
    e = model(sd, False, 1, quantized=True, quantization_type="mxfp4")
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (2, 40))
    a = g.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    assert a.shape == (2, 48) and torch.equal(a, b), (a[:, 40:], b[:, 40:])
    last = b[:, -1:].cuda()
    for m in (g, e):
        assert m.model._decode_fusable_mx(last) is True and m.model._check_decode_fusable() is False
    assert e.model._decode_fusable_mx(torch.cat([last, last], 1)) is False   # four rows: the MFMA route's

    f = model(_fake_quantized_sd(sd), False, 1)
    emb = f.model.model.embed_tokens.weight
    f.model.lm_head.weight = torch.nn.Parameter(ops.dequantize_mxfp4(*ops.quantize_mxfp4(emb), torch.bfloat16),
                                                requires_grad=False)
    f.model._decode_fused_ok = False
    f.generate(ids, max_new_tokens=8, eos_token_id=-1)
    f.model.kv_cache.copy_(e.model.kv_cache)
    pos = torch.full((2, 1), b.shape[1] - 1, dtype=torch.int64, device="cuda")
    sid = torch.arange(2, device="cuda")
    clen = torch.full((2,), b.shape[1], dtype=torch.int32, device="cuda")
    dq = e.model.forward_tokens(last, pos, sid, clen).float()
    df = f.model.forward_tokens(last, pos, sid, clen).float()
    dec = float((dq - df).abs().max() / df.abs().max())
    print(f"fused mxfp4 decode step vs fake-quantized bf16 model: {dec:.4f}")
    assert dec < 0.05, dec

    monkeypatch.setenv("NXD_DECODE_FUSED_MX", "0")
    e.model._decode_fused_mx_ok = None
    assert e.model._decode_fusable_mx(last) is False
    d0 = e.model.forward_tokens(last, pos, sid, clen)
    e.set_fused_decode(False)
    assert torch.equal(d0, e.model.forward_tokens(last, pos, sid, clen))
