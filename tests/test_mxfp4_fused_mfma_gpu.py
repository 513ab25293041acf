"""Fused decode launches over MXFP4 weights at 4-16 rows on MI355X (csrc/decode_fused_mx_mfma.hip behind
_C.dgemv_mx, ops.gemv.mx_decode_linear, the 4-8 row gate of a quantized Llama) against fp64 of the dequantized
weights rounded where tests/decode_refs.py says dgemv rounds.  The integer cases are test_mxfp4_fused_gpu's
construction at 16 rows (every fp32 partial sum exact in any order, so PLAIN / RESID must match bit for bit; GLU goes
through __expf and takes test_mx_gemv_glu's tolerance); every output is that file's NaN-sentinel-framed view."""

import pytest
import torch

from test_mxfp4_fused_gpu import GLU, PLAIN, RESID, _check, _gemv, _run
from test_mxfp4_gpu import _random_mx

pytestmark = pytest.mark.gpu

EPIS = pytest.mark.parametrize("epi", [PLAIN, RESID, GLU], ids=["plain_norm", "resid", "glu_norm"])
_REFS = {}


def _case(kind, epi, K, N):
    """GPU operands for 16 rows, the fp64 accumulators acc [16, Nw] and sum |a w| [16, Nw], built once per shape."""
    key = (kind, epi, K, N)
    if key in _REFS:
        return _REFS[key]
    ops = _gemv()
    Nw = 2 * N if epi == GLU else N
    g = torch.Generator().manual_seed(K * 37 + N * 5 + epi + (kind == "int") * 1000)
    if kind == "int":
        codes = torch.randint(0, 16, (Nw, K // 2, 2), generator=g, dtype=torch.uint8)
        packed = (codes[..., 0] | (codes[..., 1] << 4)).contiguous()
        scale = torch.randint(125, 130, (Nw, K // 32), generator=g, dtype=torch.uint8)
        sign = 2.0 * torch.randint(0, 2, (16, K), generator=g) - 1
        nw = torch.randint(1, 4, (K,), generator=g).float()
        if epi == RESID:
            x, a = torch.randint(-2, 3, (16, K), generator=g).float(), None
        else:
            x = sign * 2.0 ** torch.tensor([-2.0, 1.0, 3.0]).repeat(6)[:16, None]
            a = sign.double() * nw.double()              # the normalised row, exactly
        y0, eps = torch.randint(-8, 9, (16, N), generator=g).float(), 2.0 ** -20
    else:
        packed, scale = _random_mx(Nw, K, K + N, 121, 127)
        x, nw, y0 = torch.randn(16, K, generator=g), 1 + 0.1 * torch.randn(K, generator=g), torch.randn(16, N, generator=g)
        eps, a = 1e-5, None
    xw = torch.zeros(16, K + 64)
    xw[:, 32:32 + K] = x
    xw, nw, y0 = xw.to(torch.bfloat16), nw.to(torch.bfloat16), y0.to(torch.bfloat16)
    if a is None:
        a = xw[:, 32:32 + K].double()
        if epi != RESID:
            n64 = a * torch.rsqrt(a.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
            a = (n64 * nw.double()).float().to(torch.bfloat16).double()
    wd = ops.dequantize_mxfp4(packed, scale, torch.float32).double()
    _REFS[key] = dict(packed=packed.cuda(), scale=scale.cuda(), xw=xw.cuda(), nw=nw.cuda(), y0=y0, eps=eps, acc=a @ wd.t(),
                      mag=a.abs() @ wd.abs().t())
    return _REFS[key]


def _check_bound(c, epi, K, N, M, y, what):
    """Per element within 2^-8 |ref| + K 2^-24 sum |a w| of fp64 (RESID: once more at its second rounding)."""
    if epi == GLU:
        return _check(c, epi, N, M, y, False, what)
    acc, tol = c["acc"][:M], 2.0 ** -8 * c["acc"][:M].abs() + K * 2.0 ** -24 * c["mag"][:M]
    if epi == RESID:
        acc = c["y0"][:M].double() + acc
        tol = tol + 2.0 ** -8 * acc.abs()
    err = (y.double() - acc).abs()
    assert bool(torch.isfinite(y).all()) and bool((err <= tol).all()), f"{what}: worst {float((err - tol).max())} over the bound"


@pytest.mark.parametrize("M", [4, 5, 8, 9, 13, 16])
@pytest.mark.parametrize("K", [32, 96, 2080, 4128])
@EPIS
def test_dgemv_mx_mfma_integer_cases(epi, K, M):
    """Every T x KS instantiation (cfg = 16 T + KS) and the launcher's choice.  K = 32: three idle lane groups and
    empty k-slices; 96: one idle group; 2080: 65 blocks, no multiple of 4 or of a split; 4128: more than one slab in
    every split, a second scale dword."""
    cfgs = [0] + [16 * t + ks for t in ((1, 2) if epi == GLU else (1, 2, 4)) for ks in (1, 2, 4)]
    for N in (1, 5, 12 if epi == GLU else 17, 259):
        c = _case("int", epi, K, N)
        for cfg in cfgs:
            _check(c, epi, N, M, _run(c, epi, K, N, M, cfg), True, f"N={N} cfg={cfg}")


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("K", [2080, 4128])
@EPIS
def test_dgemv_mx_mfma_random_cases(epi, K, M):
    """Random codes and scales 2^-6..1 against fp64 within the project's bound; two calls give the same bits."""
    c = _case("rand", epi, K, 130)
    y = _run(c, epi, K, 130, M, 0)
    _check_bound(c, epi, K, 130, M, y, f"random K={K} M={M}")
    assert torch.equal(y, _run(c, epi, K, 130, M, 0))


@pytest.mark.parametrize("M", [5, 13])
@pytest.mark.parametrize("K", [32, 96])
@EPIS
def test_dgemv_mx_mfma_ignores_rows_past_m(epi, K, M):
    """x is the first M rows of a taller tensor whose other rows are NaN: nothing of them reaches the output."""
    c = dict(_case("rand", epi, K, 17))
    c["xw"] = c["xw"].clone()
    c["xw"][M:] = float("nan")
    _check_bound(c, epi, K, 17, M, _run(c, epi, K, 17, M, 0), f"row guard K={K} M={M}")


def test_mx_decode_linear_routes_by_the_rows_knob(monkeypatch):
    """At 6 rows: under the knob at 16 the op's three forms give the direct call's bits (the residual updated in place
    and returned), under the knob at 3 those of the composed route."""
    from neuronx_distributed_llama3_2_amd.ops import rms_norm

    ops = _gemv()
    K, N, M = 2080, 17, 6
    for knob in (16, 3):
        monkeypatch.setattr(ops, "_FUSED_MX_ROWS", knob)
        for epi in (RESID, PLAIN, GLU):
            c = _case("int", epi, K, N)
            x, w = c["xw"][:M, 32:32 + K], (c["packed"], c["scale"])
            if epi == RESID:
                res = c["y0"][:M].cuda()
                out = ops.mx_decode_linear(x, *w, residual=res)
                assert out is res
            else:
                out = ops.mx_decode_linear(x, *w, norm_weight=c["nw"], eps=c["eps"], glu=epi == GLU)
            if knob == 16:
                want = _run(c, epi, K, N, M, 0).cuda()
            elif epi == RESID:
                want = c["y0"][:M].cuda() + ops.mx_linear(x, *w)
            else:
                want = ops.mx_linear(rms_norm(x, c["nw"], c["eps"])[0], *w, glu=epi == GLU)
            assert out.shape == (M, N) and torch.equal(out, want), (knob, epi)


@pytest.mark.parametrize("B", [4, 8])
def test_mxfp4_model_decodes_on_fused_launches_at_4_to_8_rows(monkeypatch, B):
    """test_mxfp4_model_decodes_on_fused_launches at batch 4 and 8 with the rows knob at 16: the new gate is open and
    _decode_fusable_mx still shut, eager and hipGraph decode agree, a step is within 0.05 of the bf16 model holding
    the dequantized weights; with the knob at 3 the step is the unfused one bit for bit."""
    from test_inference_gpu import _cfg
    from test_mxfp4 import _fake_quantized_sd
    from transformers import LlamaForCausalLM as HF

    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    ops = _gemv()
    monkeypatch.setenv("NXD_DECODE_FUSED_MX", "1")
    monkeypatch.setenv("NXD_DECODE_FUSED_MX_ROWS", "16")
    cfg = _cfg()
    torch.manual_seed(0)
    sd = {k: v.detach().to(torch.bfloat16) for k, v in HF(cfg).state_dict().items()}

    def model(sd_, graphs, steps, **kw):
        icfg = InferenceConfig(batch_size=B, seq_len=256, max_context_length=128, use_hip_graphs=graphs,
                               decode_graph_steps=steps, **kw)
        m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, device=torch.device("cuda"), init_weights=False)
        m._load_full(hf_to_nxd(sd_, cfg))
        return m

    g = model(sd, True, 8, quantized=True, quantization_type="mxfp4")
    e = model(sd, False, 1, quantized=True, quantization_type="mxfp4")
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (B, 40))
    a = g.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    assert a.shape == (B, 48) and torch.equal(a, b), (a[:, 40:], b[:, 40:])
    last = b[:, -1:].cuda()
    for m in (g, e):
        assert m.model._decode_fusable_mx_rows(last) is True and m.model._decode_fusable_mx(last) is False
    assert e.model._decode_fusable_mx_rows(torch.cat([last, last[:1]], 0)) is (B == 4)   # 5 rows open, 9 shut

    f = model(_fake_quantized_sd(sd), False, 1)
    emb = f.model.model.embed_tokens.weight
    f.model.lm_head.weight = torch.nn.Parameter(ops.dequantize_mxfp4(*ops.quantize_mxfp4(emb), torch.bfloat16),
                                                requires_grad=False)
    f.model._decode_fused_ok = False
    f.generate(ids, max_new_tokens=8, eos_token_id=-1)
    f.model.kv_cache.copy_(e.model.kv_cache)
    pos = torch.full((B, 1), b.shape[1] - 1, dtype=torch.int64, device="cuda")
    sid = torch.arange(B, device="cuda")
    clen = torch.full((B,), b.shape[1], dtype=torch.int32, device="cuda")
    dq = e.model.forward_tokens(last, pos, sid, clen).float()
    df = f.model.forward_tokens(last, pos, sid, clen).float()
    dec = float((dq - df).abs().max() / df.abs().max())
    print(f"fused mxfp4 decode step at {B} rows vs fake-quantized bf16 model: {dec:.4f}")
    assert dec < 0.05, dec

    monkeypatch.setenv("NXD_DECODE_FUSED_MX_ROWS", "3")
    e.model._decode_fused_mx_ok = None
    assert e.model._decode_fusable_mx_rows(last) is False
    d0 = e.model.forward_tokens(last, pos, sid, clen)
    e.set_fused_decode(False)
    assert torch.equal(d0, e.model.forward_tokens(last, pos, sid, clen))
