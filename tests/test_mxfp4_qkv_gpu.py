"""The MXFP4 fused QKV decode launch on MI355X (_C.dgemv_mx with epi = 3: csrc/decode_fused_mx.hip at 1-3 rows,
csrc/decode_fused_mx_mfma.hip at 4-16; ops.gemv.mx_decode_qkv; the quantized tiny Llama) per element against fp64 that
rounds where tests/decode_refs.py::dgemv_ref rounds.  Integer cases are exact: x = +-2^r per row normalises to exactly
+-w_norm, codes times scales 2^-2..2^2 are multiples of 2^-3 up to 24, so every fp32 partial sum is an exact multiple
of 2^-3 below 2^20 in any order; bf16 of it, times a cos / sin from {0, +-0.5, +-1}, is a multiple of 2^-4 below 2^19,
so both rotation terms and their sum are exact in fp32 (fused or not).  _case asserts that the fp64 values fit fp32 at
both points.  y and both caches are views of NaN-sentinel buffers."""

import pytest
import torch

from test_mxfp4_gpu import _random_mx

pytestmark = pytest.mark.gpu

SENT = 0x7FA5                       # a quiet-NaN bf16 bit pattern
LMAX, P = 6, 5                      # cache length; table rows (position 5 is cached and clamped to table row 4)
POS = [3, -1, 7, 5, 0, 2, 4, 1]     # row m: POS[m % 8]; -1 and 7 stay out of the caches
HEADS = [(4, 2, 64), (2, 1, 128), (2, 1, 8)]
_REFS = {}


def _case(kind, K, heads):
    """GPU operands for 16 rows and the fp64 normalised rows a [16, K] and weight w [N, K], once per shape."""
    key = (kind, K, heads)
    if key in _REFS:
        return _REFS[key]
    from neuronx_distributed_llama3_2_amd.ops import ext, gemv as ops

    ext()
    nq, nkv, D = heads
    N = (nq + 2 * nkv) * D
    g = torch.Generator().manual_seed(K * 31 + N * 7 + D + (kind == "int") * 1000)
    if kind == "int":
        codes = torch.randint(0, 16, (N, K // 2, 2), generator=g, dtype=torch.uint8)
        packed = (codes[..., 0] | (codes[..., 1] << 4)).contiguous()
        scale = torch.randint(125, 130, (N, K // 32), generator=g, dtype=torch.uint8)
        sign = 2.0 * torch.randint(0, 2, (16, K), generator=g) - 1
        nw = torch.randint(1, 4, (K,), generator=g).float()
        x = sign * 2.0 ** torch.tensor([-2.0, 1.0, 3.0]).repeat(6)[:16, None]
        a = sign.double() * nw.double()              # the normalised row, exactly
        cos, sin = (torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0])[torch.randint(0, 5, (P, D // 2), generator=g)] for _ in "cs")
        eps = 2.0 ** -20
    else:
        packed, scale = _random_mx(N, K, K + N, 121, 127)
        x = torch.randn(16, K, generator=g)
        nw = 1 + 0.1 * torch.randn(K, generator=g)
        ang = 6.28 * torch.rand(P, D // 2, generator=g)
        cos, sin, eps, a = ang.cos(), ang.sin(), 1e-5, None
    xw = torch.zeros(16, K + 64)
    xw[:, 32:32 + K] = x
    xw, nw = xw.to(torch.bfloat16), nw.to(torch.bfloat16)
    if a is None:
        a = xw[:, 32:32 + K].double()
        n64 = a * torch.rsqrt(a.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
        a = (n64 * nw.double()).float().to(torch.bfloat16).double()
    w = ops.dequantize_mxfp4(packed, scale, torch.float32).double()
    _REFS[key] = dict(packed=packed.cuda(), scale=scale.cuda(), xw=xw.cuda(), nw=nw.cuda(), eps=eps, a=a, w=w, kind=kind,
                      cos=cos.cuda(), sin=sin.cuda(), cos64=cos.double(), sin64=sin.double(), heads=heads, K=K)
    return _REFS[key]


def _operands(M, T):
    """Positions of the M rows, sequences, and the cache row B - 1 - b of sequence b."""
    return torch.tensor([POS[m % 8] for m in range(M)]), M // T, torch.arange(M // T - 1, -1, -1, dtype=torch.int32)


def _ref(c, a, pos, T, cidx):
    """(y [M, N] bf16, k cache, v cache as [B, nkv, LMAX, D] bf16 with NaN sentinels where nothing is written)."""
    nq, nkv, D = c["heads"]
    M, h = a.shape[0], D // 2
    acc = a @ c["w"].t()
    if c["kind"] == "int":
        assert torch.equal(acc.float().double(), acc)
    p = acc.float().to(torch.bfloat16).double().view(M, nq + 2 * nkv, D)
    pt = pos.clamp(0, P - 1)
    cs, sn = c["cos64"][pt][:, None], c["sin64"][pt][:, None]
    x1, x2 = p[:, :nq + nkv, :h], p[:, :nq + nkv, h:]
    rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    if c["kind"] == "int":
        assert torch.equal(rot.float().double(), rot)
    y = torch.cat([rot, p[:, nq + nkv:]], 1).float()
    yb = y.to(torch.bfloat16)
    caches = torch.full((2, M // T, nkv, LMAX, D), SENT, dtype=torch.int16).view(torch.bfloat16)
    for m in range(M):
        if 0 <= int(pos[m]) < LMAX:
            caches[0, int(cidx[m // T]), :, int(pos[m])] = yb[m, nq:nq + nkv]
            caches[1, int(cidx[m // T]), :, int(pos[m])] = yb[m, nq + nkv:]
    return y.view(M, -1), yb.view(M, -1), caches[0], caches[1]


def _framed(shape, pad=True):
    """A NaN-sentinel buffer one larger than `shape` in every dim but the head one (3 wider), and its view."""
    big = [s + pad for s in shape[:-1]] + [shape[-1] + 3 * pad]
    if len(shape) == 4:
        big[1] = shape[1]   # caches [B, nkv, LMAX, D]: the binding wants size(1) == nkv
    buf = torch.full(big, SENT, dtype=torch.int16).view(torch.bfloat16).cuda()
    return buf, buf[tuple(slice(0, s) for s in shape)]


def _run(c, M, T, cfg, xidx=None, op=None, pos=None):
    """One dgemv_mx(3) call (or op: mx_decode_qkv) into sentinel-framed y / caches; checks the frames; returns
    (y, kc, vc[, xcopy]) on the CPU."""
    from neuronx_distributed_llama3_2_amd.ops import ext

    nq, nkv, D = c["heads"]
    K, N = c["K"], (nq + 2 * nkv) * D
    p0, B, cidx = _operands(M, T)
    pos = (p0 if pos is None else pos).cuda()
    pad = D != 8 or op is None   # the composed route's ops.kv_cache_write takes contiguous caches
    (yb, y), (kb, kc), (vb, vc) = _framed((M, N)), _framed((B, nkv, LMAX, D), pad), _framed((B, nkv, LMAX, D), pad)
    frames = [t.cpu().clone() for t in (yb, kb, vb)]
    x = c["xw"][:, 32:32 + K]
    kw = dict(xidx=xidx.cuda(), xcopy=torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")) if xidx is not None else {}
    if op is not None:
        y.copy_(op(x[:M], c["packed"], c["scale"], c["nw"], c["eps"], nq, nkv, D, c["cos"], c["sin"], pos, T, kc, vc, cidx.cuda()))
    else:
        ext().dgemv_mx(3, x if xidx is not None else x[:M], c["nw"], c["eps"], c["packed"], c["scale"], y, cfg, nq=nq, nkv=nkv,
                       D=D, cos_t=c["cos"], sin_t=c["sin"], pos=pos, T=T, kc=kc, vc=vc, cache_idx=cidx.cuda(), **kw)
    outs = []
    for buf, view, frame in zip((yb, kb, vb), (y, kc, vc), frames):
        got = buf.cpu()
        idx = tuple(slice(0, s) for s in view.shape)
        outs.append(got[idx].clone())
        got[idx] = frame[idx]
        assert torch.equal(got.view(torch.int16), frame.view(torch.int16)), "sentinel around an output changed"
    return outs + ([kw["xcopy"].cpu()] if kw else [])


def _same(got, want, what):
    for g, w, name in zip(got, want, ("y", "k cache", "v cache")):
        assert torch.equal(g.contiguous().view(torch.int16), w.contiguous().view(torch.int16)), f"{what}: {name}"


@pytest.mark.parametrize("K", [32, 2080, 4128])
@pytest.mark.parametrize("heads,M", [(h, M) for h in HEADS for M in (1, 2, 3, 4, 7, 16) if h[2] != 8 or M <= 3],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_dgemv_mx_qkv_integer_cases(heads, M, K):
    """cfg = 0 and every R x KS (1-3 rows) / T x KS (4-16 rows) the launcher admits; T = 2 tokens per sequence where M is
    even; permuted cache rows; positions -1 and 7 (M >= 3) reach y and stay out of the caches.  D = 8 at 1-3 rows only:
    the 4-16 row kernel needs (D / 2) % 16 == 0 (test_mx_decode_qkv_on_gpu)."""
    c = _case("int", K, heads)
    T = 2 if M % 2 == 0 else 1
    pos, B, cidx = _operands(M, T)
    want = _ref(c, c["a"][:M], pos, T, cidx)[1:]
    for cfg in [0] + [16 * r + ks for r in (1, 2) for ks in (1, 2, 4)]:
        _same(_run(c, M, T, cfg), want, f"cfg={cfg}")


@pytest.mark.parametrize("M", [3, 5])
def test_dgemv_mx_qkv_embedding_gather(M):
    """xidx: row m is table row xidx[m], zeros for an id outside the table; xcopy receives the gathered rows."""
    c = _case("int", 2080, HEADS[0])
    xidx = torch.tensor([5, 0, 16, -1, 9][:M], dtype=torch.int64)
    ok = ((xidx >= 0) & (xidx < 16))[:, None]
    pos, B, cidx = _operands(M, 1)
    want = _ref(c, c["a"][xidx.clamp(0, 15)] * ok, pos, 1, cidx)[1:]
    got = _run(c, M, 1, 0, xidx=xidx)
    _same(got[:3], want, "xidx")
    assert torch.equal(got[3], (c["xw"][:, 32:32 + 2080].cpu()[xidx.clamp(0, 15)] * ok).to(torch.bfloat16))


@pytest.mark.parametrize("M", [3, 16])
def test_dgemv_mx_qkv_random_cases(M):
    """Random codes, scales 2^-6..1 and real cos / sin: test_dgemv_mx_random_cases' tolerance; two calls, the same bits."""
    c = _case("rand", 2080, HEADS[0])
    pos, B, cidx = _operands(M, 1)
    ref = _ref(c, c["a"][:M], pos, 1, cidx)[0]
    got = _run(c, M, 1, 0)
    torch.testing.assert_close(got[0].float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)
    written = got[1].contiguous().view(torch.int16) != SENT
    assert int(written.sum()) == sum(0 <= POS[m % 8] < LMAX for m in range(M)) * HEADS[0][1] * HEADS[0][2]
    _same(_run(c, M, 1, 0), got, "second call")


def test_mx_decode_qkv_on_gpu():
    """The op gives the direct call's bits at 2 and 6 rows; at D = 8 with 4 rows the direct call refuses and the op
    composes the unfused route, which rounds at the same points (exact on the integer case).  The composed cache write
    takes a sequence's positions as consecutive: rows (3, 4) and (0, 1)."""
    from neuronx_distributed_llama3_2_amd.ops.gemv import mx_decode_qkv

    c = _case("int", 2080, HEADS[0])
    for M in (2, 6):
        _same(_run(c, M, 2, 0, op=mx_decode_qkv), _run(c, M, 2, 0), f"M={M}")
    c = _case("int", 2080, HEADS[2])
    pos = torch.tensor([3, 4, 0, 1])
    want = _ref(c, c["a"][:4], pos, 2, _operands(4, 2)[2])[1:]
    _same(_run(c, 4, 2, 0, op=mx_decode_qkv, pos=pos), want, "composed")
    with pytest.raises(RuntimeError):
        _run(c, 4, 2, 0)


@pytest.mark.parametrize("batch", [1, 12])
def test_quantize_qkv_model_decodes_on_gpu(batch, monkeypatch):
    """The tiny Llama with a packed QKV: hipGraph and eager decode agree on 8 tokens (12 rows: only the packed QKV
    opens the fused gate there); a fused decode step is within test_mxfp4_fused_gpu's 0.05 of the unfused route."""
    from test_inference_gpu import _cfg
    from transformers import LlamaForCausalLM as HF

    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    monkeypatch.setenv("NXD_DECODE_FUSED_MX", "1")
    monkeypatch.setenv("NXD_DECODE_FUSED_MX_ROWS", "16")
    cfg = _cfg()
    torch.manual_seed(0)
    sd = {k: v.detach().to(torch.bfloat16) for k, v in HF(cfg).state_dict().items()}

    def model(graphs, steps):
        icfg = InferenceConfig(batch_size=batch, seq_len=256, max_context_length=128, use_hip_graphs=graphs,
                               decode_graph_steps=steps, quantized=True, quantization_type="mxfp4", quantize_qkv=True)
        m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, device=torch.device("cuda"), init_weights=False)
        m._load_full(hf_to_nxd(sd, cfg))
        return m

    g, e = model(True, 8), model(False, 1)
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (batch, 40))
    a = g.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    assert a.shape == (batch, 48) and torch.equal(a, b), (a[:, 40:], b[:, 40:])
    last = b[:, -1:].cuda()
    gate = e.model._decode_fusable_mx if batch <= 3 else e.model._decode_fusable_mx_rows
    assert gate(last) is True and e.model._decode_fused_mx_qkv is True
    pos = torch.full((batch, 1), b.shape[1] - 1, dtype=torch.int64, device="cuda")
    sid = torch.arange(batch, device="cuda")
    clen = torch.full((batch,), b.shape[1], dtype=torch.int32, device="cuda")
    fused = e.model.forward_tokens(last, pos, sid, clen).float()
    e.set_fused_decode(False)
    unfused = e.model.forward_tokens(last, pos, sid, clen).float()
    dec = float((fused - unfused).abs().max() / unfused.abs().max())
    print(f"fused mxfp4 decode step with packed QKV vs unfused, batch {batch}: {dec:.4f}")
    assert dec < 0.05, dec
