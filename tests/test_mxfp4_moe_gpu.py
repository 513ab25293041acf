"""MXFP4 MoE experts on MI355X (csrc/gemv_mx.hip expert kernel): the selective and the all-experts
forms per element against fp64 of the dequantized weights, their fall-backs, the MoE block with the
routing held fixed against the bf16 kernels, and a quantized tiny Mixtral decoding eagerly and from
a hipGraph.  The fp64 references are built on the GPU from the pure-torch dequantizer."""

import pytest
import torch

pytestmark = pytest.mark.gpu

_WIDE = 8192 + 3   # takes the several-rows-per-wave launch, with a ragged last wave


def _ops():
    from neuronx_distributed_llama3_2_amd.ops import gemv

    return gemv


def _stack(E, Nw, K, seed):
    """A random expert stack on the GPU, held as a slice of a larger buffer: rows are 16 bytes and
    experts one row + 48 bytes further apart than their contents, for codes and scales alike.
    Returns (packed [E, Nw, K/2], scale [E, Nw, K/32], fp64 dequantized [E, Nw, K])."""
    from test_mxfp4_gpu import _random_mx

    p, s = _random_mx(E * Nw, K, seed, 121, 127)
    ldw, lds = K // 2 + 16, K // 32 + 3
    pb = torch.zeros(E * ((Nw + 1) * ldw + 48), dtype=torch.uint8, device="cuda")
    sb = torch.zeros(E * ((Nw + 1) * lds + 5), dtype=torch.uint8, device="cuda")
    packed = pb.as_strided((E, Nw, K // 2), ((Nw + 1) * ldw + 48, ldw, 1))
    scale = sb.as_strided((E, Nw, K // 32), ((Nw + 1) * lds + 5, lds, 1))
    packed.copy_(p.view(E, Nw, K // 2))
    scale.copy_(s.view(E, Nw, K // 32))
    assert packed.stride(0) != Nw * packed.stride(1) and packed.stride(0) % 16 == 0 and packed.data_ptr() % 16 == 0
    return packed, scale, _ops()._dequantize_mxfp4_torch(packed, scale, torch.float64)


def _poisoned(packed, scale, keep):
    """A copy of the stack, same strides, whose experts outside `keep` hold 6 * 2^127 everywhere."""
    pp = torch.empty_strided(packed.shape, packed.stride(), dtype=torch.uint8, device="cuda")
    sp = torch.empty_strided(scale.shape, scale.stride(), dtype=torch.uint8, device="cuda")
    pp.copy_(packed)
    sp.copy_(scale)
    for e in range(packed.shape[0]):
        if e not in keep:
            pp[e].fill_(0x77)
            sp[e].fill_(254)
    return pp, sp


def _x(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    xw = torch.randn(rows, K + 64, generator=g).to(torch.bfloat16).cuda()
    x = xw[:, 32:32 + K]          # a column slice of a wider tensor: ldx != K
    assert x.stride(0) != K
    return x


def _check_bound(y, ref, mag, K, what):
    """|y - ref| <= 2^-8 |ref| + K 2^-24 sum_k |x_k w_k| for every element (test_mx_gemv_matches_fp64)."""
    assert bool(torch.isfinite(y).all()), what
    err = (y.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * mag
    print(f"{what}: max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert float((err - bound).max()) <= 0, what


_EIDX = {1: [1], 2: [2, 2], 6: [0, 2, 2, 0, 2, 0]}   # each with a repeated or an unused expert


@pytest.mark.parametrize("N", [1, 5, _WIDE])
@pytest.mark.parametrize("K", [32, 2080, 4096])
def test_mx_expert_gemv_matches_fp64(K, N):
    ops = _ops()
    from neuronx_distributed_llama3_2_amd.ops import ext

    rows = ext().mx_gemv_rows_per_wave(N, K)
    assert rows == ((4 if K <= 2048 else 2) if N == _WIDE else 1)
    E = 3
    packed, scale, wd = _stack(E, N, K, 3 * K + N)
    for P, idx in _EIDX.items():
        pp, sp = _poisoned(packed, scale, set(idx))
        eidx = torch.tensor(idx, dtype=torch.int32, device="cuda")
        for xdiv in (1, 2):
            x = _x((P + xdiv - 1) // xdiv, K, 11 * P + xdiv)
            y = ops.mx_expert_linear(x, pp, sp, eidx, xdiv=xdiv)
            assert y.shape == (P, N) and y.dtype == torch.bfloat16
            assert torch.equal(y, ops.mx_expert_linear(x, pp, sp, eidx, xdiv=xdiv))   # no atomics: equal bits
            xr = x.double()[torch.arange(P, device="cuda") // xdiv]
            w = wd[eidx.long()]
            ref = torch.einsum("pk,pnk->pn", xr, w)
            mag = torch.einsum("pk,pnk->pn", xr.abs(), w.abs())
            _check_bound(y, ref, mag, K, f"selective K={K} N={N} P={P} xdiv={xdiv}")


@pytest.mark.parametrize("K,N", [(32, _WIDE), (2080, 5), (4096, 1536)])
def test_mx_expert_gemv_glu(K, N):
    """Fused SwiGLU ([gate; up] rows n and n + N of the chosen expert): through __expf, so the tolerance
    of test_mx_gemv_glu."""
    ops = _ops()
    E = 3
    packed, scale, wd = _stack(E, 2 * N, K, 5 * K + N)
    for P, idx in _EIDX.items():
        pp, sp = _poisoned(packed, scale, set(idx))
        eidx = torch.tensor(idx, dtype=torch.int32, device="cuda")
        for xdiv in (1, 2):
            x = _x((P + xdiv - 1) // xdiv, K, 13 * P + xdiv)
            y = ops.mx_expert_linear(x, pp, sp, eidx, xdiv=xdiv, glu=True)
            assert y.shape == (P, N)
            assert torch.equal(y, ops.mx_expert_linear(x, pp, sp, eidx, xdiv=xdiv, glu=True))
            xr = x.double()[torch.arange(P, device="cuda") // xdiv]
            full = torch.einsum("pk,pnk->pn", xr, wd[eidx.long()])
            ref = (torch.nn.functional.silu(full[:, :N]) * full[:, N:]).float()
            torch.testing.assert_close(y.float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)


@pytest.mark.parametrize("K,N", [(32, _WIDE), (2080, 5), (4096, _WIDE)])
def test_mx_experts_gemv_matches_fp64(K, N):
    """All experts, M rows each (2: MM 2; 3: MM 4 with a masked row; 8: MM 8), x shared or per expert."""
    ops = _ops()
    E = 4
    packed, scale, wd = _stack(E, N, K, 7 * K + N)
    for M in (2, 3, 8):
        xs = _x(M, K, 17 * M)
        xp = _x(E * M, K, 19 * M).unflatten(0, (E, M))
        assert not xp.is_contiguous()
        for x, x64 in ((xs, xs.double().expand(E, M, K)), (xp, xp.double())):
            y = ops.mx_experts_linear(x, packed, scale)
            assert y.shape == (E, M, N) and y.dtype == torch.bfloat16
            assert torch.equal(y, ops.mx_experts_linear(x, packed, scale))
            ref = torch.einsum("emk,enk->emn", x64, wd)
            mag = torch.einsum("emk,enk->emn", x64.abs(), wd.abs())
            _check_bound(y, ref, mag, K, f"all experts K={K} N={N} M={M} {'shared' if x is xs else 'per expert'}")


def test_mx_experts_gemv_glu():
    ops = _ops()
    E, K, N, M = 4, 2080, 5, 3
    packed, scale, wd = _stack(E, 2 * N, K, 23)
    x = _x(E * M, K, 29).unflatten(0, (E, M))
    y = ops.mx_experts_linear(x, packed, scale, glu=True)
    full = torch.einsum("emk,enk->emn", x.double(), wd)
    ref = (torch.nn.functional.silu(full[..., :N]) * full[..., N:]).float()
    assert y.shape == (E, M, N)
    torch.testing.assert_close(y.float(), ref, atol=2e-2 * float(ref.abs().max()), rtol=2e-2)


def test_mx_expert_fallbacks_on_gpu(monkeypatch):
    """A misaligned stack, M = 9 and NXD_FORCE_REFERENCE=1 (dequantize + bmm) agree with the kernels
    to the tolerance of test_mx_linear_fallbacks_on_gpu."""
    ops = _ops()
    E, K, N = 4, 2080, 64
    packed, scale, wd = _stack(E, 2 * N, K, 31)
    x9 = _x(9, K, 37)
    eidx = torch.tensor([3, 0, 3, 1, 1, 0], dtype=torch.int32, device="cuda")
    k_sel = ops.mx_expert_linear(x9, packed, scale, eidx, xdiv=2, glu=True).float()
    k_all = torch.cat([ops.mx_experts_linear(x9[:8], packed, scale), ops.mx_experts_linear(x9[8:], packed, scale)], 1).float()
    tol_s = dict(atol=2e-2 * float(k_sel.abs().max()), rtol=2e-2)
    tol_a = dict(atol=2e-2 * float(k_all.abs().max()), rtol=2e-2)
    ref = torch.einsum("mk,enk->emn", x9.double(), wd).float()
    torch.testing.assert_close(k_all, ref, **tol_a)
    # M = 9: more rows than the kernel carries
    torch.testing.assert_close(ops.mx_experts_linear(x9, packed, scale).float(), k_all, **tol_a)
    # a stack one byte off 16-byte alignment
    shifted = torch.empty(E * 2 * N * (K // 2) + 1, dtype=torch.uint8, device="cuda")[1:].view(E, 2 * N, K // 2)
    shifted.copy_(packed)
    assert shifted.data_ptr() % 16 != 0
    torch.testing.assert_close(ops.mx_expert_linear(x9, shifted, scale, eidx, xdiv=2, glu=True).float(), k_sel, **tol_s)
    torch.testing.assert_close(ops.mx_experts_linear(x9[:8], shifted, scale).float(), k_all[:, :8], **tol_a)
    monkeypatch.setenv("NXD_FORCE_REFERENCE", "1")
    torch.testing.assert_close(ops.mx_expert_linear(x9, packed, scale, eidx, xdiv=2, glu=True).float(), k_sel, **tol_s)
    torch.testing.assert_close(ops.mx_experts_linear(x9[:8], packed, scale).float(), k_all[:, :8], **tol_a)


def test_mx_dequant_3d_stack_bit_exact():
    ops = _ops()
    packed, scale, wd = _stack(4, 10, 2080, 41)
    p, s = packed.contiguous(), scale.contiguous()
    got = ops.dequantize_mxfp4(p, s, torch.bfloat16)
    assert got.shape == (4, 10, 2080) and torch.equal(got.double(), wd)
    out = torch.empty_like(got)
    assert torch.equal(ops.dequantize_mxfp4_into(p, s, out), got)
    assert torch.equal(ops.dequantize_mxfp4(packed, scale, torch.bfloat16), got)   # strided stack: the torch form


# ------------------------------------------------------------------------------------------ model
# seeds picked on the CPU: the fp32 fake-quantized twin's smallest gap between the k-th and the
# (k+1)-th router probability, over both layers of the decode step of _decode_step_ids, is >= 0.02
# (E = 8 at batch 1: 0.0346; E = 4 at batch 4: 0.0281)
_TWIN_SEED = {8: 2, 4: 13}


def _tiny(E, seed):
    from transformers import MixtralConfig, MixtralForCausalLM

    from neuronx_distributed_llama3_2_amd.models.mixtral.convert import mixtral_hf_to_nxd

    cfg = MixtralConfig(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=8,
                        num_key_value_heads=2, vocab_size=1000, max_position_embeddings=512, num_local_experts=E,
                        num_experts_per_tok=2, eos_token_id=2)
    torch.manual_seed(seed)
    hf = MixtralForCausalLM(cfg)
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if "experts" in n:
                p.normal_(0.0, 0.05)
            if "gate.weight" in n:
                p.mul_(8.0)                # routing that is not near-uniform
        hf.lm_head.weight.mul_(20.0)       # wide argmax margins: random-init logits are otherwise near-tied
    # bf16 up front: the loader casts to the activation dtype before it quantizes, and the
    # fake-quantized twin must quantize the very same values
    full = mixtral_hf_to_nxd({k: v.detach().to(torch.bfloat16) for k, v in hf.state_dict().items()}, cfg)
    return cfg, full


def _app(cfg, full, batch, graphs, device="cuda", dtype=torch.bfloat16, **kw):
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, MixtralForCausalLMInference

    icfg = InferenceConfig(batch_size=batch, seq_len=128, max_context_length=64, use_hip_graphs=graphs,
                           decode_graph_steps=4 if graphs else 1, **kw)
    m = MixtralForCausalLMInference(cfg, icfg, dtype=dtype, device=torch.device(device), init_weights=False)
    m._load_full(full)
    return m


def _decode_step_ids(cfg, batch):
    g = torch.Generator().manual_seed(100 + batch)
    return torch.randint(3, cfg.vocab_size, (batch, 41), generator=g)


def _decode_step(app, ids):
    """Prefill ids[:, :-1], then one eager decode step on ids[:, -1]: (logits [B, V] fp32, smallest
    gap between the k-th and the (k+1)-th router probability over every layer and token of the step)."""
    m = app.model
    app._context_encode(ids[:, :-1])
    gaps = []
    route = m._route

    def spy(layer, x):
        router = layer.block_sparse_moe.router.linear_router
        probs = torch.softmax(torch.nn.functional.linear(x, router.weight.to(x.dtype)).float(), dim=-1)
        top = torch.topk(probs, m.top_k + 1, dim=-1).values
        gaps.append(float((top[:, m.top_k - 1] - top[:, m.top_k]).min()))
        return route(layer, x)

    m._route = spy
    try:
        B, T = ids.shape
        pos = torch.full((B, 1), T - 1, dtype=torch.int64)
        logits = app._token_generate(ids[:, -1:], position_ids=pos)[:, 0]
    finally:
        del m._route
    assert len(gaps) == len(m.model.layers)
    return logits, min(gaps)


def test_moe_block_fixed_routing_matches_bf16_kernels():
    """One block of the quantized tiny Mixtral against the bf16 kernels on its dequantized experts,
    the same top_w / top_i on both sides: 1 token (selective), 4 tokens with E = 4 (all-experts
    form), 40 tokens (scratch).  Criterion: max-abs difference / max-abs output < 0.05.
    Measured on MI355X: 0.00000, 0.00397, 0.00000 (profiles/LOG.md, MXFP4 MoE experts)."""
    for E, n in ((8, 1), (4, 4), (4, 40)):
        cfg, full = _tiny(E, _TWIN_SEED[E])
        m = _app(cfg, full, 1, False, quantized=True, quantization_type="mxfp4").model
        layer = m.model.layers[0]
        gu, d = m._expert_weights(layer)
        assert isinstance(gu, tuple) and gu[0].dtype == torch.uint8 and gu[0].is_cuda
        # bf16 copies of the dequantized experts, output-major under the logical [E, in, out] shape
        w_gu, w_d = (s.transpose(1, 2).clone().transpose(1, 2) for s in m._dequantized_experts(gu, d))
        torch.manual_seed(50 + n)
        x = torch.randn(n, cfg.hidden_size, device="cuda").to(torch.bfloat16)
        top_w, top_i = m._route(layer, x)
        got = m._experts(x, top_w, top_i, gu, d).float()
        want = m._experts(x, top_w, top_i, w_gu, w_d).float()
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"fixed routing E={E} n={n}: max-abs difference / max-abs output {rel:.5f}")
        assert rel < 0.05, (E, n, rel)


@pytest.mark.parametrize("E,batch,kv", [(8, 1, None), (4, 4, None), (8, 1, "mxfp8")])
def test_mxfp4_mixtral_graph_decode_matches_eager(E, batch, kv):
    """hipGraph decode and eager decode give the same 8 greedy tokens: batch 1 (n * k <= E, selective)
    and batch 4 with E = 4, k = 2 (all-experts form); once more on an MXFP8 KV cache."""
    from neuronx_distributed_llama3_2_amd.quantization import MXFP4ExpertFusedColumnParallel

    cfg, full = _tiny(E, _TWIN_SEED[E])
    kw = dict(quantized=True, quantization_type="mxfp4")
    if kv:
        kw["kv_cache_dtype"] = kv
    g, e = _app(cfg, full, batch, True, **kw), _app(cfg, full, batch, False, **kw)
    mo = g.model.model.layers[0].block_sparse_moe.expert_mlps.mlp_op
    assert isinstance(mo.gate_up_proj, MXFP4ExpertFusedColumnParallel) and mo.gate_up_proj.weight.is_cuda
    called = []
    for name in ("_selective_mx", "_all_experts_mx"):
        def spy(*a, _n=name, _f=getattr(e.model, name), **k):
            called.append(_n)
            return _f(*a, **k)
        setattr(e.model, name, spy)
    ids = _decode_step_ids(cfg, batch)[:, :40]
    a = g.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=8, eos_token_id=-1).cpu()
    assert set(called) == {"_selective_mx" if batch * 2 <= E else "_all_experts_mx"}, set(called)
    assert a.shape == (batch, 48) and torch.equal(a, b), (a[:, 40:], b[:, 40:])


@pytest.mark.parametrize("E,batch", [(8, 1), (4, 4)])
def test_mxfp4_mixtral_decode_step_matches_bf16_twin(E, batch):
    """One decode step of the quantized model against the bf16 model holding the dequantized weights:
    max-abs difference / max-abs logit < 0.05.  The two routers see slightly different inputs, so
    the twin's routing must not be near a tie: its smallest gap between the k-th and the (k+1)-th
    router probability is asserted to be at least 0.01 (the seed gives the fp32 model >= 0.02).
    Measured on MI355X: gap 0.0351 / 0.0235, decode step 0.00000 (E = 8, batch 1) and 0.00913 (E = 4,
    batch 4) (profiles/LOG.md, MXFP4 MoE experts)."""
    from test_mxfp4_moe import _fake_quantized_full_sd

    cfg, full = _tiny(E, _TWIN_SEED[E])
    q = _app(cfg, full, batch, False, quantized=True, quantization_type="mxfp4")
    f = _app(cfg, _fake_quantized_full_sd(full), batch, False)
    ids = _decode_step_ids(cfg, batch)
    lf, gap = _decode_step(f, ids)
    print(f"E={E} batch={batch}: bf16 twin's smallest router gap {gap:.4f}")
    assert gap >= 0.01, gap
    lq, _ = _decode_step(q, ids)
    rel = float((lq - lf).abs().max() / lf.abs().max())
    print(f"E={E} batch={batch}: decode step max-abs difference / max-abs logit {rel:.5f}")
    assert rel < 0.05, rel
