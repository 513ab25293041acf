"""The fp64 references of rowwise_refs.py against independent torch built-ins in double, the
per-element bound helper itself, and the project's CPU fallbacks (which several GPU tests use as
their reference) inside the same bounds.  Runs without a GPU."""

import math

import pytest
import torch
import torch.nn.functional as F

import neuronx_distributed_llama3_2_amd.ops as ops
from neuronx_distributed_llama3_2_amd.ops import cross_entropy

import rowwise_refs as R

D64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, what, tol=1e-12):
    a, b = a.to(D64), b.to(D64)
    err = (a - b).abs() / (1.0 + b.abs())
    assert float(err.max()) <= tol, f"{what}: {float(err.max())}"


# ---- the helper --------------------------------------------------------------------------------

def test_helper_bf16_rounded_reference_passes():
    ref = torch.randn(64, 33, generator=_gen(0), dtype=D64) * torch.logspace(-6, 3, 33, dtype=D64)
    worst = R.assert_elementwise(ref.to(torch.bfloat16), ref, R.BF16_REL, 0.0, "rounded")
    assert 0.3 < worst <= 0.5     # round to nearest: half of the bound, reached among 2112 samples


def test_helper_planted_two_ulps_in_one_small_element_fails():
    ref = torch.randn(64, 33, generator=_gen(1), dtype=D64)
    ref[17, 5] = 1.2345e-4        # four orders of magnitude below the largest element
    out = ref.to(torch.bfloat16)
    bits = out.view(torch.int16)
    bits[17, 5] += 2              # two bf16 ulps
    with pytest.raises(AssertionError, match=r"planted: worst err/bound .* at \(17, 5\)"):
        R.assert_elementwise(out, ref, R.BF16_REL, 0.0, "planted")
    # the max-norm metric of the older tests does not see it
    assert float((out.double() - ref).abs().max() / ref.abs().max()) < 1e-2


def test_helper_nan_inf_shape_and_floor():
    ref = torch.ones(4, dtype=D64)
    for bad in (float("nan"), float("inf")):
        out = ref.clone()
        out[2] = bad
        with pytest.raises(AssertionError, match=r"at \(2,\)"):
            R.assert_elementwise(out, ref, 1e-3, 0.0, "bad")
    with pytest.raises(AssertionError, match="shape"):
        R.assert_elementwise(torch.ones(3), ref, 1e-3, 0.0, "shape")
    # a reference that cancels to ~0 is judged by its floor alone; subnormal references count as zero
    assert R.assert_elementwise(torch.tensor([1e-9]), torch.tensor([0.0], dtype=D64), 0.0, torch.tensor([2e-9]), "f") == pytest.approx(0.5)
    R.assert_elementwise(torch.tensor([0.0]), torch.tensor([1e-40], dtype=D64), R.BF16_REL, 0.0, "subnormal")
    with pytest.raises(AssertionError):
        R.assert_bit_equal(torch.tensor([0.0]), torch.tensor([-0.0]), "signed zero")


# ---- cross-entropy -------------------------------------------------------------------------------

def _sharded_double(x, labels, eps, world):
    """Loss and gradient assembled in double from the per-shard references."""
    N, Vt = x.shape
    V = Vt // world
    st = [R.xent_stats_ref(x[:, r * V:(r + 1) * V], labels, r * V) for r in range(world)]
    m = torch.stack([s["M"] for s in st], -1)
    M = m.max(-1).values
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - M[:, None]))
    S = (torch.stack([s["S"] for s in st], -1) * w).sum(-1)
    T = sum(s["tgt"] for s in st)
    X = sum(s["X"] for s in st)
    lse = torch.log(S) + M
    loss = (1 - eps) * (lse - T) + eps * (lse - X / Vt) if eps > 0 else lse - T
    loss = torch.where(labels == -100, torch.zeros_like(loss), loss)
    return loss, M, S


# (a -inf logit with label smoothing has an infinite loss by definition: masks come without it)
@pytest.mark.parametrize("eps,mask", [(0.0, None), (0.1, None), (0.0, "trailing"), (0.0, "leading"), (0.0, "shard")])
def test_xent_refs_match_torch_cross_entropy(eps, mask):
    N, V, world = 5, 24, 4
    x = 3 * torch.randn(N, V * world, generator=_gen(2), dtype=D64)
    if mask == "trailing":
        x[:, -8:] = float("-inf")
    elif mask == "leading":
        x[:, :8] = float("-inf")
    elif mask == "shard":
        x[:, V:2 * V] = float("-inf")
    labels = torch.tensor([V - 1, 2 * V, 3 * V - 1, 3 * V + 5, -100])
    xa = x.clone().requires_grad_(True)
    tl = F.cross_entropy(xa, labels, reduction="none", label_smoothing=eps)
    g = torch.rand(N, generator=_gen(3), dtype=D64) + 0.5
    (tl * g).sum().backward()
    loss, M, S = _sharded_double(x, labels, eps, world)
    _close(loss, tl.detach(), "sharded loss")
    full_loss, bound = R.xent_loss_ref(x, labels, eps)
    _close(full_loss, tl.detach(), "full loss")
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    gz = torch.where(labels == -100, torch.zeros_like(g), g)
    for r in range(world):
        gr, floor, _ = R.xent_bwd_ref(x[:, r * V:(r + 1) * V], labels, r * V, M, 1.0 / S, gz, eps, V * world)
        _close(gr, xa.grad[:, r * V:(r + 1) * V], f"grad shard {r}")
        assert bool((floor >= 0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("world", [1, 4])
def test_xent_cpu_fallback_inside_bounds(dtype, eps, world, monkeypatch):
    N, V = 6, 520
    x = (3 * torch.randn(N, V * world, generator=_gen(4))).to(dtype)
    labels = torch.tensor([V - 1, V, V * world - 1, 0, -100, (2 * V + 7) % (V * world)])
    shards = [x[:, r * V:(r + 1) * V].detach().requires_grad_(True) for r in range(world)]
    stats = []
    for r in range(world):
        s = R.xent_stats_ref(shards[r], labels, r * V)
        stats.append(torch.stack([s["M"], s["S"], s["tgt"], s["X"]], 1).float())
    monkeypatch.setattr(cross_entropy.comm, "all_gather_into_tensor",
                        lambda out, inp, group=None: out.copy_(torch.stack(stats)))
    ref_loss, bound = R.xent_loss_ref(x, labels, eps)
    st = R.xent_stats_ref(x, labels, 0)
    g = torch.rand(N, generator=_gen(5)) + 0.5
    gz = torch.where(labels == -100, torch.zeros_like(g), g)
    for r in range(world):
        loss = ops.vocab_parallel_cross_entropy(shards[r], labels, label_smoothing=eps, world=world, rank=r)
        R.assert_elementwise(loss, ref_loss, 0.0, bound, f"loss rank {r}")
        loss.backward(g)
        gr, floor, p = R.xent_bwd_ref(shards[r], labels, r * V, st["M"], 1.0 / st["S"], gz, eps, V * world)
        floor = floor + gz[:, None].abs() * p * (st["S_bound"] / st["S"] + 2 * R.U)[:, None]
        R.assert_elementwise(shards[r].grad, gr, R.BF16_REL, floor, f"grad rank {r}")


# ---- RoPE ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", R.ROPE_D)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_rope_ref_and_cpu_fallback(D, sign):
    T, nh, col0 = 7, 3, 8
    W = col0 + nh * D + 8
    buf = torch.randn(T, W, generator=_gen(6)).to(torch.bfloat16)
    cos_t, sin_t = ops.rope_tables(ops.llama3_inv_freq(D, 10000.0), 16)
    pos = torch.tensor([15, 3, 3, 0, 9, 1, 15])
    ref, floor = R.rope_ref(buf, col0, nh, D, cos_t, sin_t, pos, sign)
    # independent: x * cos + rotate_half(x) * sin with the half swap written as a roll
    x = buf[:, col0:col0 + nh * D].double().view(T, nh, D)
    c = torch.cat([cos_t, cos_t], -1).double()[pos][:, None]
    s = torch.cat([sin_t, sin_t], -1).double()[pos][:, None] * sign
    flip = torch.cat([-torch.ones(D // 2, dtype=D64), torch.ones(D // 2, dtype=D64)])
    _close(ref, (x * c + torch.roll(x, D // 2, -1) * flip * s).reshape(T, -1), "rope")
    out = buf.clone()
    ops.rope_inplace_(out, col0, nh, D, cos_t, sin_t, pos, sign=sign)
    R.assert_elementwise(out[:, col0:col0 + nh * D], ref, R.BF16_REL, floor, "cpu rope")
    R.assert_bit_equal(out[:, :col0], buf[:, :col0], "left of the span")
    R.assert_bit_equal(out[:, col0 + nh * D:], buf[:, col0 + nh * D:], "right of the span")
    # implicit positions
    out2 = buf.clone()
    ops.rope_inplace_(out2, col0, nh, D, cos_t, sin_t, None, pos_div=2, pos_mod=3, sign=sign)
    ref2, floor2 = R.rope_ref(buf, col0, nh, D, cos_t, sin_t, R.rope_positions(T, None, 2, 3), sign)
    R.assert_elementwise(out2[:, col0:col0 + nh * D], ref2, R.BF16_REL, floor2, "cpu rope implicit")
    assert R.rope_positions(T, None, 2, 3).tolist() == [0, 0, 1, 1, 2, 2, 0]


# ---- SwiGLU --------------------------------------------------------------------------------------

def test_swiglu_ref_and_cpu_fallback():
    N, I = 3, 24
    gu = torch.randn(N, 2 * I, generator=_gen(7)).to(torch.bfloat16)
    gu[0, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0]).to(torch.bfloat16)
    dh = torch.randn(N, I, generator=_gen(8)).to(torch.bfloat16)
    ga = gu.double().requires_grad_(True)
    g, u = ga.chunk(2, -1)
    h = F.silu(g) * u
    h.backward(dh.double())
    _close(R.swiglu_fwd_ref(gu), h.detach(), "swiglu fwd")
    dref, floor = R.swiglu_bwd_ref(gu, dh)
    _close(dref, ga.grad, "swiglu bwd")
    gl = gu.clone().requires_grad_(True)
    out = ops.swiglu(gl)
    out.backward(dh)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(gl.grad.float()).all())
    R.assert_elementwise(out, R.swiglu_fwd_ref(gu), R.BF16_REL, 0.0, "cpu swiglu fwd")
    R.assert_elementwise(gl.grad, dref, R.BF16_REL, floor, "cpu swiglu bwd")


# ---- embedding -----------------------------------------------------------------------------------

def test_embedding_ref_and_cpu_fallback():
    V, H, start = 6, 16, 5
    w = torch.randn(V, H, generator=_gen(9)).to(torch.bfloat16)
    ids = torch.tensor([[start - 1, start, start + V - 1], [start + V, -3, start + 2]])
    local = ids - start
    mask = (local >= 0) & (local < V)
    ind = F.embedding(local.clamp(0, V - 1), w) * mask[..., None].to(w.dtype)
    # (value equality: the masking multiply of the built-in leaves -0.0 where the reference has +0.0)
    assert torch.equal(R.embedding_fwd_ref(ids, w, start), ind)
    assert torch.equal(ops.vocab_parallel_embedding(ids, w, start), ind)
    assert bool((R.embedding_fwd_ref(ids, w, start)[~mask].view(torch.int16) == 0).all())
    dout = torch.randn(2, 3, H, generator=_gen(10)).to(torch.bfloat16)
    dw0 = torch.randn(V, H, generator=_gen(11))
    ref, bound = R.embedding_bwd_ref(ids, dout, dw0, start)
    ind = dw0.double().clone()
    ind.index_add_(0, local.clamp(0, V - 1).view(-1), (dout.double() * mask[..., None]).view(-1, H))
    _close(ref, ind, "embedding bwd")
    untouched = torch.bincount(local[mask], minlength=V) == 0
    assert bool((ref[untouched] == dw0.double()[untouched]).all()) and bool((bound > 0).all())


# ---- RMSNorm -------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_res", [False, True])
def test_rmsnorm_ref_and_cpu_fallback(with_res):
    T, H = 3, 72
    x, r, dy, dres = (torch.randn(T, H, generator=_gen(12 + i)).to(torch.bfloat16) for i in range(4))
    w = (1 + 0.1 * torch.randn(H, generator=_gen(16))).to(torch.bfloat16)
    if not with_res:
        r = dres = None
    h, y, rstd, rstd_rel = R.rmsnorm_fwd_ref(x, r, w, 1e-5)
    ha = h.double().requires_grad_(True)
    wa = w.double().requires_grad_(True)
    ya = ha * torch.rsqrt(ha.pow(2).mean(-1, keepdim=True) + 1e-5) * wa
    ya.backward(dy.double())
    _close(y, ya.detach(), "rmsnorm y")
    dw0 = torch.randn(H, generator=_gen(17))
    dx, dx_floor, dw, dw_bound = R.rmsnorm_bwd_ref(dy, h, w, rstd, dres, dw0)
    _close(dx, ha.grad + (dres.double() if with_res else 0.0), "rmsnorm dx")
    _close(dw, wa.grad + dw0.double(), "rmsnorm dw")
    # the CPU fallback (fp32 leaves holding the bf16 values, as the GPU tests call it)
    xf = x.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    rf = r.float() if with_res else None
    yf, hf = ops.rms_norm(xf, wf, 1e-5, residual=rf)
    if with_res:
        R.assert_elementwise(hf, x.double() + r.double(), R.U, 0.0, "cpu h")
    hl = h.float().requires_grad_(True)   # from the stored h, like the kernel's backward
    yl = ops.rms_norm_reference(hl, wf, 1e-5)
    R.assert_elementwise(yl, y, R.BF16_REL, 0.0, "cpu y")
    yl.backward(dy.float())
    _, _, dw_fresh, dw_fresh_bound = R.rmsnorm_bwd_ref(dy, h, w, rstd, None, None)
    dx_nores, dx_nores_floor, _, _ = R.rmsnorm_bwd_ref(dy, h, w, rstd, None, None)
    # the fallback computes its own fp32 rstd (relative error rstd_rel): xhat carries it once, the
    # subtracted term three times, every dw term once
    R.assert_elementwise(hl.grad, dx_nores, R.BF16_REL, dx_nores_floor * (1 + 3 * rstd_rel / R.FLOOR), "cpu dx")
    R.assert_elementwise(wf.grad, dw_fresh, 0.0, dw_fresh_bound * (1 + rstd_rel / ((T + H) * R.U)), "cpu dw")


# ---- flat optimizer ------------------------------------------------------------------------------

def test_adamw_ref_matches_torch_adamw_over_three_steps():
    n = 37
    h = R.ADAM
    p0 = torch.randn(n, generator=_gen(18), dtype=D64)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"])
    p, m, v = p0.clone(), torch.zeros(n, dtype=D64), torch.zeros(n, dtype=D64)
    for step in (1, 2, 3):
        g = torch.randn(n, generator=_gen(18 + step), dtype=D64)
        pt.grad = g.clone()
        opt.step()
        (p, m, v), bounds = R.adamw_ref(p, g, m, v, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"],
                                        1 - h["beta1"] ** step, 1 - h["beta2"] ** step)
        _close(p, pt.detach(), f"adamw p step {step}")
        _close(m, opt.state[pt]["exp_avg"], f"adamw m step {step}")
        _close(v, opt.state[pt]["exp_avg_sq"], f"adamw v step {step}")
        assert all(bool((b >= 0).all()) for b in bounds)
    # the hyper-parameters of the case table are exact in fp32
    for k, val in h.items():
        assert float(torch.tensor(val, dtype=torch.float32)) == val, k
    for step in (1, 2, 3):
        for b in (h["beta1"], h["beta2"]):
            assert float(torch.tensor(1 - b ** step, dtype=torch.float32)) == 1 - b ** step
    assert float(torch.tensor(R.GRAD_SCALE_DEV, dtype=torch.float32) * R.GRAD_SCALE_HOST) == R.GRAD_SCALE_DEV * R.GRAD_SCALE_HOST


@pytest.mark.parametrize("n", [1, 3, 5, 1031])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("variant", ["plain", "hyper", "nobc"])
def test_flat_optimizer_cpu_fallback_inside_bounds(n, gdtype, variant):
    h = R.ADAM
    p = torch.randn(n, generator=_gen(30))
    m = 0.1 * torch.randn(n, generator=_gen(31))
    v = 0.01 * torch.rand(n, generator=_gen(32))
    p16 = torch.empty(n, dtype=torch.bfloat16)
    scale = torch.tensor([R.GRAD_SCALE_DEV])
    # the fallback applies the two scales one after the other: exact for bf16 gradients, one more
    # rounding than the bound allows for fp32 ones, which therefore take the device scale alone
    host = R.GRAD_SCALE_HOST if gdtype == torch.bfloat16 else 1.0
    for step in (1, 2, 3):
        g = torch.randn(n, generator=_gen(33 + step)).to(gdtype)
        bc1, bc2 = (1.0, 1.0) if variant == "nobc" else (1 - h["beta1"] ** step, 1 - h["beta2"] ** step)
        (rm, rv), (mb, vb) = R.adamw_moments_ref(g, m, v, h["beta1"], h["beta2"], gscale=R.GRAD_SCALE_DEV * host)
        p_old = p.clone()
        hyper = torch.tensor([h["lr"], bc1, bc2]) if variant == "hyper" else None
        ops.adamw_flat_(p, g, m, v, p16, 123.0 if variant == "hyper" else h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"],
                        7 if variant == "hyper" else step, grad_scale=scale, grad_scale_host=host,
                        bias_correction=variant != "nobc", hyper=hyper)
        R.assert_elementwise(m, rm, 0.0, mb, f"cpu m step {step}")
        R.assert_elementwise(v, rv, 0.0, vb, f"cpu v step {step}")
        rp, pb = R.adamw_param_ref(p_old, m, v, h["lr"], h["eps"], h["wd"], bc1, bc2)   # from the new m, v just checked
        R.assert_elementwise(p, rp, 0.0, pb, f"cpu p step {step}")
        R.assert_bit_equal(p16, p.to(torch.bfloat16), "cpu p16")
    x = torch.randn(n, generator=_gen(40)).to(gdtype)
    ref, bound = R.sumsq_ref(x)
    R.assert_elementwise(ops.flat_sumsq(x).reshape(()), ref, 0.0, bound, "cpu sumsq")
    ref, bound = R.sumsq_ref(x, 2.5)
    R.assert_elementwise(ops.flat_sumsq(x, torch.tensor([2.5]), accumulate=True).reshape(()), ref, 0.0, bound, "cpu sumsq acc")
    x[n - 1] = -77.0
    assert ops.flat_absmax(x).item() == 77.0
    assert ops.flat_absmax(x, torch.tensor([1000.0]), accumulate=True).item() == 1000.0
    assert ops.flat_absmax(x, torch.tensor([1.0]), accumulate=True).item() == 77.0
    for is_sumsq in (True, False):
        for stat in (0.0, 0.25, 9.0):
            coef = ops.clip_coefficient(torch.tensor([stat]), 1.0, is_sumsq=is_sumsq)
            norm = math.sqrt(stat) if is_sumsq else stat
            assert coef[1].item() == norm
            R.assert_elementwise(coef[0], torch.tensor(min(1.0, 1.0 / (norm + 1e-6)), dtype=D64), 4 * R.U, 0.0, "cpu coef")
    y = torch.randn(n, generator=_gen(41))
    s = torch.tensor([0.3])
    exp = y * s
    ops.scale_flat_(y, s)
    R.assert_bit_equal(y, exp, "cpu scale")
