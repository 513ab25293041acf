"""Per-element fp64 checks of the row-wise training kernels (cross-entropy, RoPE, SwiGLU, embedding,
the one-row-per-workgroup RMSNorm, the flat optimizer) at the shapes that reach their guards,
tails and grid-stride loops.  References, bounds and case tables: rowwise_refs.py.

Every test records its worst err / bound ratio per output (record_property "worst_<output>").
"""

import os

import pytest
import torch

import neuronx_distributed_llama3_2_amd.ops as ops
from neuronx_distributed_llama3_2_amd.ops import _ext, cross_entropy

import rowwise_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _native():
    assert _ext.ext_available(), "HIP extension must be built for GPU tests"
    torch.manual_seed(0)
    yield


@pytest.fixture
def worst(record_property):
    """worst(name, ratio) keeps the largest err / bound ratio per output and records it at the end."""
    seen = {}

    def note(name, ratio):
        seen[name] = max(seen.get(name, 0.0), float(ratio))

    yield note
    for k, v in seen.items():
        record_property("worst_" + k, round(v, 4))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, dtype=F32, scale=1.0):
    """Seeded on the host (the same inputs on every machine), then moved."""
    return (scale * torch.randn(*shape, generator=_gen(seed))).to(dtype).to(DEV)


def _padded(N, V, pad, dtype, seed, scale=3.0):
    """[N, V] view of an [N, V + pad] buffer (row stride V + pad) and the buffer."""
    full = _randn(N, V + pad, seed=seed, dtype=dtype, scale=scale)
    return full[:, :V], full


# ---- cross-entropy -------------------------------------------------------------------------------

def _xent_check(C, worst, x, labels, start, eps, vtot, gpad, inplace_too):
    """stats against fp64, then the backward alone: its gstat comes from the fp64 M and 1 / S."""
    N, V = x.shape
    lab = torch.tensor(labels, dtype=torch.int64, device=DEV)
    stats = torch.full((N, 4), float("nan"), device=DEV)
    C.xent_stats(x, lab, stats, start)
    ref = R.xent_stats_ref(x, lab, start)
    R.assert_bit_equal(stats[:, 0], ref["M"].float(), "row max")
    R.assert_bit_equal(stats[:, 2], ref["tgt"].float(), "target logit")
    worst("S", R.assert_elementwise(stats[:, 1], ref["S"], 0.0, ref["S_bound"], "S"))
    if bool(torch.isfinite(ref["X"]).all()):
        worst("sum_x", R.assert_elementwise(stats[:, 3], ref["X"], 0.0, ref["X_bound"], "sum x"))
    else:
        assert torch.equal(stats[:, 3].double(), ref["X"])
    g = (torch.rand(N, generator=_gen(N + V)) + 0.5).to(DEV)
    g = torch.where(lab == -100, torch.zeros_like(g), g)
    gstat = torch.stack([ref["M"], 1.0 / ref["S"], g.double(), torch.zeros_like(ref["M"])], 1).float().contiguous()
    gfull = torch.full((N, V + gpad), float("nan"), device=DEV, dtype=BF16)
    grad = gfull[:, :V]
    C.xent_bwd(x, lab, gstat, grad, start, eps, vtot)
    gref, floor, _ = R.xent_bwd_ref(x, lab, start, gstat[:, 0], gstat[:, 1], gstat[:, 2], eps, vtot)
    worst("grad", R.assert_elementwise(grad, gref, R.BF16_REL, floor, "grad"))
    assert bool(torch.isnan(gfull[:, V:]).all()), "the backward wrote past the row"
    if inplace_too:
        xfull = torch.zeros(N, x.stride(0), device=DEV, dtype=BF16)
        xi = xfull[:, :V]
        xi.copy_(x)
        C.xent_bwd(xi, lab, gstat, xi, start, eps, vtot)
        R.assert_bit_equal(xi, grad, "in-place backward")
        assert bool((xfull[:, V:] == 0).all())


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("V", R.XENT_V)
def test_xent_stats_and_bwd(V, N, dtype, eps, strided, worst):
    """V = 8: 255 idle threads; 2056: one vector in the second block; 4096: two vectors per thread.
    vocab_start = 2 V of a 4 V vocabulary, every label of xent_labels() in turn; strided: ld = V + 8
    and gld = V + 16.  bf16 logits also run the backward in place, bit-equal to out of place.

    The gradient's floor carries the documented __expf term |g| p (2 |x - M| + 2) 2^-24 (see
    rowwise_refs): where p cancels against eps / Vtot the argument rounding of the fast
    exponential, not the four fp32 roundings of 2^-22, is the larger error."""
    C = _ext.ext()
    start = 2 * V
    x, _ = _padded(N, V, 8 if strided else 0, dtype, seed=V + N)
    labels = R.xent_labels(V, start)
    for i in range(0, len(labels), N):
        group = (labels + labels)[i:i + N]
        _xent_check(C, worst, x, group, start, eps, 4 * V, 16 if strided else 0, dtype == BF16)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_xent_wide_shard(dtype, worst):
    """nvec = 16385 > 64 * 256: the backward's block count per row is capped and block 0 takes a
    second trip (the last vector, which also holds one label)."""
    N, V = R.XENT_BIG
    start = 3 * V
    x, _ = _padded(N, V, 8, dtype, seed=11)
    _xent_check(_ext.ext(), worst, x, [start + 2048 + 5, start + V - 3], start, 0.1, 4 * V, 8, dtype == BF16)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("V,lo,hi", [(4096, 4088, 4096), (2048, 0, 8), (4096, 0, 8)])
def test_xent_masked_columns(V, lo, hi, dtype, worst):
    """-inf logits (masked columns), no smoothing: a trailing block, and an aligned leading block
    of 8 with one and with two vectors per thread.  In the last case thread 0 meets an all -inf
    vector first and a finite one later: exp(-inf - (-inf)) used to put a NaN into S."""
    N = 3
    x, _ = _padded(N, V, 0, dtype, seed=V + lo)
    x[:, lo:hi] = float("-inf")
    _xent_check(_ext.ext(), worst, x, [100, V // 2, V - 20], 0, 0.0, V, 0, dtype == BF16)


def test_xent_stats_finite_inputs_unchanged():
    """The masked-column fix leaves finite rows bit-identical: statistics recorded from the kernel
    before the fix (tests/golden/xent_stats_finite.pt, inputs included)."""
    C = _ext.ext()
    cases = torch.load(os.path.join(GOLDEN, "xent_stats_finite.pt"), weights_only=True)
    assert len(cases) == 2
    for name, c in cases.items():
        x = c["x"].to(DEV)
        stats = torch.empty(x.shape[0], 4, device=DEV)
        C.xent_stats(x, c["labels"].to(DEV), stats, int(c["start"]))
        assert bool(torch.isfinite(c["stats"]).all())
        R.assert_bit_equal(stats, c["stats"], name)


@pytest.mark.parametrize("dtype,inplace,eps,masked", [(BF16, False, 0.0, False), (BF16, True, 0.1, False),
                                                      (F32, False, 0.1, False), (BF16, True, 0.0, True),
                                                      (F32, False, 0.0, True)])
def test_xent_sharded_end_to_end(dtype, inplace, eps, masked, worst, monkeypatch):
    """Four ranks over the column views (row stride 2080) of one [N, 2080] matrix through
    ops.vocab_parallel_cross_entropy, the all-gather replaced by the four kernel-made statistics,
    against the fp64 full-vocabulary loss and gradient; masked: shard 1 is all -inf.

    Gradient floor: the backward's own (xent_bwd_ref) plus |g| p times the relative error of the
    combined S (the statistics' a-priori bound) and of 1 / S."""
    C = _ext.ext()
    N, V, W = 6, 520, 4
    full = _randn(N, V * W, seed=21, dtype=dtype, scale=3.0)
    labels = [V - 1, V, V * W - 1, 0, -100, 2 * V + 7]
    if masked:
        full[:, V:2 * V] = float("-inf")
        labels[1] = 2 * V
    lab = torch.tensor(labels, device=DEV)
    orig = full.clone()
    ref_loss, loss_bound = R.xent_loss_ref(orig, lab, eps)
    st = R.xent_stats_ref(orig, lab, 0)
    g = (torch.rand(N, generator=_gen(22)) + 0.5).to(DEV)
    gz = torch.where(lab == -100, torch.zeros_like(g), g)
    gref, floor, p = R.xent_bwd_ref(orig, lab, 0, st["M"], 1.0 / st["S"], gz, eps, V * W)
    floor = floor + gz.double()[:, None].abs() * p * (st["S_bound"] / st["S"] + 2 * R.U)[:, None]

    views = [full[:, r * V:(r + 1) * V].detach().requires_grad_(True) for r in range(W)]
    assert all(v.stride(0) == V * W and v.data_ptr() == full.data_ptr() + r * V * full.element_size()
               for r, v in enumerate(views))
    stats = torch.empty(W, N, 4, device=DEV)
    for r in range(W):
        C.xent_stats(views[r], lab, stats[r], r * V)
    if masked:
        assert bool(torch.isinf(stats[1, :, 0]).all()) and bool((stats[1, :, 1] == 0).all())
    calls = []

    def gather(out, inp, group=None):
        calls.append(bool((inp == stats).flatten(1).all(1).any()))   # the rank's own kernel statistics
        out.copy_(stats)

    monkeypatch.setattr(cross_entropy.comm, "all_gather_into_tensor", gather)
    losses = [ops.vocab_parallel_cross_entropy(views[r], lab, label_smoothing=eps, world=W, rank=r,
                                               inplace_backward=inplace) for r in range(W)]
    assert calls == [True] * W
    for r in range(W):
        worst("loss", R.assert_elementwise(losses[r], ref_loss, 0.0, loss_bound, f"loss of rank {r}"))
    for r in range(W):
        losses[r].backward(g)
    grad = torch.cat([v.grad for v in views], dim=1)
    assert grad.dtype == dtype
    worst("grad", R.assert_elementwise(grad, gref, R.BF16_REL, floor, "gradient"))
    if inplace and dtype == BF16:
        R.assert_bit_equal(full, grad, "the gradient overwrote the logits")
    else:
        assert torch.equal(full, orig)


# ---- RoPE ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("posmode", ["explicit", "div_mod", "mod_only"])
@pytest.mark.parametrize("col0", [0, 72])
@pytest.mark.parametrize("T,nheads", R.ROPE_TH)
@pytest.mark.parametrize("D", R.ROPE_D)
def test_rope_inplace(D, T, nheads, col0, posmode, sign, worst):
    """(3, 5): fewer work items than one block; (37, 7): a partial last block.  Explicit positions
    are unsorted, repeated and include the table's last row; the implicit ones wrap (pos_div = 2,
    pos_mod = 7, and pos_div = 1, pos_mod = 5, both below the 64-row table)."""
    max_pos = 64
    W = col0 + nheads * D + 8
    buf0 = _randn(T, W, seed=D + T + col0, dtype=BF16)
    cos_t, sin_t = ops.rope_tables(ops.llama3_inv_freq(D, 10000.0), max_pos, device=DEV)
    pos, div, mod = None, 1, None
    if posmode == "explicit":
        pos = torch.randint(0, max_pos, (T,), generator=_gen(T)).to(DEV)
        pos[0] = max_pos - 1
        pos[2] = pos[1]
    elif posmode == "div_mod":
        div, mod = 2, 7
    else:
        mod = 5
    buf = buf0.clone()
    ops.rope_inplace_(buf, col0, nheads, D, cos_t, sin_t, pos, pos_div=div, pos_mod=mod, sign=sign)
    ref, floor = R.rope_ref(buf0, col0, nheads, D, cos_t, sin_t, R.rope_positions(T, pos, div, mod), sign)
    worst("out", R.assert_elementwise(buf[:, col0:col0 + nheads * D], ref, R.BF16_REL, floor, "rotated span"))
    R.assert_bit_equal(buf[:, :col0], buf0[:, :col0], "columns left of the span")
    R.assert_bit_equal(buf[:, col0 + nheads * D:], buf0[:, col0 + nheads * D:], "columns right of the span")


# ---- SwiGLU --------------------------------------------------------------------------------------

def _swiglu_inputs(N, I, seed):
    gu = _randn(N, 2 * I, seed=seed, dtype=BF16, scale=2.0)
    sat = torch.tensor([30.0, -30.0, 100.0, -100.0], device=DEV, dtype=BF16)
    gu[0, :4] = sat                      # gates at which the sigmoid saturates
    gu[N - 1, I - 4:I] = sat             # ... and in the row's last vector
    dh = _randn(N, I, seed=seed + 1, dtype=BF16)
    return gu, dh


@pytest.mark.parametrize("N,I", [(n, i) for i in R.SWIGLU_I for n in (1, 3)] + [(32773, 8)])
def test_swiglu(N, I, worst):
    """I = 2056: a second column block with one live thread; N = 32773: rows past the 32768-row
    grid.  Plain kernels, and the same numbers through autograd."""
    C = _ext.ext()
    gu, dh = _swiglu_inputs(N, I, seed=N + I)
    h = torch.full((N, I), float("nan"), device=DEV, dtype=BF16)
    C.swiglu_fwd(gu, h)
    dgu = torch.full((N, 2 * I), float("nan"), device=DEV, dtype=BF16)
    C.swiglu_bwd(gu, dh, dgu)
    assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(dgu.float()).all())
    worst("h", R.assert_elementwise(h, R.swiglu_fwd_ref(gu), R.BF16_REL, 0.0, "h"))
    dref, floor = R.swiglu_bwd_ref(gu, dh)
    worst("dgu", R.assert_elementwise(dgu, dref, R.BF16_REL, floor, "d(gate_up)"))
    ga = gu.clone().requires_grad_(True)
    ha = ops.swiglu(ga)
    ha.backward(dh)
    R.assert_bit_equal(ha, h, "autograd forward")
    R.assert_bit_equal(ga.grad, dgu, "autograd backward")


def test_swiglu_dual_minimal_tile(worst):
    C = _ext.ext()
    N = I = 64
    gu, dh = _swiglu_inputs(N, I, seed=5)
    h, dgu = torch.empty(N, I, device=DEV, dtype=BF16), torch.empty(N, 2 * I, device=DEV, dtype=BF16)
    C.swiglu_fwd(gu, h)
    C.swiglu_bwd(gu, dh, dgu)
    h2, h_t = torch.empty_like(h), torch.full((I, N), float("nan"), device=DEV, dtype=BF16)
    C.swiglu_fwd_dual(gu, h2, h_t)
    d2, d_t = torch.empty_like(dgu), torch.full((2 * I, N), float("nan"), device=DEV, dtype=BF16)
    C.swiglu_bwd_dual(gu, dh, d2, d_t)
    R.assert_bit_equal(h2, h, "dual forward")
    R.assert_bit_equal(h_t, h.t().contiguous(), "transposed h")
    R.assert_bit_equal(d2, dgu, "dual backward")
    R.assert_bit_equal(d_t, dgu.t().contiguous(), "transposed d(gate_up)")
    worst("h", R.assert_elementwise(h2, R.swiglu_fwd_ref(gu), R.BF16_REL, 0.0, "h"))
    dref, floor = R.swiglu_bwd_ref(gu, dh)
    worst("dgu", R.assert_elementwise(d2, dref, R.BF16_REL, floor, "d(gate_up)"))


# ---- embedding -----------------------------------------------------------------------------------

@pytest.mark.parametrize("H,T", [(8, 37), (520, 37), (8, 2_097_155)])
def test_embedding_fwd(H, T):
    """Bit-exact gather; T * H / 8 = 2 097 155 > 8192 * 256 gives the loop a second trip."""
    C = _ext.ext()
    V, start = 16, 5
    w = _randn(V, H, seed=H, dtype=BF16)
    ids = torch.randint(-4, start + V + 6, (T,), generator=_gen(T)).to(DEV)
    ids[:5] = torch.tensor([start - 1, start, start + V - 1, start + V, -3], device=DEV)
    ids[-1] = start + V - 1
    out = torch.full((T, H), float("nan"), device=DEV, dtype=BF16)
    C.embedding_fwd(ids, w, out, start)
    ref = R.embedding_fwd_ref(ids, w, start)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert bool((out[0] == 0).all()) and torch.equal(out[1], w[0]) and torch.equal(out[2], w[V - 1])


def test_embedding_bwd(worst):
    """T = 4099 > 4096 workgroups (token stride), H = 264 = 256 + 8 (column loop and remainder),
    V = 4 with every token in range: about 1025 contended atomic adds per row, onto a non-zero dw.
    Out-of-range ids leave dw untouched."""
    C = _ext.ext()
    T, H, V, start = 4099, 264, 4, 7
    ids = torch.randint(start, start + V, (T,), generator=_gen(1)).to(DEV)
    dout = _randn(T, H, seed=2, dtype=BF16)
    dw0 = _randn(V, H, seed=3)
    dw = dw0.clone()
    C.embedding_bwd(ids, dout, dw, start)
    ref, bound = R.embedding_bwd_ref(ids, dout, dw0, start)
    worst("dw", R.assert_elementwise(dw, ref, 0.0, bound, "dw"))
    outside = torch.tensor([start - 1, start + V, -1, start + V + 100] * 3, device=DEV)
    dw = dw0.clone()
    C.embedding_bwd(outside, dout[:12].contiguous(), dw, start)
    R.assert_bit_equal(dw, dw0, "dw after out-of-range ids")
    # one row hit, the others untouched
    dw = dw0.clone()
    C.embedding_bwd(torch.full((3,), start + 2, device=DEV), dout[:3].contiguous(), dw, start)
    R.assert_bit_equal(dw[[0, 1, 3]], dw0[[0, 1, 3]], "rows no token points at")
    ref, bound = R.embedding_bwd_ref(torch.full((3,), start + 2, device=DEV), dout[:3], dw0, start)
    worst("dw", R.assert_elementwise(dw, ref, 0.0, bound, "dw, three tokens"))


# ---- RMSNorm -------------------------------------------------------------------------------------

def _rmsnorm_case(H, T, with_res, rows_path, worst):
    C = _ext.ext()
    x, r, dy, dres = (_randn(T, H, seed=H + T + i, dtype=BF16) for i in range(4))
    w = (1 + 0.1 * torch.randn(H, generator=_gen(H))).to(BF16).to(DEV)
    dw0 = _randn(H, seed=H + 9)
    if not with_res:
        r = dres = None
    try:
        C.rmsnorm_set_rows_path(rows_path)
        y = torch.full((T, H), float("nan"), device=DEV, dtype=BF16)
        h = torch.full((T, H), float("nan"), device=DEV, dtype=BF16) if with_res else None
        rstd = torch.full((T,), float("nan"), device=DEV)
        C.rmsnorm_fwd(x, r, w, y, h, rstd, 1e-5)
        h_ref, y_ref, rstd_ref, rstd_rel = R.rmsnorm_fwd_ref(x, r, w, 1e-5)
        if with_res:
            R.assert_bit_equal(h, h_ref, "h")
        worst("rstd", R.assert_elementwise(rstd, rstd_ref, rstd_rel, 0.0, "rstd"))
        worst("y", R.assert_elementwise(y, y_ref, R.BF16_REL, 0.0, "y"))
        # the backward alone: it reads the (exact) h and the fp64 rstd rounded to fp32
        rstd_in = rstd_ref.float()
        for acc in (False, True):
            dx = torch.full((T, H), float("nan"), device=DEV, dtype=BF16)
            dw = dw0.clone() if acc else torch.full((H,), float("nan"), device=DEV)
            C.rmsnorm_bwd(dy, h_ref, w, rstd_in, dres, dx, dw, acc)
            dx_ref, dx_floor, dw_ref, dw_bound = R.rmsnorm_bwd_ref(dy, h_ref, w, rstd_in, dres, dw0 if acc else None)
            worst("dx", R.assert_elementwise(dx, dx_ref, R.BF16_REL, dx_floor, "dx"))
            worst("dw_acc" if acc else "dw", R.assert_elementwise(dw, dw_ref, 0.0, dw_bound, "dw"))
    finally:
        C.rmsnorm_set_rows_path(True)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("T", R.RMS_T)
@pytest.mark.parametrize("H", R.RMS_H)
def test_rmsnorm_row_per_workgroup(H, T, with_res, worst):
    """One-row-per-workgroup kernels at widths whose last vector slot is partially filled (every
    H here but 16384, which fills all 8 slots of 256 threads); T = 515 > 512 partial rows: three
    workgroups take a second row with the prefetch in flight."""
    _rmsnorm_case(H, T, with_res, False, worst)


@pytest.mark.parametrize("H", [1024, 5120])
def test_rmsnorm_rows_path_per_element(H, worst):
    """The row-per-wave kernels under the same metric, one width per SPLIT value."""
    _rmsnorm_case(H, 9, True, True, worst)


# ---- flat optimizer ------------------------------------------------------------------------------

_SMALL = [(n, gd, p16, sc, var) for n in R.FLAT_N[:3] for gd in (BF16, F32) for p16 in (True, False)
          for sc in ("none", "device", "host", "both") for var in ("plain", "hyper", "nobc")]
_BIG = [(R.FLAT_N[3], BF16, True, "both", "plain"), (R.FLAT_N[3], F32, True, "device", "hyper"),
        (R.FLAT_N[3], F32, False, "host", "nobc"), (R.FLAT_N[3], BF16, False, "none", "plain")]


@pytest.mark.parametrize("n,gdtype,has_p16,scale,variant", _SMALL + _BIG)
def test_adamw_flat(n, gdtype, has_p16, scale, variant, worst):
    """Three steps; each step's fp64 reference starts from the kernel's own previous state, so the
    per-step bounds apply: m and v from the old state, p from the old p and the new m and v just
    checked (rowwise_refs.adamw_param_ref says why: judged from the old moments, an element whose
    beta m and (1 - beta) g cancel misses 8 u (|p| + |update|) through m alone -- 1.32 of the bound
    at one of 2 098 179 elements).  hyper: lr and the bias corrections come from the device tensor
    while the host arguments are wrong on purpose."""
    h = R.ADAM
    p, m, v = _randn(n, seed=n), _randn(n, seed=n + 1, scale=0.1), (0.01 * torch.rand(n, generator=_gen(n + 2))).to(DEV)
    p16 = torch.full((n,), float("nan"), device=DEV, dtype=BF16) if has_p16 else None
    dev_scale = torch.tensor([R.GRAD_SCALE_DEV], device=DEV) if scale in ("device", "both") else None
    host_scale = R.GRAD_SCALE_HOST if scale in ("host", "both") else 1.0
    gscale = (R.GRAD_SCALE_DEV if dev_scale is not None else 1.0) * host_scale
    for step in (1, 2, 3):
        g = _randn(n, seed=n + 10 + step, dtype=gdtype)
        bc1, bc2 = (1.0, 1.0) if variant == "nobc" else (1 - h["beta1"] ** step, 1 - h["beta2"] ** step)
        (rm, rv), (mb, vb) = R.adamw_moments_ref(g, m, v, h["beta1"], h["beta2"], gscale=gscale)
        p_old = p.clone()
        hyper = torch.tensor([h["lr"], bc1, bc2], device=DEV) if variant == "hyper" else None
        ops.adamw_flat_(p, g, m, v, p16, 123.0 if variant == "hyper" else h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"],
                        7 if variant == "hyper" else step, grad_scale=dev_scale, grad_scale_host=host_scale,
                        bias_correction=variant != "nobc", hyper=hyper)
        worst("m", R.assert_elementwise(m, rm, 0.0, mb, f"m, step {step}"))
        worst("v", R.assert_elementwise(v, rv, 0.0, vb, f"v, step {step}"))
        rp, pb = R.adamw_param_ref(p_old, m, v, h["lr"], h["eps"], h["wd"], bc1, bc2)   # from the new m, v just checked
        worst("p", R.assert_elementwise(p, rp, 0.0, pb, f"p, step {step}"))
        if has_p16:
            R.assert_bit_equal(p16, p.to(BF16), "p16")


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("n", R.FLAT_N)
def test_flat_reduce(n, dtype, worst):
    """sum of squares against the a-priori bound n u sum x^2; max |x| exact, with a negative
    maximum planted in the tail and (largest n) inside the second grid-stride trip; accumulate
    onto a non-zero out, for the maximum both above and below the new value."""
    x = _randn(n, seed=n, dtype=dtype)
    ref, bound = R.sumsq_ref(x)
    worst("sumsq", R.assert_elementwise(ops.flat_sumsq(x).reshape(()), ref, 0.0, bound, "sumsq"))
    ref, bound = R.sumsq_ref(x, 2.5)
    out = torch.tensor([2.5], device=DEV)
    worst("sumsq_acc", R.assert_elementwise(ops.flat_sumsq(x, out, accumulate=True).reshape(()), ref, 0.0, bound, "sumsq acc"))
    x[n - 1] = -77.0                       # the tail (n % 4 != 0 for every n here)
    assert n % 4 != 0 and ops.flat_absmax(x).item() == 77.0
    assert ops.flat_absmax(x, torch.tensor([1000.0], device=DEV), accumulate=True).item() == 1000.0
    assert ops.flat_absmax(x, torch.tensor([1.0], device=DEV), accumulate=True).item() == 77.0
    if n > R.FLAT_SECOND_TRIP:
        x[R.FLAT_SECOND_TRIP] = -99.0
        assert ops.flat_absmax(x).item() == 99.0
        x[R.FLAT_SECOND_TRIP] = 50.0       # ... and a square that only the second trip adds
        x[n - 1] = 0.0
        ref, bound = R.sumsq_ref(x)
        got = ops.flat_sumsq(x)
        worst("sumsq", R.assert_elementwise(got.reshape(()), ref, 0.0, bound, "sumsq, second trip"))


@pytest.mark.parametrize("is_sumsq", [True, False])
def test_clip_coefficient(is_sumsq, worst):
    for stat in (0.0, 0.2, 7.0):            # zero norm, below max_norm = 1, above it
        st = torch.tensor([stat], device=DEV)
        coef = ops.clip_coefficient(st, 1.0, is_sumsq=is_sumsq)
        norm = torch.sqrt(st) if is_sumsq else st
        R.assert_bit_equal(coef[1:2], norm, "norm")
        want = torch.clamp(1.0 / (norm.double() + 1e-6), max=1.0)
        worst("coef", R.assert_elementwise(coef[0:1], want, 4 * R.U, 0.0, "coef"))
        assert (coef[0].item() == 1.0) == (norm.item() < 0.99)


@pytest.mark.parametrize("n", [1, 2048 * 256 + 7])
def test_scale_flat(n):
    x = _randn(n, seed=n)
    s = torch.tensor([0.3], device=DEV)
    want = x * s
    ops.scale_flat_(x, s)
    R.assert_bit_equal(x, want, "scaled")
