"""fp64 references, the per-element bound and the case tables of the row-wise training kernels
(cross-entropy, RoPE, SwiGLU, embedding, RMSNorm, flat optimizer).

Plain module (like dist_utils.py), shared by test_rowwise_refs.py (CPU) and
test_rowwise_kernels_gpu.py.  Every reference is written out from the op's definition in double
and also returns the absolute `floor` of its outputs, computed from the absolute values of the
summands of each element's own expression.

Where the constants come from (u = 2^-24, the unit roundoff of fp32):

* bf16 outputs, rel = 2^-7: round-to-nearest to bf16 costs up to 2^-8 |ref|; one more unit of
  that is granted to the fp32 internals.
* floor = 2^-22 * sum|summands|: four fp32 roundings of an expression whose terms cancel.
* fp32 reductions: the order-independent a-priori bound k * u * sum|terms| (k terms); k + H when
  the terms carry the error of a length-H reduction themselves.
* single correctly rounded fp32 operations: bit-equal, no bound.
* __expf (v_exp_f32 of x * log2(e)): the product x * log2(e) is rounded to fp32 and log2(e) is
  itself a rounded constant, so the argument of the base-2 exponential is off by up to
  2 u |x| log2(e), i.e. the result by a factor 1 +- 2 u |x|; the instruction adds 1 ulp = 2 u.
  rel_expf(x) = (2 |x| + 2) u.  This is the one widening beyond the plain rules, applied only
  where a kernel calls __expf and the term can dominate (cross-entropy).
* values below the smallest normal (2^-126, the same for bf16 and fp32) count as zero: the
  hardware may flush them.
"""

import math

import torch

U = 2.0 ** -24
BF16_REL = 2.0 ** -7
FLOOR = 2.0 ** -22
TINY = 2.0 ** -126


def f64(t):
    """Lift to double on the tensor's own device (the references run wherever their inputs are)."""
    return t.detach().to(torch.float64)


def assert_elementwise(out, ref64, rel, floor64, what):
    """|out - ref| <= rel * |ref| + floor for every element; returns the worst err / bound."""
    r = f64(ref64)
    o = f64(out).to(r.device)
    assert o.shape == r.shape, f"{what}: shape {tuple(o.shape)} vs reference {tuple(r.shape)}"
    if o.numel() == 0:
        return 0.0
    r = torch.where(r.abs() < TINY, torch.zeros_like(r), r)
    fl = f64(floor64).to(r.device) if torch.is_tensor(floor64) else float(floor64)
    bound = rel * r.abs() + fl + TINY
    ratio = torch.nan_to_num((o - r).abs() / bound, nan=float("inf"), posinf=float("inf"))
    ratio = ratio.expand(o.shape)
    flat = int(ratio.reshape(-1).argmax())
    worst = float(ratio.reshape(-1)[flat])
    if not worst <= 1.0:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), o.shape)) if o.dim() else ()
        bound = bound.expand(o.shape)
        raise AssertionError(f"{what}: worst err/bound {worst:.4g} at {idx}: out {float(o.reshape(-1)[flat])!r} "
                             f"ref {float(r.reshape(-1)[flat])!r} bound {float(bound.reshape(-1)[flat]):.4g}")
    return worst


def assert_bit_equal(out, ref, what):
    o, r = out.detach().cpu(), ref.detach().cpu()
    assert o.dtype == r.dtype and o.shape == r.shape, f"{what}: {o.dtype}{tuple(o.shape)} vs {r.dtype}{tuple(r.shape)}"
    if o.dtype == torch.bfloat16:
        same = o.view(torch.int16) == r.view(torch.int16)
    elif o.dtype == torch.float32:
        same = o.view(torch.int32) == r.view(torch.int32)
    else:
        same = o == r
    if not bool(same.all()):
        bad = (~same).reshape(-1).nonzero()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {o.numel()} elements differ, first at flat index {i}: "
                             f"{o.reshape(-1)[i].item()!r} vs {r.reshape(-1)[i].item()!r}")
    return 0.0


def rel_expf(x64):
    return (2.0 * x64.abs() + 2.0) * U


# ------------------------------------------------------------------------------------------------
# cross-entropy
# ------------------------------------------------------------------------------------------------

def xent_stats_ref(x, labels, vocab_start):
    """Shard-local statistics of logits x [N, V] (any dtype, lifted to double; -inf allowed).

    Returns dict M, S, tgt, X and the bounds S_bound, X_bound.  An all -inf row gives M = -inf,
    S = 0.  S_bound: V summed terms, each a product with at most ceil(V / 2048) + 10 rescaling
    factors __expf(m_old - m_new) (per-thread trips, 6 wave levels, 3 block steps, the term's own
    exponential), every argument at most the row's range R = M - min finite x."""
    x = f64(x)
    N, V = x.shape
    M = x.max(-1).values
    Ms = torch.where(torch.isinf(M), torch.zeros_like(M), M)
    fin = torch.isfinite(x)
    e = torch.where(fin, torch.exp(torch.where(fin, x, torch.zeros_like(x)) - Ms[:, None]), torch.zeros_like(x))
    S = e.sum(-1)
    lab = f64(labels).long() - vocab_start
    inr = (lab >= 0) & (lab < V)
    tgt = torch.where(inr, x.gather(1, lab.clamp(0, V - 1)[:, None]).squeeze(1), torch.zeros_like(M))
    X = x.sum(-1)
    xmin = torch.where(fin, x, Ms[:, None].expand_as(x)).min(-1).values
    R = Ms - xmin
    S_bound = (V + (math.ceil(V / 2048) + 10) * (2 * R + 2)) * U * S
    X_bound = V * U * torch.where(fin, x, torch.zeros_like(x)).abs().sum(-1)
    return dict(M=M, S=S, tgt=tgt, X=X, S_bound=S_bound, X_bound=X_bound)


def xent_loss_ref(x_full, labels, eps, ignore_index=-100):
    """Full-vocabulary per-token loss in double and its bound for a loss assembled in fp32 from
    kernel statistics: the relative error of S (as in xent_stats_ref, over the whole vocabulary)
    passes through the logarithm unchanged, each of the handful of fp32 operations costs u of its
    operands, and the smoothing term carries the error of sum x."""
    st = xent_stats_ref(x_full, labels, 0)
    V = x_full.shape[1]
    lse = torch.log(st["S"]) + st["M"]
    nll = lse - st["tgt"]
    xf = f64(x_full)
    absx = torch.where(torch.isfinite(xf), xf, torch.zeros_like(xf)).abs().sum(-1)
    loss = (1 - eps) * nll + eps * (lse - st["X"] / V) if eps > 0 else nll
    valid = f64(labels).long() != ignore_index
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    bound = st["S_bound"] / st["S"] + 4 * U * (st["M"].abs() + torch.log(st["S"]).abs() + lse.abs() + st["tgt"].abs()
                                               + loss.abs())
    if eps > 0:
        bound = bound + eps * (V * U * absx / V + 2 * U * st["X"].abs() / V)
    return loss, bound


def xent_bwd_ref(x, labels, vocab_start, M, invS, g, eps, vtot):
    """grad = g * (exp(x - M) * invS - (1 - eps) * onehot - eps / vtot) and its floor
    2^-22 |g| (p + onehot + eps / vtot) plus the __expf term |g| p rel_expf(x - M).
    M, invS, g are the values the kernel reads (fp32), lifted to double.  Also returns p."""
    x = f64(x)
    N, V = x.shape
    M, invS, g = f64(M), f64(invS), f64(g)
    fin = torch.isfinite(x)
    d = torch.where(fin, x, torch.zeros_like(x)) - M[:, None]
    p = torch.where(fin, torch.exp(d) * invS[:, None], torch.zeros_like(x))
    lab = f64(labels).long() - vocab_start
    inr = (lab >= 0) & (lab < V)
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, lab.clamp(0, V - 1)[:, None], inr.to(torch.float64)[:, None])
    grad = g[:, None] * (p - (1 - eps) * onehot - eps / vtot)
    floor = g.abs()[:, None] * (FLOOR * (p + onehot + eps / vtot) + p * rel_expf(d))
    return grad, floor, p


# ------------------------------------------------------------------------------------------------
# RoPE
# ------------------------------------------------------------------------------------------------

def rope_positions(T, pos, pos_div, pos_mod):
    if pos is not None:
        return pos.detach().long()
    return (torch.arange(T) // pos_div) % pos_mod


def rope_ref(buf, col0, nheads, D, cos_t, sin_t, positions, sign):
    """Rotated span [T, nheads * D] of buf [T, W] in double (bf16 input and fp32 tables lifted)
    and the floor 2^-22 (|x1 c| + |x2 s|) per element."""
    T = buf.shape[0]
    x = f64(buf)[:, col0:col0 + nheads * D].reshape(T, nheads, D)
    positions = positions.to(buf.device)
    c = f64(cos_t)[positions][:, None, :]
    s = f64(sin_t)[positions][:, None, :] * sign
    x1, x2 = x[..., : D // 2], x[..., D // 2:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    floor = FLOOR * torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return out.reshape(T, nheads * D), floor.reshape(T, nheads * D)


# ------------------------------------------------------------------------------------------------
# SwiGLU
# ------------------------------------------------------------------------------------------------

def swiglu_fwd_ref(gu):
    g, u = f64(gu).chunk(2, dim=-1)
    return g * torch.sigmoid(g) * u


def swiglu_bwd_ref(gu, dh):
    """d(gate_up) = [dh u s (1 + g (1 - s)) | dh g s]; the gate half cancels near g = -1.278, its
    floor is 2^-22 |dh u s| (1 + |g| (1 - s))."""
    g, u = f64(gu).chunk(2, dim=-1)
    d = f64(dh)
    s = torch.sigmoid(g)
    one_minus_s = torch.sigmoid(-g)
    dg = d * u * s * (1 + g * one_minus_s)
    du = d * g * s
    floor = torch.cat([FLOOR * (d * u * s).abs() * (1 + g.abs() * one_minus_s), torch.zeros_like(du)], dim=-1)
    return torch.cat([dg, du], dim=-1), floor


# ------------------------------------------------------------------------------------------------
# embedding
# ------------------------------------------------------------------------------------------------

def embedding_fwd_ref(ids, w, start):
    """Exact gather: rows of w for ids inside [start, start + V), zero rows elsewhere."""
    V, H = w.shape
    local = ids.reshape(-1).long() - start
    inr = (local >= 0) & (local < V)
    out = w[local.clamp(0, V - 1)]
    out = torch.where(inr[:, None], out, torch.zeros_like(out))
    return out.reshape(tuple(ids.shape) + (H,))


def embedding_bwd_ref(ids, dout, dw0, start):
    """dw0 + scatter-add of dout rows in double; bound k u sum|terms| per row, k = hits (+1 for a
    non-zero dw0 row, itself a term of the sum)."""
    V, H = dw0.shape
    local = ids.detach().reshape(-1).long() - start
    inr = (local >= 0) & (local < V)
    d = f64(dout).reshape(-1, H)[inr]
    rows = local[inr]
    dw = f64(dw0).clone()
    dw.index_add_(0, rows, d)
    absum = f64(dw0).abs()
    absum.index_add_(0, rows, d.abs())
    k = torch.bincount(rows, minlength=V).to(torch.float64) + 1
    return dw, k[:, None] * U * absum


# ------------------------------------------------------------------------------------------------
# RMSNorm
# ------------------------------------------------------------------------------------------------

def rmsnorm_fwd_ref(x, res, w, eps):
    """h (bf16, exact: one fp32 add rounded once), y and rstd in double from the stored h.
    rstd: the sum of squares is a length-H fp32 reduction of rounded products (all positive, so
    its relative error is at most (H + 1) u); the mean, + eps and the reciprocal square root add
    a few more."""
    h = (x.float() + res.float()).to(torch.bfloat16) if res is not None else x
    h64 = f64(h)
    H = h64.shape[-1]
    rstd = 1.0 / torch.sqrt(h64.pow(2).mean(-1) + eps)
    y = h64 * rstd[:, None] * f64(w)
    return h, y, rstd, (H + 8) * U


def rmsnorm_bwd_ref(dy, h, w, rstd, dres, dw0):
    """dx = rs (dy w - xhat mean) (+ dres), dw = dw0 + sum_rows dy xhat; rstd is the fp32 tensor
    the kernel reads.  Floors: dx 2^-22 (rs (|dy w| + |xhat mean|) + |dres|); dw (T + H) u sum|terms|."""
    dy, h, w, rs = f64(dy), f64(h), f64(w), f64(rstd)[:, None]
    T, H = h.shape
    xh = h * rs
    gw = dy * w
    mean = (gw * xh).mean(-1, keepdim=True)
    dx = rs * (gw - xh * mean)
    floor = rs * (gw.abs() + (xh * mean).abs())
    if dres is not None:
        dx = dx + f64(dres)
        floor = floor + f64(dres).abs()
    terms = dy * xh
    dw = terms.sum(0)
    dw_abs = terms.abs().sum(0)
    if dw0 is not None:
        dw = dw + f64(dw0)
        dw_abs = dw_abs + f64(dw0).abs()
    return dx, FLOOR * floor, dw, (T + H) * U * dw_abs


# ------------------------------------------------------------------------------------------------
# flat optimizer
# ------------------------------------------------------------------------------------------------

# Hyper-parameters that fp32 holds exactly (so 1 - beta, 1 - lr * wd and the bias corrections of
# the first three steps are exact and the reference does not depend on where a double is
# narrowed), and gradient scales whose product is exact.
ADAM = dict(lr=2.0 ** -10, beta1=0.875, beta2=0.96875, eps=2.0 ** -27, wd=0.125)
GRAD_SCALE_DEV = 0.375
GRAD_SCALE_HOST = 3.0


def adamw_moments_ref(g, m, v, beta1, beta2, gscale=1.0):
    """New moments in double from the old ones and their bounds
    4 u (|beta old| + |(1 - beta) g^(1 or 2)|)."""
    g, m, v = f64(g) * gscale, f64(m), f64(v)
    m1 = beta1 * m + (1 - beta1) * g
    v1 = beta2 * v + (1 - beta2) * g * g
    mb = 4 * U * ((beta1 * m).abs() + ((1 - beta1) * g).abs())
    vb = 4 * U * ((beta2 * v).abs() + ((1 - beta2) * g * g).abs())
    return (m1, v1), (mb, vb)


def adamw_param_ref(p, m1, v1, lr, eps, wd, bc1, bc2):
    """p (1 - lr wd) - update, update = (lr / bc1) m1 / (sqrt(v1 / bc2) + eps), from the NEW moments
    given (lifted to double), and the bound 8 u (|p| + |update|): the eight roundings between the
    moments and the update (square root, 1 / sqrt(bc2), their product, + eps, lr / bc1, its product
    with m, the division, the final subtraction).  A kernel's p is judged against this reference
    taken from the kernel's own new moments: where beta m and (1 - beta) g cancel, m -- and with it
    the update -- has no relative accuracy, which the moments' own absolute bound covers and this
    one cannot."""
    p, m1, v1 = f64(p), f64(m1), f64(v1)
    upd = (lr / bc1) * m1 / (torch.sqrt(v1) / math.sqrt(bc2) + eps)
    return p * (1 - lr * wd) - upd, 8 * U * (p.abs() + upd.abs())


def adamw_ref(p, g, m, v, lr, beta1, beta2, eps, wd, bc1, bc2, gscale=1.0):
    """One whole AdamW step in double from the given state: (p, m, v) and their bounds."""
    (m1, v1), (mb, vb) = adamw_moments_ref(g, m, v, beta1, beta2, gscale)
    p1, pb = adamw_param_ref(p, m1, v1, lr, eps, wd, bc1, bc2)
    return (p1, m1, v1), (pb, mb, vb)


def sumsq_ref(x, out0=0.0):
    x = f64(x)
    s = x.pow(2).sum() + out0
    return s, x.numel() * U * (x.pow(2).sum() + abs(out0))


# n = 1, 3: tail only; 5: one quad plus a tail; 2 098 179 = 4*256*2048 + 4*256 + 3: the first 256
# threads take a second trip of the grid-stride loop, plus a tail of 3
FLAT_N = [1, 3, 5, 4 * 256 * 2048 + 4 * 256 + 3]
FLAT_SECOND_TRIP = 4 * 256 * 2048 + 17      # an element inside the second trip (n = FLAT_N[-1])

XENT_V = [8, 2056, 4096]
XENT_BIG = (2, 131080)                      # nvec > 64 * 256: gx cap and a second backward trip
ROPE_D = [64, 128, 256]
ROPE_TH = [(3, 5), (37, 7)]
SWIGLU_I = [8, 1792, 2056]
RMS_H = [8, 72, 2056, 4608, 9216, 16384]
RMS_T = [1, 3, 515]


def xent_labels(V, start):
    """Labels at the shard's edges: one below it, its first and last column, one past it, the
    last vector, the second 256-vector block (or the middle of a narrower shard), ignored."""
    second_block = start + 2048 + 5 if V > 2053 else start + V // 2
    return [start - 1, start, start + V - 1, start + V, start + V - 3, second_block, -100]
