"""Decode-path linear ops (csrc/gemv.hip): skinny GEMM for M <= 8 tokens with bf16 or int8 weights,
optional per-row / per-tensor scale, bias and fused SwiGLU epilogue; int8 -> bf16 dequantisation
for the prefill path.  CPU / large-M calls fall back to dequantise + GEMM.

MXFP4 weight-only format (csrc/gemv_mx.hip; OCP Microscaling Formats v1.0).  This docstring is the
definition every other layer refers to:

* Block: 32 consecutive elements along the in-features axis of an [out, in] weight
  (in % 32 != 0 raises ValueError).
* Scale: one E8M0 byte e per block, value 2^(e-127), stored as uint8 [out, in/32].
* Element: e2m1 as a 4-bit code s<<3 | i; the magnitude i indexes {0, 0.5, 1, 1.5, 2, 3, 4, 6}.
* Packing: byte j of a row holds element 2j in its low nibble and element 2j+1 in its high nibble,
  stored as uint8 [out, in/2].  Plain uint8 storage, no float4 / e8m0 torch dtypes.

That is 4.25 bits per weight.  The quantizer: per block amax = max|v|, X = floor(log2(amax)) - 2
(from frexp, never a float log2), e = X + 127 clamped to [1, 254]; elements are v / 2^X rounded to
the nearest grid value, ties to the code with an even mantissa bit, saturating at +-6.  An all-zero
block gets e = 127 and zero codes; non-finite input raises ValueError.  The quantizer emits neither
e = 0 nor e = 255; the dequantizer below reads e = 0 as 2^-127 and e = 255 as NaN (what the GPU
kernels do with those two bytes is unspecified).  Every e2m1 value has at most two significant bits,
so code * 2^X is exact in bf16 over the normal range: dequantisation to bf16 loses nothing."""

from __future__ import annotations

import os
from typing import Optional

import torch

from ._ext import ext, use_native
from .gemm import linear as _linear


def dequantize_weight(w: torch.Tensor, scale: Optional[torch.Tensor], dtype=torch.bfloat16) -> torch.Tensor:
    """int8 [N, K] (* scale [N] / [N,1] / [1]) -> dtype [N, K]; bf16 weights pass through."""
    if w.dtype != torch.int8:
        return w
    if use_native(w) and dtype == torch.bfloat16 and w.shape[1] % 16 == 0:
        s = scale.reshape(-1).float().contiguous() if scale is not None else None
        out = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
        if s is not None and s.numel() == 1:
            ext().dequant_int8(w, s.expand(w.shape[0]).contiguous(), 1.0, out)
        else:
            ext().dequant_int8(w, s, 1.0, out)
        return out
    if scale is None:
        s = 1.0
    elif scale.numel() == 1:
        s = scale.float().reshape(())
    else:
        s = scale.float().reshape(-1, 1)
    return (w.float() * s).to(dtype)


def skinny_linear(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                  bias: Optional[torch.Tensor] = None, glu: bool = False) -> torch.Tensor:
    """x [..., K] @ W^T (+ bias) (W bf16 or int8 [Nw, K]); glu=True: W = [gate; up] rows and the
    result is silu(gate) * up of width Nw / 2."""
    K = x.shape[-1]
    lead = x.shape[:-1]
    M = x.numel() // K
    Nw = w.shape[0]
    N = Nw // 2 if glu else Nw
    if use_native(x, w) and M <= 8 and x.dtype == torch.bfloat16 and w.stride(-1) == 1:
        x2 = x.reshape(M, K)
        if x2.stride(0) % 8 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        epl = 16 if w.dtype == torch.int8 else 8
        if K % epl == 0 and w.data_ptr() % 16 == 0 and w.stride(0) % epl == 0:
            y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
            s = None
            if scale is not None:
                s = scale.reshape(-1).float()
                s = (s.expand(Nw) if s.numel() == 1 else s).contiguous()
            ext().gemv(x2, w, s, 1.0, bias, y, glu)
            return y.view(lead + (N,))
    wd = dequantize_weight(w, scale, x.dtype) if w.dtype == torch.int8 else w
    y = _linear(x, wd, bias)
    if glu:
        from .activations import swiglu

        y = swiglu(y)
    return y


def expert_linear(x: torch.Tensor, w_t: torch.Tensor, eidx: torch.Tensor, xdiv: int = 1,
                  glu: bool = False) -> torch.Tensor:
    """MoE decode projection for P (token, expert-slot) pairs: y[p] = x[p // xdiv] @ W[eidx[p]]^T,
    W given output-major as w_t [E, Nw, K]; glu=True: rows [gate; up] -> silu(gate) * up.  Reads
    only the selected experts' weights (csrc/gemv.hip expert mode); static shapes, no host sync,
    so it is captured in the decode hipGraph."""
    P = eidx.numel()
    Nw, K = w_t.shape[1], w_t.shape[2]
    N = Nw // 2 if glu else Nw
    if use_native(x, w_t) and x.dtype == torch.bfloat16 and w_t.dtype == torch.bfloat16 and w_t.stride(2) == 1 \
            and K % 8 == 0 and w_t.stride(1) % 8 == 0 and w_t.stride(0) % 8 == 0 and w_t.data_ptr() % 16 == 0:
        x2 = x.reshape(-1, K)
        if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        y = torch.empty((P, N), dtype=torch.bfloat16, device=x.device)
        ext().expert_gemv(x2, w_t, eidx.reshape(-1).to(torch.int32).contiguous(), int(xdiv), y, glu)
        return y
    rows = x.reshape(-1, K).index_select(0, torch.arange(P, device=x.device) // xdiv)
    y = torch.bmm(rows.unsqueeze(1), w_t.index_select(0, eidx.reshape(-1).long()).transpose(1, 2)).squeeze(1)
    if glu:
        from .activations import swiglu

        y = swiglu(y)
    return y


MX_BLOCK = 32
_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mxfp4(w: torch.Tensor):
    """float [out, in] -> (packed uint8 [out, in/2], E8M0 scale uint8 [out, in/32]); the format and
    the rounding rule are in the module docstring.  Pure torch, on w's device."""
    if not w.is_floating_point():
        raise TypeError(f"quantize_mxfp4 needs a floating-point weight, got {w.dtype}")
    if w.dim() < 1 or w.shape[-1] % MX_BLOCK != 0 or w.shape[-1] == 0:
        raise ValueError(f"MXFP4 blocks are {MX_BLOCK} elements along the last axis; got shape {tuple(w.shape)}")
    v = w.detach().float()
    if not bool(torch.isfinite(v).all()):
        raise ValueError("quantize_mxfp4: non-finite weight")
    lead, K = tuple(v.shape[:-1]), v.shape[-1]
    b = v.reshape(lead + (K // MX_BLOCK, MX_BLOCK))
    amax = b.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)                       # amax = m * 2^ex, 0.5 <= m < 1: floor(log2) = ex - 1
    e = (ex.to(torch.int32) - 3 + 127).clamp(1, 254)
    e = torch.where(amax == 0, torch.full_like(e, 127), e)
    nx = (127 - e).unsqueeze(-1)                    # -X; 2^-X applied in two exact steps, each a normal f32
    h = torch.div(nx, 2, rounding_mode="floor")
    a = (b * torch.exp2(h.float())) * torch.exp2((nx - h).float())
    mag = a.abs().clamp(max=6.0)
    # nearest grid value, ties to the even code: the grid step is 0.5 below 2, 1 below 4, 2 above,
    # and torch.round is round-half-to-even on the step count
    code = torch.where(mag < 2.0, torch.round(mag * 2.0),
                       torch.where(mag < 4.0, torch.round(mag) + 2.0, torch.round(mag * 0.5) + 4.0)).to(torch.uint8)
    code = code | (torch.signbit(a).to(torch.uint8) << 3)
    code = code.reshape(lead + (K // 2, 2))
    packed = code[..., 0] | (code[..., 1] << 4)
    return packed.contiguous(), e.to(torch.uint8).contiguous()


def _dequantize_mxfp4_torch(packed: torch.Tensor, scale: torch.Tensor, dtype) -> torch.Tensor:
    lut = torch.tensor(_E2M1_VALUES + tuple(-x for x in _E2M1_VALUES), dtype=torch.float32, device=packed.device)
    codes = torch.stack((packed & 0xF, packed >> 4), dim=-1).reshape(packed.shape[:-1] + (packed.shape[-1] * 2,))
    vals = lut[codes.long()]
    e = scale.to(torch.float32)
    s = torch.where(e == 255, torch.full_like(e, float("nan")), torch.exp2(e - 127.0))
    return (vals.reshape(scale.shape + (MX_BLOCK,)) * s.unsqueeze(-1)).reshape(vals.shape).to(dtype)


def _check_mxfp4(packed: torch.Tensor, scale: torch.Tensor) -> None:
    if packed.dtype != torch.uint8 or scale.dtype != torch.uint8:
        raise TypeError("MXFP4 weights are uint8 packed codes + uint8 E8M0 scales")
    if packed.shape[-1] % (MX_BLOCK // 2) != 0 or packed.shape[:-1] != scale.shape[:-1] or \
            scale.shape[-1] * (MX_BLOCK // 2) != packed.shape[-1]:
        raise ValueError(f"MXFP4 shapes: packed [out, in/2] and scale [out, in/32], got {tuple(packed.shape)} "
                         f"and {tuple(scale.shape)}")


def _mx_native_ok(packed: torch.Tensor, scale: torch.Tensor) -> bool:
    return packed.dim() == 2 and packed.stride(1) == 1 and scale.stride(1) == 1 and packed.stride(0) % 16 == 0 and \
        packed.data_ptr() % 16 == 0 and packed.numel() > 0


def dequantize_mxfp4(packed: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """MXFP4 (packed [out, in/2], scale [out, in/32]) -> dtype [out, in].  On the GPU the bf16 result
    comes from the mx_dequant kernel (bit-identical to the torch form here)."""
    _check_mxfp4(packed, scale)
    if use_native(packed, scale) and dtype == torch.bfloat16:
        if _mx_native_ok(packed, scale):
            out = torch.empty((packed.shape[0], packed.shape[1] * 2), dtype=torch.bfloat16, device=packed.device)
            ext().mx_dequant(packed, scale, out)
            return out
        if packed.dim() == 3 and packed.is_contiguous() and scale.is_contiguous() and packed.numel() > 0 and \
                packed.data_ptr() % 16 == 0:
            # an expert stack [E, out, in/2] is the 2-D kernel over its [E * out, in/2] view
            E, Nw, K2 = packed.shape
            out = torch.empty((E, Nw, K2 * 2), dtype=torch.bfloat16, device=packed.device)
            ext().mx_dequant(packed.view(E * Nw, K2), scale.view(E * Nw, -1), out.view(E * Nw, K2 * 2))
            return out
    return _dequantize_mxfp4_torch(packed, scale, dtype)


def dequantize_mxfp4_into(packed: torch.Tensor, scale: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """dequantize_mxfp4 of a contiguous expert stack into a preallocated contiguous `out`
    [E, out, in] (the MoE prefill scratch): no allocation, so it is safe under graph capture."""
    _check_mxfp4(packed, scale)
    if tuple(out.shape) != tuple(packed.shape[:-1]) + (packed.shape[-1] * 2,) or not out.is_contiguous():
        raise ValueError(f"dequantize_mxfp4_into: out {tuple(out.shape)} against packed {tuple(packed.shape)}")
    if use_native(packed, scale, out) and out.dtype == torch.bfloat16 and packed.is_contiguous() and \
            scale.is_contiguous() and packed.numel() > 0 and packed.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 \
            and packed.shape[-1] % 16 == 0:
        K2 = packed.shape[-1]
        ext().mx_dequant(packed.view(-1, K2), scale.view(-1, scale.shape[-1]), out.view(-1, K2 * 2))
    else:
        out.copy_(_dequantize_mxfp4_torch(packed, scale, out.dtype))
    return out


# NXD_MX_MFMA: the smallest row count M from which mx_linear takes the MFMA form of the MXFP4 decode product
# (csrc/gemv_mx_mfma.hip, up to MX_GEMM_MAX_ROWS rows); 0 = never.  Rows 9..16 take it whenever it is
# on, so values above 9 mean 9.  Read once per process.  Default 4: the smallest measured row count
# from which the MFMA form beats the VALU kernel at every shape of tools/bench_mx_gemv.py (at 2 rows
# it loses at three of the seven, profiles/mxfp4_mfma_gemv.jsonl).
MX_GEMM_MAX_ROWS = 16
_MX_MFMA_DEFAULT = 4
_MX_MFMA = int(os.environ.get("NXD_MX_MFMA", str(_MX_MFMA_DEFAULT)))


def mx_route(M: int) -> str:
    """Which form an M-row MXFP4 product takes once the native path applies: "gemv" (VALU kernel,
    M <= 8), "gemm" (MFMA weight tiles, M <= 16) or "dequant" (dequantise + GEMM)."""
    if _MX_MFMA > 0 and min(_MX_MFMA, 9) <= M <= MX_GEMM_MAX_ROWS:
        return "gemm"
    return "gemv" if 1 <= M <= 8 else "dequant"


def mx_linear(x: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
              glu: bool = False) -> torch.Tensor:
    """x [..., K] @ deq(W)^T (+ bias) for MXFP4 W (packed [Nw, K/2], scale [Nw, K/32]); glu=True:
    W = [gate; up] rows and the result is silu(gate) * up of width Nw / 2.  Decode-sized bf16 inputs
    on the GPU (M <= 16) read the 4-bit weights directly (mx_gemv or mx_gemm, see mx_route);
    everything else dequantises and goes through the GEMM."""
    _check_mxfp4(packed, scale)
    K = x.shape[-1]
    if packed.dim() != 2 or packed.shape[1] * 2 != K:
        raise ValueError(f"mx_linear: x [..., {K}] against packed weight {tuple(packed.shape)}")
    lead = x.shape[:-1]
    M = x.numel() // K
    Nw = packed.shape[0]
    N = Nw // 2 if glu else Nw
    route = mx_route(M)
    if use_native(x, packed, scale) and route != "dequant" and x.dtype == torch.bfloat16 and N >= 1 and \
            _mx_native_ok(packed, scale) and (bias is None or bias.dtype == torch.bfloat16):
        x2 = x.reshape(M, K)
        if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
        kernel = ext().mx_gemm if route == "gemm" else ext().mx_gemv
        kernel(x2, packed, scale, bias.contiguous() if bias is not None else None, y, glu)
        return y.view(lead + (N,))
    y = _linear(x, dequantize_mxfp4(packed, scale, x.dtype), bias)
    if glu:
        from .activations import swiglu

        y = swiglu(y)
    return y


def _check_mx_stack(x: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor, glu: bool, op: str) -> None:
    _check_mxfp4(packed, scale)
    if packed.dim() != 3 or packed.shape[2] * 2 != x.shape[-1]:
        raise ValueError(f"{op}: x [..., {x.shape[-1]}] against a packed expert stack {tuple(packed.shape)}; "
                         "expected [E, out, in/2]")
    if glu and packed.shape[1] % 2:
        raise ValueError(f"{op}: glu needs [gate; up] rows, got {packed.shape[1]} weight rows")


def _mx_stack_native_ok(packed: torch.Tensor, scale: torch.Tensor) -> bool:
    return packed.stride(2) == 1 and scale.stride(2) == 1 and packed.stride(1) % 16 == 0 and \
        packed.stride(0) % 16 == 0 and packed.data_ptr() % 16 == 0 and packed.numel() > 0 and \
        packed.stride(1) >= packed.shape[2] and scale.stride(1) >= scale.shape[2]


def _glu(y: torch.Tensor) -> torch.Tensor:
    from .activations import swiglu

    return swiglu(y)


def mx_expert_linear(x: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor, eidx: torch.Tensor, xdiv: int = 1,
                     glu: bool = False) -> torch.Tensor:
    """`expert_linear` on an MXFP4 expert stack (packed [E, Nw, K/2], scale [E, Nw, K/32], output-major):
    y[p] = x[p // xdiv] @ deq(W[eidx[p]])^T for P (token, expert-slot) pairs; glu=True: rows
    [gate; up] -> silu(gate) * up.  bf16 inputs on the GPU read only the selected experts' codes and
    scales (csrc/gemv_mx.hip expert kernel; eidx stays on the device, static shapes, capturable);
    everything else dequantises the selected experts and does a bmm."""
    _check_mx_stack(x, packed, scale, glu, "mx_expert_linear")
    if eidx.is_floating_point() or eidx.dtype == torch.bool:
        raise TypeError(f"mx_expert_linear: eidx must be an integer tensor, got {eidx.dtype}")
    xdiv = int(xdiv)
    if xdiv < 1:
        raise ValueError("mx_expert_linear: xdiv must be at least 1")
    P = eidx.numel()
    K = x.shape[-1]
    Nw = packed.shape[1]
    N = Nw // 2 if glu else Nw
    x2 = x.reshape(-1, K)
    if (P + xdiv - 1) // xdiv > x2.shape[0]:
        raise ValueError(f"mx_expert_linear: {P} pairs with xdiv {xdiv} need more than the {x2.shape[0]} rows of x")
    if use_native(x, packed, scale, eidx) and x.dtype == torch.bfloat16 and 1 <= P <= 65535 and N >= 1 and \
            _mx_stack_native_ok(packed, scale):
        if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        y = torch.empty((P, N), dtype=torch.bfloat16, device=x.device)
        ext().mx_expert_gemv(x2, packed, scale, eidx.reshape(-1).to(torch.int32).contiguous(), xdiv, y, glu)
        return y
    sel = eidx.reshape(-1).long()
    w = dequantize_mxfp4(packed.index_select(0, sel), scale.index_select(0, sel), x.dtype)   # [P, Nw, K]
    rows = x2.index_select(0, torch.arange(P, device=x.device) // xdiv)
    y = torch.bmm(rows.unsqueeze(1), w.transpose(1, 2)).squeeze(1)
    return _glu(y) if glu else y


def mx_experts_linear(x: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor, glu: bool = False) -> torch.Tensor:
    """Every expert of an MXFP4 stack on a few rows: y[e, m] = x[(e,) m] @ deq(W[e])^T with x shared
    [M, K] or per expert [E, M, K]; result [E, M, N].  bf16 inputs with M <= 8 on the GPU read each
    expert's 4-bit weights once (csrc/gemv_mx.hip expert kernel); everything else dequantises the
    stack and does a bmm.  (mx_route does not apply here: the MFMA expert form, ext().mx_experts_gemm,
    is built and tested as a kernel but not routed to.)"""
    _check_mx_stack(x, packed, scale, glu, "mx_experts_linear")
    E, Nw = packed.shape[0], packed.shape[1]
    if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[0] != E):
        raise ValueError(f"mx_experts_linear: x must be [M, K] or [{E}, M, K], got {tuple(x.shape)}")
    M, K = x.shape[-2], x.shape[-1]
    N = Nw // 2 if glu else Nw
    if use_native(x, packed, scale) and x.dtype == torch.bfloat16 and 1 <= M <= 8 and 1 <= E <= 65535 and N >= 1 and \
            _mx_stack_native_ok(packed, scale):
        if x.stride(-1) != 1 or x.stride(-2) % 8 or x.data_ptr() % 16 or (x.dim() == 3 and x.stride(0) % 8):
            x = x.contiguous()
        y = torch.empty((E, M, N), dtype=torch.bfloat16, device=x.device)
        ext().mx_experts_gemv(x, packed, scale, y, glu)
        return y
    w = dequantize_mxfp4(packed, scale, x.dtype)                                             # [E, Nw, K]
    xe = x.unsqueeze(0).expand(E, M, K) if x.dim() == 2 else x
    y = torch.bmm(xe, w.transpose(1, 2))
    return _glu(y) if glu else y
