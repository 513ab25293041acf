"""Decode-path kernels (csrc/inference.hip): flash-decoding attention over a persistent KV cache,
in-place KV-cache writes, argmax and top-k multinomial sampling.

Cache layout: [batch, kv_heads, max_len, head_dim] (the reference's KV-cache parameter layout,
examples/inference/modules/model_base.py:114-125); valid length per sequence comes from a device
int32 tensor, so a decode step has static shapes and can be captured in a hipGraph.

MXFP8 KV cache (OCP Microscaling v1.0; csrc/kv_cache_mx.hip, the KV8 form of csrc/decode_attn.hip)
-----------------------------------------------------------------------------------------------
A cache may hold 8.25 bits per element (33/64 of bf16) instead of bf16: `kv_cache_write` and
`decode_attention` take `uint8` caches together with `k_scale` / `v_scale`.

Codes: `uint8`, the shape of the bf16 cache, `[B, Hkv, Lmax, D]`.  The byte is the OCP FP8 E4M3 bit
pattern (`e4m3fn`, gfx950's native form, not `fnuz`): bias 7, largest value 448, no infinity,
NaN = 0x7F / 0xFF.  `D % 32 != 0` raises `ValueError`.

Scales: `uint8` `[B, Hkv, Lmax, D/32]`, E8M0: byte `e` means `2^(e-127)`; block `j` of a head vector
covers its elements `32j .. 32j+31`.

Quantizer (`quantize_mxfp8` is the definition; the native write equals it bit for bit), per block:
`amax = max|v|`; `X = floor(log2(amax)) - 8`, taken from the exponent (`frexp`), never a float
`log2`; `e = X + 127` clamped to [1, 254]; the elements are `v / 2^(e-127)` clamped to +-448 and
rounded to nearest-even E4M3 -- saturating, never NaN.  An all-zero block gets `e = 127` and zero codes.

Unspecified: the op runs inside hipGraphs, so it never raises on values.  Non-finite input, bf16
subnormals and blocks with `0 < amax < 2^-100` give unspecified codes (they do not fault).  The
quantizer never emits `e = 0`, `e = 255` or a NaN code; what the kernels do with those is unspecified.
A zeroed cache (`reset_kv_cache`) is valid: code 0 is 0 under any scale.

Every code times `2^(e-127)` has at most four significant bits, so dequantization to bf16 loses
nothing: a decode step over a quantized cache equals the same step over its bf16 dequantization.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from ._ext import ext, use_native

CHUNK = 128


def decode_window(window: Optional[int], num_keys: int) -> int:
    """The window the decode kernels get: 0 (none) for None, 0 or a window of at least num_keys keys."""
    if window is None:
        return 0
    window = int(window)
    if window < 0:
        raise ValueError(f"window must be positive, got {window}")
    return 0 if window >= num_keys else window


MX8_BLOCK = 32


def quantize_mxfp8(x: torch.Tensor):
    """x [..., D] (any float dtype, any device), D % 32 == 0 -> (codes uint8 [..., D], scale uint8
    [..., D/32]): the MXFP8 format of the module docstring, blocks along the last axis."""
    D = x.shape[-1]
    if D % MX8_BLOCK:
        raise ValueError(f"MXFP8 blocks are {MX8_BLOCK} elements: last dim {D} is not a multiple")
    v = x.detach().to(torch.float32).reshape(x.shape[:-1] + (D // MX8_BLOCK, MX8_BLOCK))
    amax = v.abs().amax(-1)
    # amax = m * 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1, so e = (ex - 1 - 8) + 127
    ex = torch.frexp(amax)[1].to(torch.int32)
    e = torch.where(amax > 0, (ex + 118).clamp(1, 254), torch.full_like(ex, 127))
    inv = ((254 - e) << 23).view(torch.float32)   # 2^(127 - e), exact
    codes = (v * inv.unsqueeze(-1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.reshape(x.shape), e.to(torch.uint8)


def dequantize_mxfp8(codes: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """codes uint8 [..., D], scale uint8 [..., D/32] -> code * 2^(scale - 127) in `dtype` (exact in bf16)."""
    D = codes.shape[-1]
    if D % MX8_BLOCK or scale.shape[-1] * MX8_BLOCK != D or scale.shape[:-1] != codes.shape[:-1]:
        raise ValueError(f"MXFP8 codes {tuple(codes.shape)} / scales {tuple(scale.shape)} do not match")
    if codes.dtype != torch.uint8 or scale.dtype != torch.uint8:
        raise TypeError("MXFP8 codes and scales are uint8")
    v = codes.contiguous().view(torch.float8_e4m3fn).to(torch.float32).reshape(codes.shape[:-1] + (D // MX8_BLOCK, MX8_BLOCK))
    s = (scale.to(torch.int32) << 23).view(torch.float32)
    return (v * s.unsqueeze(-1)).reshape(codes.shape).to(dtype)


def _mx8_caches(k_cache, v_cache, k_scale, v_scale) -> bool:
    """True for an MXFP8 cache (uint8 codes with both scale tensors); TypeError for half of one."""
    quant = k_cache.dtype == torch.uint8 or v_cache.dtype == torch.uint8
    if not quant:
        if k_scale is not None or v_scale is not None:
            raise TypeError("k_scale / v_scale go with uint8 (MXFP8) caches")
        return False
    if k_cache.dtype != torch.uint8 or v_cache.dtype != torch.uint8:
        raise TypeError("an MXFP8 cache needs both caches as uint8 codes")
    if k_scale is None or v_scale is None:
        raise TypeError("uint8 (MXFP8) caches need k_scale and v_scale")
    if k_scale.dtype != torch.uint8 or v_scale.dtype != torch.uint8:
        raise TypeError("MXFP8 scales are uint8 (E8M0)")
    D = k_cache.shape[-1]
    if D % MX8_BLOCK:
        raise ValueError(f"MXFP8 blocks are {MX8_BLOCK} elements: head dim {D} is not a multiple")
    want = tuple(k_cache.shape[:-1]) + (D // MX8_BLOCK,)
    if tuple(k_scale.shape) != want or tuple(v_scale.shape) != want or v_cache.shape != k_cache.shape:
        raise ValueError(f"MXFP8 scales must be {want} for caches {tuple(k_cache.shape)}")
    return True


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, seq_len: torch.Tensor,
                     cache_idx: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None,
                     out: Optional[torch.Tensor] = None, window: Optional[int] = None,
                     k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q: [B, T, Hq, D] new-token queries; keys [0, seq_len[b]) are valid for the LAST token, and
    token t sees keys < lim = seq_len[b] - (T - 1 - t).  window: sliding-window attention, token t
    sees only the keys >= lim - window (itself and the window - 1 before it); None, 0 or at least
    the cache length mean no window.  uint8 caches with k_scale / v_scale: an MXFP8 cache (module
    docstring).  Returns [B, T, Hq, D]."""
    B, T, Hq, D = q.shape
    quant = _mx8_caches(k_cache, v_cache, k_scale, v_scale)
    window = decode_window(window, k_cache.shape[2])
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty((B, T, Hq, D), dtype=q.dtype, device=q.device)
    if use_native(q, k_cache):
        nsplit = max(1, (k_cache.shape[2] + CHUNK - 1) // CHUNK)
        ext().decode_attn(q, k_cache, v_cache, cache_idx.to(torch.int32) if cache_idx is not None else None,
                          seq_len.to(torch.int32), out, float(scale), nsplit, *((window,) if window else ()),
                          **(dict(k_scale=k_scale, v_scale=v_scale) if quant else {}))
        return out
    Hkv = k_cache.shape[1]
    g = Hq // Hkv
    for b in range(B):
        cb = int(cache_idx[b]) if cache_idx is not None else b
        L = int(seq_len[b])
        if quant:   # the visible rows, dequantized (exact), then the same fp32 loop
            kk = dequantize_mxfp8(k_cache[cb, :, :L], k_scale[cb, :, :L], torch.float32).repeat_interleave(g, 0)
            vv = dequantize_mxfp8(v_cache[cb, :, :L], v_scale[cb, :, :L], torch.float32).repeat_interleave(g, 0)
        else:
            kk = k_cache[cb, :, :L].float().repeat_interleave(g, 0)  # [Hq, L, D]
            vv = v_cache[cb, :, :L].float().repeat_interleave(g, 0)
        qq = q[b].float().permute(1, 0, 2)  # [Hq, T, D]
        s = torch.matmul(qq, kk.transpose(-1, -2)) * scale
        ti = torch.arange(T, device=q.device)[:, None]
        ki = torch.arange(L, device=q.device)[None, :]
        lim = L - (T - 1 - ti)
        hidden = ki >= lim
        if window:
            hidden = hidden | (ki < lim - window)
        s = s.masked_fill(hidden, float("-inf"))
        p = torch.softmax(s, -1).nan_to_num(0.0)   # a row with no visible key (seq_len < T) is 0, as the kernels
        out[b] = torch.matmul(p, vv).permute(1, 0, 2).to(out.dtype)
    return out


def kv_cache_write(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                   positions: torch.Tensor, cache_idx: Optional[torch.Tensor] = None,
                   k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> None:
    """k_new/v_new: [B, T, Hkv, D]; writes cache[cache_idx[b], :, positions[b] + t] in place (positions
    past the cache are dropped).  uint8 caches with k_scale / v_scale: the rows are quantized to MXFP8
    (module docstring) and written as codes plus scales."""
    quant = _mx8_caches(k_cache, v_cache, k_scale, v_scale)
    if quant and use_native(k_new, k_cache):
        ext().kv_cache_write(k_new, v_new, k_cache, v_cache,
                             cache_idx.to(torch.int32) if cache_idx is not None else None, positions.to(torch.int32),
                             k_scale=k_scale, v_scale=v_scale)
        return
    if quant:
        B, T = k_new.shape[:2]
        for b in range(B):
            cb = int(cache_idx[b]) if cache_idx is not None else b
            p0 = int(positions[b])
            n = max(0, min(T, k_cache.shape[2] - p0))
            for new, cache, sc in ((k_new, k_cache, k_scale), (v_new, v_cache, v_scale)):
                codes, e = quantize_mxfp8(new[b, :n].transpose(0, 1))
                cache[cb, :, p0:p0 + n] = codes
                sc[cb, :, p0:p0 + n] = e
        return
    if use_native(k_new, k_cache):
        ext().kv_cache_write(k_new, v_new, k_cache, v_cache,
                             cache_idx.to(torch.int32) if cache_idx is not None else None, positions.to(torch.int32))
        return
    B, T = k_new.shape[:2]
    for b in range(B):
        cb = int(cache_idx[b]) if cache_idx is not None else b
        p0 = int(positions[b])
        n = max(0, min(T, k_cache.shape[2] - p0))
        k_cache[cb, :, p0:p0 + n] = k_new[b, :n].transpose(0, 1).to(k_cache.dtype)
        v_cache[cb, :, p0:p0 + n] = v_new[b, :n].transpose(0, 1).to(v_cache.dtype)


def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    if use_native(x):
        out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
        ext().argmax_rows(x if x.stride(-1) == 1 else x.contiguous(), out)
        return out
    return torch.argmax(x, dim=-1)


def greedy_advance_(logits: torch.Tensor, slot: torch.Tensor, out: torch.Tensor, step: torch.Tensor,
                    tokens: torch.Tensor, positions: torch.Tensor, cache_len: torch.Tensor) -> None:
    """Greedy decode tail in two launches (multi-workgroup argmax + state feed-back):
    t = argmax(logits, -1); out[:, step] = t; tokens = t; positions += 1; cache_len += 1; step += 1.
    `slot` is int64 [B] scratch that must be zero on entry (the kernel leaves it zeroed)."""
    if use_native(logits):
        ext().greedy_advance(logits if logits.stride(-1) == 1 else logits.contiguous(), slot, out, step,
                             tokens.view(-1), positions.view(-1), cache_len.view(-1))
        return
    t = torch.argmax(logits, dim=-1)
    B = logits.shape[0]
    out.scatter_(1, step.view(1, 1).expand(B, 1), t.view(B, 1))
    tokens.copy_(t.view(tokens.shape))
    positions.add_(1)
    cache_len.add_(1)
    step.add_(1)


def topk_sample(x: torch.Tensor, top_k: int, temperature: float = 1.0, uniform: Optional[torch.Tensor] = None,
                return_topk: bool = False):
    """Multinomial sampling among the top-k logits (reference Sampler.multinomial semantics:
    softmax over the sorted top-k, CDF, count entries below a uniform draw)."""
    B = x.shape[0]
    if uniform is None:
        uniform = torch.rand(B, device=x.device, dtype=torch.float32)
    if use_native(x):
        out = torch.empty(B, dtype=torch.int64, device=x.device)
        vals = torch.empty((B, top_k), dtype=torch.float32, device=x.device) if return_topk else None
        idx = torch.empty((B, top_k), dtype=torch.int64, device=x.device) if return_topk else None
        ext().topk_sample(x if x.stride(-1) == 1 else x.contiguous(), int(top_k), float(temperature), uniform.float(), out,
                          vals, idx)
        return (out, vals, idx) if return_topk else out
    v, i = torch.topk(x.float(), top_k, dim=-1)
    p = torch.softmax(v / (temperature if temperature > 0 else 1.0), dim=-1)
    cdf = torch.cumsum(p, -1)
    pick = (cdf < uniform[:, None]).sum(-1).clamp(max=top_k - 1)
    out = i.gather(1, pick[:, None]).squeeze(1)
    return (out, v, i) if return_topk else out
