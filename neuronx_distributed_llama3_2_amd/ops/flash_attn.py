"""Flash attention (fwd + bwd) on the CDNA4 kernels in csrc/flash_attn_{fwd,bwd}.hip.

API parity with the reference `nki_flash_attn_func` (src/neuronx_distributed/kernels/flash_attn.py:151-191)
but without its restrictions: any sequence length (the reference needs multiples of 2048), GQA
without `repeat_kv`, arbitrary strides (reads Q/K/V straight out of a fused QKV buffer), D = 64/128.

Also provides `rope_attention`, the training attention core used by the Llama model: RoPE applied
in place to the fused [S, B, (Hq+2Hkv)*D] QKV projection output, flash attention over strided
views of it, and a backward that writes dQ/dK/dV straight back into one fused dQKV buffer and
un-rotates it in place — no transposes, no repeat_kv, no separate q/k/v copies.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from ._ext import ext, use_native
from .attention_ranges import KeyRanges, validate
from .rope import rope_inplace_


def _checked_ranges(key_ranges: Optional[KeyRanges], B: int, Sq: int, Sk: int, device) -> Optional[KeyRanges]:
    """Shape / device / contract check of an interval mask against the attention problem."""
    if key_ranges is None:
        return None
    if not isinstance(key_ranges, KeyRanges):
        raise TypeError("key_ranges must be an ops.attention_ranges.KeyRanges")
    if (key_ranges.batch, key_ranges.num_queries, key_ranges.num_keys) != (B, Sq, Sk):
        raise ValueError(f"key_ranges is for [B, Sq, Sk] = [{key_ranges.batch}, {key_ranges.num_queries}, "
                         f"{key_ranges.num_keys}], attention is [{B}, {Sq}, {Sk}]")
    if key_ranges.device != device:
        raise ValueError(f"key_ranges is on {key_ranges.device}, attention on {device}")
    validate(key_ranges)
    return key_ranges


def attention_reference(q, k, v, causal: bool = True, softmax_scale: Optional[float] = None, causal_offset: Optional[int] = None,
                        key_ranges: Optional[KeyRanges] = None):
    """Plain fp32 reference. q: [B, Sq, Hq, D], k/v: [B, Sk, Hkv, D] -> (o [B, Sq, Hq, D], lse [B, Hq, Sq]).
    key_ranges: interval mask (ops/attention_ranges.py); an empty row gives o = 0, lse = -inf."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    g = Hq // Hkv
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        off = Sk - Sq if causal_offset is None else causal_offset
        qi = torch.arange(Sq, device=q.device)[:, None]
        ki = torch.arange(Sk, device=q.device)[None, :]
        s = s.masked_fill(ki > qi + off, float("-inf"))
    if key_ranges is not None:
        key_ranges = _checked_ranges(key_ranges, B, Sq, Sk, q.device)
        s = s.masked_fill(~key_ranges.dense_mask()[:, None], float("-inf"))
        # rows with no visible key: softmax over zeros instead of over -inf (whose gradient is NaN),
        # then the row is zeroed -- o = 0, lse = -inf, zero gradients
        dead = torch.isneginf(s).all(dim=-1, keepdim=True)
        lse = torch.logsumexp(s, dim=-1)
        p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
        o = torch.matmul(p, vf).permute(0, 2, 1, 3)
        return o, lse
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)
    o = torch.matmul(p, vf).permute(0, 2, 1, 3)
    return o, lse


_NO_DROPOUT = (0.0, 0, 0)


def _fwd(q, k, v, causal, scale, causal_offset, out=None, dropout=_NO_DROPOUT, key_ranges=None):
    B, Sq, Hq, D = q.shape
    o = out if out is not None else torch.empty(q.shape, dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device)
    if key_ranges is None:
        ext().flash_attn_fwd(q, k, v, o, lse, float(scale), bool(causal), int(causal_offset), *dropout)
    else:
        ext().flash_attn_fwd(q, k, v, o, lse, float(scale), bool(causal), int(causal_offset), *dropout,
                             key_ranges.lo, key_ranges.hi)
    return o, lse


def _bwd(q, k, v, o, do, lse, dq, dk, dv, scale, causal, causal_offset, dropout=_NO_DROPOUT, key_ranges=None):
    if key_ranges is None:
        ext().flash_attn_bwd(q, k, v, o, do, lse, dq, dk, dv, float(scale), bool(causal), int(causal_offset), *dropout)
    else:
        q_lo, q_hi = key_ranges.transposed()
        ext().flash_attn_bwd(q, k, v, o, do, lse, dq, dk, dv, float(scale), bool(causal), int(causal_offset), *dropout,
                             key_ranges.lo, key_ranges.hi, q_lo, q_hi)


class FlashAttnFunc(torch.autograd.Function):
    """dropout = (p, seed, head_offset): dropout on the probabilities inside both kernels (keep mask
    hashed from (seed, batch, global head, query, key) -- ops/attention_dropout.dropout_keep_mask --
    so nothing is stored and the backward regenerates it).
    range_lo .. range_q_hi: the four tensors of a KeyRanges (or all None); no gradients."""

    @staticmethod
    def forward(ctx, q, k, v, causal, softmax_scale, causal_offset, dropout=_NO_DROPOUT, range_lo=None, range_hi=None,
                range_q_lo=None, range_q_hi=None):
        kr = None if range_lo is None else KeyRanges(range_lo, range_hi, k.shape[1], range_q_lo, range_q_hi)
        o, lse = _fwd(q, k, v, causal, softmax_scale, causal_offset, dropout=dropout, key_ranges=kr)
        if kr is None:
            ctx.save_for_backward(q, k, v, o, lse)
        else:
            ctx.save_for_backward(q, k, v, o, lse, kr.lo, kr.hi, kr.q_lo, kr.q_hi)
        ctx.causal, ctx.scale, ctx.off, ctx.dropout = causal, softmax_scale, causal_offset, dropout
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors[:5]
        kr = KeyRanges(*ctx.saved_tensors[5:7], k.shape[1], *ctx.saved_tensors[7:9]) if len(ctx.saved_tensors) > 5 else None
        do = do if do.stride(-1) == 1 else do.contiguous()
        dq = torch.empty_like(q, memory_format=torch.contiguous_format)
        dk = torch.empty_like(k, memory_format=torch.contiguous_format)
        dv = torch.empty_like(v, memory_format=torch.contiguous_format)
        _bwd(q, k, v, o, do, lse, dq, dk, dv, ctx.scale, ctx.causal, ctx.off, ctx.dropout, kr)
        return dq, dk, dv, None, None, None, None, None, None, None, None


def flash_attn_func(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
                    softmax_scale: Optional[float] = None, causal_offset: Optional[int] = None,
                    dropout_p: float = 0.0, seed: Optional[int] = None, head_offset: int = 0,
                    key_ranges: Optional[KeyRanges] = None) -> torch.Tensor:
    """q: [B, Sq, Hq, D], k/v: [B, Sk, Hkv, D] (bf16, unit stride on D) -> o [B, Sq, Hq, D].
    dropout_p > 0: dropout on the attention probabilities (inverted scaling), mask from `seed`
    with local head h drawn as global head head_offset + h (tensor-parallel ranks).
    key_ranges: interval mask (ops/attention_ranges.py: packed documents, right padding, sliding
    windows), applied on top of `causal`; not available together with dropout."""
    D = q.shape[-1]
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    off = (k.shape[1] - q.shape[1]) if causal_offset is None else causal_offset
    if key_ranges is not None:
        if dropout_p:
            raise ValueError("key_ranges cannot be combined with attention dropout")
        kr = _checked_ranges(key_ranges, q.shape[0], q.shape[1], k.shape[1], q.device)
        if use_native(q, k, v):
            return FlashAttnFunc.apply(q, k, v, causal, scale, off, _NO_DROPOUT, kr.lo, kr.hi, kr.q_lo, kr.q_hi)
        o, _ = attention_reference(q, k, v, causal, scale, off, key_ranges=kr)
        return o.to(q.dtype)
    if dropout_p:
        from .attention_dropout import attention_with_dropout

        if causal_offset is not None and causal_offset != k.shape[1] - q.shape[1]:
            raise ValueError("dropout attention supports the bottom-right causal alignment only")
        o = attention_with_dropout(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), dropout_p, causal=causal,
                                   softmax_scale=scale, seed=seed, head_offset=head_offset)
        return o.transpose(1, 2)
    if use_native(q, k, v):
        return FlashAttnFunc.apply(q, k, v, causal, scale, off)
    o, _ = attention_reference(q, k, v, causal, scale, off)
    return o.to(q.dtype)


def flash_attn_fwd_lse(q, k, v, causal=True, softmax_scale=None, causal_offset=None, out=None, key_ranges=None):
    """Forward only, returning (o, lse) — used by inference prefill and ring/segment merges."""
    D = q.shape[-1]
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    off = (k.shape[1] - q.shape[1]) if causal_offset is None else causal_offset
    key_ranges = _checked_ranges(key_ranges, q.shape[0], q.shape[1], k.shape[1], q.device)
    if use_native(q, k, v):
        return _fwd(q, k, v, causal, scale, off, out=out, key_ranges=key_ranges)
    o, lse = attention_reference(q, k, v, causal, scale, off, key_ranges=key_ranges)
    o = o.to(q.dtype)
    if out is not None:
        out.copy_(o)
        o = out
    return o, lse


# --------------------------------------------------------------------------------------------
# fused RoPE + attention core over a [S, B, (Hq + 2Hkv) * D] QKV projection output
# --------------------------------------------------------------------------------------------


def _views(qkv: torch.Tensor, nq: int, nkv: int, D: int):
    """[S, B, W] -> q [B, S, nq, D], k/v [B, S, nkv, D] strided views (no copies)."""
    S, B, W = qkv.shape
    st = qkv.stride()
    q = qkv.as_strided((B, S, nq, D), (st[1], st[0], D, 1), qkv.storage_offset())
    k = qkv.as_strided((B, S, nkv, D), (st[1], st[0], D, 1), qkv.storage_offset() + nq * D)
    v = qkv.as_strided((B, S, nkv, D), (st[1], st[0], D, 1), qkv.storage_offset() + (nq + nkv) * D)
    return q, k, v


class RopeAttentionFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos_t, sin_t, nq, nkv, D, causal, scale, position_offset, range_lo=None, range_hi=None,
                range_q_lo=None, range_q_hi=None, positions=None):
        S, B, W = qkv.shape
        flat = qkv.view(S * B, W)
        # rotate q and k heads (contiguous columns [0, (nq+nkv)*D)) in place; position = row // B,
        # or positions[b, s] for row s * B + b
        pos_rows = None if positions is None else positions.t().reshape(-1)
        if pos_rows is not None:
            rope_inplace_(flat, 0, nq + nkv, D, cos_t, sin_t, pos_rows)
        else:
            rope_inplace_(flat, 0, nq + nkv, D, cos_t, sin_t, None, pos_div=B, pos_mod=cos_t.shape[0]) if position_offset == 0 else \
                rope_inplace_(flat, 0, nq + nkv, D, cos_t, sin_t,
                              (torch.arange(S * B, device=qkv.device) // B + position_offset))
        ctx.mark_dirty(qkv)
        # the rotated qkv output is never differentiated through: do not let autograd zero-fill
        # a [S, B, W] gradient for it every layer
        ctx.set_materialize_grads(False)
        q, k, v = _views(qkv, nq, nkv, D)
        o = torch.empty((S, B, nq * D), dtype=qkv.dtype, device=qkv.device)
        o_v = o.view(S, B, nq, D).permute(1, 0, 2, 3)
        kr = None if range_lo is None else KeyRanges(range_lo, range_hi, S, range_q_lo, range_q_hi)
        _, lse = _fwd(q, k, v, causal, scale, 0, out=o_v, key_ranges=kr)
        ctx.save_for_backward(qkv, o, lse, cos_t, sin_t, *(() if kr is None else (kr.lo, kr.hi, kr.q_lo, kr.q_hi)))
        ctx.pos_rows = pos_rows
        ctx.meta = (nq, nkv, D, causal, scale, position_offset)
        return qkv, o

    @staticmethod
    def backward(ctx, _dqkv_unused, do):
        qkv, o, lse, cos_t, sin_t = ctx.saved_tensors[:5]
        nq, nkv, D, causal, scale, position_offset = ctx.meta
        S, B, W = qkv.shape
        kr = KeyRanges(*ctx.saved_tensors[5:7], S, *ctx.saved_tensors[7:9]) if len(ctx.saved_tensors) > 5 else None
        do = do.contiguous()
        q, k, v = _views(qkv, nq, nkv, D)
        o_v = o.view(S, B, nq, D).permute(1, 0, 2, 3)
        do_v = do.view(S, B, nq, D).permute(1, 0, 2, 3)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = _views(dqkv, nq, nkv, D)
        _bwd(q, k, v, o_v, do_v, lse, dq, dk, dv, scale, causal, 0, key_ranges=kr)
        flat = dqkv.view(S * B, W)
        if ctx.pos_rows is not None:
            rope_inplace_(flat, 0, nq + nkv, D, cos_t, sin_t, ctx.pos_rows, sign=-1.0)
        elif position_offset == 0:
            rope_inplace_(flat, 0, nq + nkv, D, cos_t, sin_t, None, pos_div=B, pos_mod=cos_t.shape[0], sign=-1.0)
        else:
            rope_inplace_(flat, 0, nq + nkv, D, cos_t, sin_t,
                          (torch.arange(S * B, device=qkv.device) // B + position_offset), sign=-1.0)
        return (dqkv,) + (None,) * 13


def rope_attention(qkv: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, nq: int, nkv: int, head_dim: int,
                   causal: bool = True, softmax_scale: Optional[float] = None, position_offset: int = 0,
                   key_ranges: Optional[KeyRanges] = None, positions: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention core of a Llama block.

    qkv: [S, B, (nq + 2 nkv) * D] output of the (column-parallel) QKV projection, q heads first,
    then k heads, then v heads.  Returns o: [S, B, nq * D].  `qkv` is rotated in place.
    key_ranges: interval mask over the S keys (ops/attention_ranges.py), on top of `causal`.
    positions: int [B, S] rotary positions (e.g. restarting per document); overrides position_offset.
    """
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(head_dim)
    S, B, W = qkv.shape
    key_ranges = _checked_ranges(key_ranges, B, S, S, qkv.device)
    if positions is not None and tuple(positions.shape) != (B, S):
        raise ValueError(f"positions must be [B, S] = [{B}, {S}], got {tuple(positions.shape)}")
    if use_native(qkv):
        assert qkv.is_contiguous(), "fused qkv must be contiguous"
        if key_ranges is None and positions is None:
            _, o = RopeAttentionFunc.apply(qkv, cos_t, sin_t, nq, nkv, head_dim, causal, scale, position_offset)
        else:
            kr = key_ranges
            _, o = RopeAttentionFunc.apply(qkv, cos_t, sin_t, nq, nkv, head_dim, causal, scale, position_offset,
                                           *((None,) * 4 if kr is None else (kr.lo, kr.hi, kr.q_lo, kr.q_hi)), positions)
        return o
    # reference path (CPU): out-of-place, differentiable through plain torch ops
    x = qkv.view(S, B, nq + 2 * nkv, head_dim)
    if positions is not None:
        pos = positions.t().long()   # [S, B]
        c = cos_t.to(qkv.device)[pos][:, :, None, :].float()
        s = sin_t.to(qkv.device)[pos][:, :, None, :].float()
    else:
        pos = torch.arange(S, device=qkv.device) + position_offset
        c = cos_t.to(qkv.device)[pos][:, None, None, :].float()
        s = sin_t.to(qkv.device)[pos][:, None, None, :].float()

    def rot(t):
        tf = t.float()
        t1, t2 = tf[..., : head_dim // 2], tf[..., head_dim // 2:]
        return torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], dim=-1).to(t.dtype)

    q = rot(x[:, :, :nq]).permute(1, 0, 2, 3)
    k = rot(x[:, :, nq:nq + nkv]).permute(1, 0, 2, 3)
    v = x[:, :, nq + nkv:].permute(1, 0, 2, 3)
    g = nq // nkv
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(g, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(g, dim=1)
    sc = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        mask = torch.ones(S, S, dtype=torch.bool, device=qkv.device).triu(1)
        sc = sc.masked_fill(mask, float("-inf"))
    if key_ranges is not None:
        sc = sc.masked_fill(~key_ranges.dense_mask()[:, None], float("-inf"))
        dead = torch.isneginf(sc).all(dim=-1, keepdim=True)   # empty rows: o = 0, no NaN gradient
        p = torch.softmax(sc.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    else:
        p = torch.softmax(sc, dim=-1)
    o = torch.matmul(p, vf)  # [B, H, S, D]
    return o.permute(2, 0, 1, 3).reshape(S, B, nq * head_dim).to(qkv.dtype)
