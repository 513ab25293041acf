"""Interval masks for flash attention: every query sees one contiguous interval of keys.

Query `q` of batch row `b` sees key `k` iff `lo[b, q] <= k < hi[b, q]` (and, under `causal`, also
`k <= q + causal_offset`).  Packed documents, right padding and sliding windows are all of this
form.  Contract: `lo` and `hi` are each non-decreasing along `q`; `hi <= lo` is an empty row
(output 0, LSE -inf, zero gradients).

Under that contract the queries that see a given key are one interval too,
`q_lo[b, k] <= q < q_hi[b, k]`, with

    q_hi = searchsorted(lo, k, right=True)     (queries whose lo <= k are a prefix)
    q_lo = searchsorted(hi, k, right=True)     (queries whose hi <= k are a prefix)

which the backward kernel consumes (it keeps the key on the lane).  Everything here runs on the
tensors' device without a host sync, except `validate` on GPU tensors, which is opt-in
(`NXD_ATTN_RANGE_CHECK=1`).
"""

from __future__ import annotations

import os
from typing import Optional

import torch


class KeyRanges:
    """(lo, hi) int32 [B, Sq] over `num_keys` keys, plus the transposed (q_lo, q_hi) int32 [B, Sk],
    built on first use and shared by every layer that receives this object."""

    __slots__ = ("lo", "hi", "num_keys", "_q_lo", "_q_hi", "_checked")

    def __init__(self, lo: torch.Tensor, hi: torch.Tensor, num_keys: int, q_lo: Optional[torch.Tensor] = None,
                 q_hi: Optional[torch.Tensor] = None):
        if lo.dim() != 2 or lo.shape != hi.shape:
            raise ValueError(f"lo / hi must be [B, Sq] of one shape, got {tuple(lo.shape)} and {tuple(hi.shape)}")
        self.lo = lo.to(torch.int32).contiguous()
        self.hi = hi.to(torch.int32).contiguous()
        self.num_keys = int(num_keys)
        self._q_lo = q_lo
        self._q_hi = q_hi
        self._checked = False

    @property
    def batch(self) -> int:
        return self.lo.shape[0]

    @property
    def num_queries(self) -> int:
        return self.lo.shape[1]

    @property
    def device(self):
        return self.lo.device

    def transposed(self):
        """(q_lo, q_hi) int32 [B, Sk]: key k is seen by the queries [q_lo[b, k], q_hi[b, k])."""
        if self._q_lo is None:
            keys = torch.arange(self.num_keys, device=self.lo.device, dtype=torch.int32).expand(self.batch, -1).contiguous()
            self._q_hi = torch.searchsorted(self.lo, keys, right=True).to(torch.int32).contiguous()
            self._q_lo = torch.searchsorted(self.hi, keys, right=True).to(torch.int32).contiguous()
        return self._q_lo, self._q_hi

    @property
    def q_lo(self) -> torch.Tensor:
        return self.transposed()[0]

    @property
    def q_hi(self) -> torch.Tensor:
        return self.transposed()[1]

    def __getitem__(self, rows) -> "KeyRanges":
        """Batch rows `rows` (a slice), e.g. one part of a split micro-batch."""
        if not isinstance(rows, slice):
            raise TypeError("KeyRanges is indexed by a slice of batch rows")
        out = KeyRanges(self.lo[rows], self.hi[rows], self.num_keys,
                        None if self._q_lo is None else self._q_lo[rows].contiguous(),
                        None if self._q_hi is None else self._q_hi[rows].contiguous())
        out._checked = self._checked
        return out

    def to(self, device) -> "KeyRanges":
        out = KeyRanges(self.lo.to(device), self.hi.to(device), self.num_keys,
                        None if self._q_lo is None else self._q_lo.to(device),
                        None if self._q_hi is None else self._q_hi.to(device))
        out._checked = self._checked
        return out

    def dense_mask(self, causal: bool = False, causal_offset: Optional[int] = None) -> torch.Tensor:
        """bool [B, Sq, Sk], True where the query sees the key (reference paths and tests)."""
        Sq, Sk = self.num_queries, self.num_keys
        ki = torch.arange(Sk, device=self.lo.device)[None, None, :]
        m = (ki >= self.lo[:, :, None]) & (ki < self.hi[:, :, None])
        if causal:
            off = Sk - Sq if causal_offset is None else causal_offset
            qi = torch.arange(Sq, device=self.lo.device)[None, :, None]
            m = m & (ki <= qi + off)
        return m


def validate(ranges: KeyRanges) -> None:
    """Raise ValueError unless lo / hi are non-decreasing along the query and 0 <= lo, hi <= Sk.
    Always checked for CPU tensors; for GPU tensors only with NXD_ATTN_RANGE_CHECK=1 (it syncs)."""
    if ranges._checked:
        return
    if ranges.lo.is_cuda and os.environ.get("NXD_ATTN_RANGE_CHECK", "0") != "1":
        return
    lo, hi = ranges.lo, ranges.hi
    if lo.shape[1] > 1:
        if bool((lo[:, 1:] < lo[:, :-1]).any()):
            raise ValueError("key ranges: lo must be non-decreasing along the query")
        if bool((hi[:, 1:] < hi[:, :-1]).any()):
            raise ValueError("key ranges: hi must be non-decreasing along the query")
    if lo.numel() and (bool((lo < 0).any()) or bool((hi > ranges.num_keys).any())):
        raise ValueError(f"key ranges: need 0 <= lo and hi <= {ranges.num_keys}")
    ranges._checked = True


def ranges_from_document_starts(is_start: torch.Tensor) -> KeyRanges:
    """is_start: bool [B, S], True where a document begins (position 0 always begins one).
    lo = start of the query's document, hi = S (combine with causal=True)."""
    B, S = is_start.shape
    idx = torch.arange(S, device=is_start.device, dtype=torch.int32).expand(B, S)
    lo = torch.cummax(torch.where(is_start.bool(), idx, torch.zeros_like(idx)), dim=1).values
    hi = torch.full_like(lo, S)
    return KeyRanges(lo, hi, S)


def ranges_from_eos(input_ids: torch.Tensor, eos_token_id: int) -> KeyRanges:
    """A document ends with its EOS token; the next token starts a new one."""
    is_start = torch.zeros_like(input_ids, dtype=torch.bool)
    is_start[:, 1:] = input_ids[:, :-1] == eos_token_id
    return ranges_from_document_starts(is_start)


def ranges_from_cu_seqlens(cu_seqlens: torch.Tensor, B: int, S: int) -> KeyRanges:
    """cu_seqlens: cumulative document offsets [0, ..., B * S] into the flattened [B * S] token
    stream.  A document that crosses a row boundary is cut there (rows do not see each other)."""
    flat = torch.zeros(B * S + 1, dtype=torch.bool, device=cu_seqlens.device)
    flat[cu_seqlens.long().clamp(0, B * S)] = True
    return ranges_from_document_starts(flat[: B * S].view(B, S))


def ranges_from_lengths(lengths: torch.Tensor, Sq: int, Sk: int, empty_padded_queries: bool = False) -> KeyRanges:
    """Right padding: row b has lengths[b] valid keys.  lo = 0, hi = length; with
    `empty_padded_queries` the query rows q >= length are empty (lo = hi = length)."""
    B = lengths.shape[0]
    ln = lengths.to(torch.int32).clamp(0, Sk)[:, None].expand(B, Sq)
    lo = torch.zeros_like(ln)
    if empty_padded_queries:
        q = torch.arange(Sq, device=lengths.device, dtype=torch.int32)[None, :]
        lo = torch.where(q >= ln, ln, lo)
    return KeyRanges(lo, ln, Sk)


def ranges_sliding_window(B: int, S: int, window: int, device=None) -> KeyRanges:
    """Each query sees itself and the window - 1 keys before it."""
    q = torch.arange(S, device=device, dtype=torch.int32)
    lo = (q - window + 1).clamp(min=0).expand(B, S)
    hi = (q + 1).expand(B, S)
    return KeyRanges(lo, hi, S)


def intersect_ranges(a: KeyRanges, b: KeyRanges) -> KeyRanges:
    """Keys both masks show: lo = max, hi = min (e.g. a sliding window inside packed documents).
    The maximum / minimum of non-decreasing sequences is non-decreasing, so the contract holds."""
    if (a.batch, a.num_queries, a.num_keys) != (b.batch, b.num_queries, b.num_keys):
        raise ValueError(f"cannot intersect key ranges of [B, Sq, Sk] = [{a.batch}, {a.num_queries}, {a.num_keys}] "
                         f"and [{b.batch}, {b.num_queries}, {b.num_keys}]")
    if a.device != b.device:
        raise ValueError(f"cannot intersect key ranges on {a.device} and {b.device}")
    return KeyRanges(torch.maximum(a.lo, b.lo), torch.minimum(a.hi, b.hi), a.num_keys)


def positions_from_ranges(ranges: KeyRanges) -> torch.Tensor:
    """q - lo[q] (int32 [B, S]): positions that restart at every document start."""
    q = torch.arange(ranges.num_queries, device=ranges.lo.device, dtype=torch.int32)[None, :]
    return q - ranges.lo
