"""The argument contract of the decode-attention bindings: every malformed call stops in a host-side
check with its message, before any kernel is launched.  Accepted calls are covered by the kernel,
sliding-window, MXFP8-cache and inference tests."""
import pytest
import torch

from neuronx_distributed_llama3_2_amd.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, T, HQ, HKV, D, LMAX = 2, 1, 4, 2, 64, 128
SENTINEL = 3.0


def _bf16(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16, device=DEV)


def _u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8, device=DEV)


def _attn(native, **kw):
    """decode_attn at the module's shapes with the given arguments replaced; returns `out`."""
    q = kw.pop("q", None)
    if q is None:
        q = _bf16(B, T, HQ, D)
    a = dict(q=q, k_cache=_bf16(B, HKV, LMAX, D), v_cache=_bf16(B, HKV, LMAX, D), cache_idx=None,
             seq_len=torch.full((B,), 7, dtype=torch.int32, device=DEV), out=torch.full_like(q, SENTINEL),
             scale=D ** -0.5, nsplit=1, window=0)
    a.update(kw)
    try:
        native.decode_attn(**a)
    finally:
        torch.cuda.synchronize()
        assert bool((a["out"] == SENTINEL).all()), "a rejected call wrote the output"
    return a["out"]


def _mx8(rows=B, d=D):
    return dict(k_cache=_u8(rows, HKV, LMAX, d), v_cache=_u8(rows, HKV, LMAX, d),
                k_scale=_u8(rows, HKV, LMAX, d // 32), v_scale=_u8(rows, HKV, LMAX, d // 32))


def _oproj(native, **kw):
    """decode_attn_oproj at the module's shapes (Hout = 256); returns (result, oacc)."""
    q = kw.pop("q", None)
    if q is None:
        q = _bf16(B, T, HQ, D)
    a = dict(q=q, k_cache=_bf16(B, HKV, LMAX, D), v_cache=_bf16(B, HKV, LMAX, D), cache_idx=None,
             seq_len=torch.full((B,), 7, dtype=torch.int32, device=DEV), wo=_bf16(256, HQ * D),
             oacc=torch.zeros(q.shape[0] * q.shape[1], 256, dtype=torch.float32, device=DEV), scale=D ** -0.5, window=0)
    a.update(kw)
    try:
        r = native.decode_attn_oproj(**a)
    finally:
        torch.cuda.synchronize()
        assert not bool(a["oacc"].any()), "a call that launched nothing changed oacc"
    return r, a["oacc"]


def _write(native, **kw):
    a = dict(k=_bf16(B, T, HKV, D), v=_bf16(B, T, HKV, D), k_cache=_bf16(B, HKV, LMAX, D), v_cache=_bf16(B, HKV, LMAX, D),
             cache_idx=None, pos=torch.zeros(B, dtype=torch.int32, device=DEV))
    a.update(kw)
    native.kv_cache_write(**a)


def test_decode_attention_argument_contract():
    assert _ext.ext_available(), "HIP extension must be built for GPU tests"
    native = _ext.ext()
    idx_long = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    small = dict(k_cache=_bf16(B - 1, HKV, LMAX, D), v_cache=_bf16(B - 1, HKV, LMAX, D))

    # ---- decode_attn, either cache format
    with pytest.raises(RuntimeError, match="go together"):
        _attn(native, k_scale=_u8(B, HKV, LMAX, D // 32))
    for cache in ({}, _mx8()):
        with pytest.raises(RuntimeError, match=r"nsplit \* 128 must cover the cache length"):
            _attn(native, nsplit=0, **cache)
        with pytest.raises(RuntimeError, match=r"window must be >= 0"):
            _attn(native, window=-1, **cache)
        with pytest.raises(RuntimeError, match=r"seq_len must be int32 \[B\]"):
            _attn(native, seq_len=torch.full((B,), 7, dtype=torch.int64, device=DEV), **cache)
        with pytest.raises(RuntimeError, match=r"cache_idx must be int32 \[B\]"):
            _attn(native, cache_idx=idx_long, **cache)
        with pytest.raises(RuntimeError, match="out shape mismatch"):
            _attn(native, out=torch.full((B, T + 1, HQ, D), SENTINEL, dtype=torch.bfloat16, device=DEV), **cache)
    with pytest.raises(RuntimeError, match="cache batch too small"):
        _attn(native, **small)
    with pytest.raises(RuntimeError, match="cache batch too small"):
        _attn(native, **_mx8(rows=B - 1))
    with pytest.raises(RuntimeError, match="head dim mismatch"):
        _attn(native, k_cache=_bf16(B, HKV, LMAX, 128), v_cache=_bf16(B, HKV, LMAX, 128))
    with pytest.raises(RuntimeError, match="head dim mismatch"):
        _attn(native, **_mx8(d=128))
    # ---- decode_attn, the rules of the bf16 cache
    with pytest.raises(RuntimeError, match=r"\(64/128\)"):
        _attn(native, q=_bf16(B, T, HQ, 32), k_cache=_bf16(B, HKV, LMAX, 32), v_cache=_bf16(B, HKV, LMAX, 32))
    with pytest.raises(RuntimeError, match="q heads must be a multiple of kv heads"):
        _attn(native, q=_bf16(B, T, 3, D))
    with pytest.raises(RuntimeError, match=r"\(Hq/Hkv\) \* new_tokens <= 64"):
        _attn(native, q=_bf16(B, 33, HQ, D))

    # ---- decode_attn_oproj
    with pytest.raises(RuntimeError, match=r"wo must be \[Hout, Hq \* D\]"):
        _oproj(native, wo=_bf16(256, HQ * D + 8))
    with pytest.raises(RuntimeError, match="oacc must be fp32 contiguous"):
        _oproj(native, oacc=_bf16(B * T, 256))
    with pytest.raises(RuntimeError, match=r"window must be >= 0"):
        _oproj(native, window=-1)
    with pytest.raises(RuntimeError, match=r"seq_len must be int32 \[B\]"):
        _oproj(native, seq_len=torch.full((B,), 7, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match=r"cache_idx must be int32 \[B\]"):
        _oproj(native, cache_idx=idx_long)
    with pytest.raises(RuntimeError, match="cache batch too small"):
        _oproj(native, **small)
    with pytest.raises(RuntimeError, match="head dim mismatch"):
        _oproj(native, k_cache=_bf16(B, HKV, LMAX, 128), v_cache=_bf16(B, HKV, LMAX, 128))
    # (Hq / Hkv) * T = 20 query rows per kv head: more than the fused kernel's 16, so nothing is launched
    r, oacc = _oproj(native, q=_bf16(B, 10, HQ, D))
    assert r is False and not bool(oacc.any())

    # ---- kv_cache_write, either cache format
    with pytest.raises(RuntimeError, match="go together"):
        _write(native, k_scale=_u8(B, HKV, LMAX, D // 32))
    for cache in ({}, _mx8()):
        with pytest.raises(RuntimeError, match=r"cache_idx must be int32 \[B\]"):
            _write(native, cache_idx=idx_long, **cache)
    with pytest.raises(RuntimeError, match="cache batch too small"):
        _write(native, **small)
    with pytest.raises(RuntimeError, match="cache batch too small"):
        _write(native, **_mx8(rows=B - 1))
