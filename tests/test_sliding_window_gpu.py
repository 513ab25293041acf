"""Sliding-window attention on MI355X: the windowed decode-attention kernels against the CPU
fallback, the fused attention + o_proj launches with a window, end-to-end generation of a windowed
model (graphed prefill + hipGraph decode), and windowed training against the reference ops."""

import os
import socket

import pytest
import torch
import torch.distributed as dist

import neuronx_distributed_llama3_2_amd.ops as ops
from neuronx_distributed_llama3_2_amd.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
L = 2304          # cache length: more than one 1,024-key split
POISON = 1e4      # finite (0 x V stays 0); one unmasked read would own the softmax


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _caches(B, Hkv, D, T, seq, window, seed):
    """Random caches with every slot outside each row's visible span [first key of the oldest new
    token, seq_len) overwritten by POISON."""
    g = torch.Generator().manual_seed(seed)
    kc = torch.randn(B, Hkv, L, D, generator=g)
    vc = torch.randn(B, Hkv, L, D, generator=g)
    pos = torch.arange(L)
    for b, s in enumerate(seq):
        lo = max(0, s - (T - 1) - window) if window and window < L else 0
        out = (pos < lo) | (pos >= s)
        kc[b, :, out] = POISON
        vc[b, :, out] = POISON
    return kc.to(torch.bfloat16), vc.to(torch.bfloat16)


@pytest.mark.parametrize("window", [1, 63, 64, 200, 1024])
@pytest.mark.parametrize("Hq,Hkv,T", [(8, 2, 1), (8, 2, 4), (8, 1, 3)])   # M = 4, 16 (MFMA kernel, its limit), 24 (chunk kernel)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_window(D, Hq, Hkv, T, window):
    """Native decode_attention(window=) against the CPU fallback (bound of
    test_decode_attention_mfma_groups).  Lengths: the whole cache, the shortest legal one (window not
    binding), window + T (the oldest new token's window starts exactly at key 1), and one whose window
    crosses the 1,024-key split edge."""
    assert _ext.ext_available(), "HIP extension must be built for GPU tests"
    B = 4
    seq = [L, T, window + T, 1029 + window]
    kc, vc = _caches(B, Hkv, D, T, seq, window, seed=window + T)
    torch.manual_seed(2)
    q = (torch.randn(B, T, Hq, D) * 2).to(torch.bfloat16)
    seq_t = torch.tensor(seq, dtype=torch.int32)
    ref = ops.decode_attention(q, kc, vc, seq_t, window=window)
    assert torch.isfinite(ref.float()).all() and ref.float().abs().max() < 10    # the oracle saw no poison
    o = ops.decode_attention(q.to(DEV), kc.to(DEV), vc.to(DEV), seq_t.to(DEV), window=window)
    assert torch.isfinite(o.float()).all()
    rel = _rel(o.cpu(), ref)
    # cache rows through a permuting cache_idx (continuous batching)
    idx = torch.tensor([3, 0, 2, 1], dtype=torch.int32)
    inv = torch.argsort(idx)
    o2 = ops.decode_attention(q.to(DEV), kc[inv].to(DEV), vc[inv].to(DEV), seq_t.to(DEV), idx.to(DEV), window=window)
    rel2 = _rel(o2.cpu(), ref)
    print(f"D {D} Hq {Hq} Hkv {Hkv} T {T} window {window}: rel {rel:.3e}, through cache_idx {rel2:.3e}")
    assert rel < 2e-2
    assert rel2 < 2e-2


@pytest.mark.parametrize("Hq,Hkv,T", [(8, 2, 1), (8, 2, 4), (8, 1, 3)])
def test_window_covering_the_cache_is_bitwise_no_window(Hq, Hkv, T):
    """window >= L and window=None are the same launches (two-launch path: split attention + merge,
    no atomics), and windowed calls in between leave the un-windowed results what they were."""
    D, B = 64, 4
    torch.manual_seed(3)
    kc = torch.randn(B, Hkv, L, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn(B, Hkv, L, D, device=DEV, dtype=torch.bfloat16)
    q = torch.randn(B, T, Hq, D, device=DEV, dtype=torch.bfloat16) * 2
    seq = torch.tensor([L, T, 1500, 777], device=DEV, dtype=torch.int32)
    golden = ops.decode_attention(q, kc, vc, seq).clone()
    windowed = ops.decode_attention(q, kc, vc, seq, window=200)
    assert not torch.equal(windowed, golden)
    for w in (None, 0, L, L + 5, 1 << 20):
        assert torch.equal(ops.decode_attention(q, kc, vc, seq, window=w), golden), w
    assert torch.equal(ops.decode_attention(q, kc, vc, seq, window=200), windowed)


@pytest.mark.parametrize("maxl", [1024, 256])    # one pass over the window / split attention + merge_oproj_kernel
@pytest.mark.parametrize("D,T", [(64, 1), (128, 1), (64, 4)])
def test_decode_attn_oproj_window_op(D, T, maxl):
    """The fused attention + o_proj launch itself, window 512 on the 2,304-key cache: it covers the
    shape (returns True) although the cache is past the one-pass limit, and its fp32 accumulator is
    o_proj of the windowed CPU attention (poisoned caches: it read nothing outside the window)."""
    native = _ext.ext()
    B, Hq, Hkv, window = 2, 8, 2, 512
    seq = [1800, window + T]
    kc, vc = _caches(B, Hkv, D, T, seq, window, seed=D + T)
    g = torch.Generator().manual_seed(4)
    q = (torch.randn(B, T, Hq, D, generator=g) * 2).to(torch.bfloat16)
    wo = (torch.randn(Hq * D, Hq * D, generator=g) * 0.05).to(torch.bfloat16)
    seq_t = torch.tensor(seq, dtype=torch.int32)
    att = ops.decode_attention(q, kc, vc, seq_t, window=window)                      # bf16-rounded, as the kernel's
    ref = att.reshape(B * T, Hq * D).float() @ wo.float().t()
    oacc = torch.zeros(8, Hq * D, dtype=torch.float32, device=DEV)
    native.decode_attn_set_oproj_maxl(maxl)
    try:
        ok = native.decode_attn_oproj(q.to(DEV), kc.to(DEV), vc.to(DEV), None, seq_t.to(DEV), wo.to(DEV), oacc,
                                      1.0 / D ** 0.5, window)
    finally:
        native.decode_attn_set_oproj_maxl(int(os.environ.get("NXD_DECODE_ATTN_OPROJ_MAXL", "1024")))
    assert ok, "the fused launch declined the windowed shape"
    rel = _rel(oacc[:B * T].cpu(), ref)
    print(f"D {D} T {T} one-pass limit {maxl}: rel {rel:.3e}")
    assert rel < 2e-2
    assert int((oacc[B * T:] != 0).sum()) == 0


# ---------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------

def _llama_cfg(hidden, window, max_pos=4096):
    from transformers import LlamaConfig

    cfg = LlamaConfig(hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=2, vocab_size=1000, max_position_embeddings=max_pos, rms_norm_eps=1e-5,
                      rope_theta=500000.0, tie_word_embeddings=True, eos_token_id=2)
    cfg.sliding_window = window
    return cfg


def _state(cfg, seed=0):
    from transformers import LlamaForCausalLM as HF

    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in HF(cfg).state_dict().items()}


def _model(cfg, sd, dtype, device, graphs=True, steps=8, seq_len=256, ctx=128, **kw):
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    icfg = InferenceConfig(batch_size=2, seq_len=seq_len, max_context_length=ctx, use_hip_graphs=graphs,
                           decode_graph_steps=steps, **kw)
    m = LlamaForCausalLMInference(cfg, icfg, dtype=dtype, device=device, init_weights=False)
    m._load_full(hf_to_nxd(sd, cfg))
    return m


@pytest.mark.parametrize("hidden", [512, 1024])   # head_dim 64, 128
def test_fused_attention_oproj_with_window(monkeypatch, hidden):
    """sliding_window = 512 on a 2,304-key cache filled to ~1,800: the window's key span fits the
    one-pass attention + o_proj launch; with the one-pass limit at 256 keys the windowed split
    attention + merge_oproj_kernel form runs.  One decode step each against the two-launch path on
    identical caches (bound of test_fused_attention_oproj_long_context); accumulator left zero."""
    from neuronx_distributed_llama3_2_amd.inference import model_base

    native = _ext.ext()
    cfg = _llama_cfg(hidden, 512)
    sd = _state(cfg)
    torch.manual_seed(7)
    P = 1800
    ids = torch.randint(3, cfg.vocab_size, (2, P))
    m = _model(cfg, sd, torch.bfloat16, torch.device(DEV), graphs=False, steps=1, seq_len=2304, ctx=2048)
    assert m.model.sliding_window == 512 and m.model._decode_window() == 512
    m.generate(ids, max_new_tokens=2, eos_token_id=-1)    # fills the cache with P + 1 positions
    f = m.model
    last = torch.randint(3, cfg.vocab_size, (2, 1), device=DEV)
    pos = torch.full((2, 1), P + 1, dtype=torch.int64, device=DEV)
    sid = torch.arange(2, device=DEV)
    clen = torch.full((2,), P + 2, dtype=torch.int32, device=DEV)
    saved = f.kv_cache.clone()

    def step(fuse, maxl, window=512):
        f.kv_cache.copy_(saved)
        f.sliding_window = window
        monkeypatch.setattr(model_base, "_ATTN_OPROJ", fuse)
        native.decode_attn_set_oproj_maxl(maxl)
        try:
            out = f.forward_tokens(last, pos, sid, clen).float()
        finally:
            native.decode_attn_set_oproj_maxl(int(os.environ.get("NXD_DECODE_ATTN_OPROJ_MAXL", "1024")))
            f.sliding_window = 512
        if fuse:
            buf = getattr(f, "_oacc_buf", None)
            assert buf is not None and int((buf != 0).sum()) == 0, "fused path not taken or accumulator not consumed"
        return out

    lu = step(False, 1024)
    one_pass = step(True, 1024)
    split = step(True, 256)
    no_window = step(False, 1024, window=0)
    r1, r2, r0 = _rel(one_pass, lu), _rel(split, lu), _rel(no_window, lu)
    print(f"hidden {hidden}: one pass {r1:.3e}, split + merge_oproj {r2:.3e}; without the window {r0:.3e}")
    assert r1 < 2e-2
    assert r2 < 2e-2


def test_windowed_generation_graphs_match_eager_and_fp32_cpu():
    """W = 16, prompt 40, 24 new tokens: graphed prefill + hipGraph decode give the eager tokens
    (deterministic=True: no fp32 atomics), and one bf16 decode step matches the fp32 CPU model on the
    same cache contents within the bf16-vs-fp32 bound of test_inference_gpu.py (3e-2 of the largest
    logit)."""
    cfg = _llama_cfg(512, 16, max_pos=1024)
    sd = _state(cfg)
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (2, 40))
    dev = torch.device(DEV)
    g = _model(cfg, sd, torch.bfloat16, dev, graphs=True, steps=8, deterministic=True, prefill_graphs=True)
    e = _model(cfg, sd, torch.bfloat16, dev, graphs=False, steps=1, deterministic=True, prefill_graphs=False)
    a = g.generate(ids, max_new_tokens=24, eos_token_id=-1).cpu()
    b = e.generate(ids, max_new_tokens=24, eos_token_id=-1).cpu()
    assert a.shape == (2, 64)
    assert g._prefill_cache, "the prefill graph was not used"
    assert len(g.model._prefill_ranges) == 1          # one ranges object per (batch, bucket), reused by the graph
    print(f"graph vs eager tokens equal: {(a == b).float().mean().item():.3f}")
    assert torch.equal(a, b), (a, b)
    # one decode step, bf16 kernels vs the fp32 CPU reference path, same cache contents
    cpu = _model(cfg, sd, torch.float32, torch.device("cpu"), graphs=False, steps=1)
    cpu.model.kv_cache.copy_(e.model.kv_cache.float().cpu())
    n = b.shape[1]
    last = b[:, -1:]
    pos = torch.full((2, 1), n - 1, dtype=torch.int64)
    sid = torch.arange(2)
    clen = torch.full((2,), n, dtype=torch.int32)
    lg = e.model.forward_tokens(last.to(dev), pos.to(dev), sid.to(dev), clen.to(dev)).float().cpu()
    lc = cpu.model.forward_tokens(last, pos, sid, clen).float()
    cpu.model.sliding_window = 0
    cpu.model.kv_cache.copy_(e.model.kv_cache.float().cpu())
    lc_plain = cpu.model.forward_tokens(last, pos, sid, clen).float()
    err = ((lg - lc).abs().max() / lc.abs().max()).item()
    off = ((lc_plain - lc).abs().max() / lc.abs().max()).item()
    print(f"bf16 gpu vs fp32 cpu, one windowed decode step: {err:.3e} (fp32 without the window: {off:.3e})")
    assert err < 3e-2, err


def _single_process():
    from neuronx_distributed_llama3_2_amd.parallel_layers import parallel_state as ps

    if not dist.is_initialized():
        dist.init_process_group("cpu:gloo,cuda:nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    if not ps.model_parallel_is_initialized():
        ps.initialize_model_parallel(1)


def _training_pair(kind):
    _single_process()
    if kind == "llama":
        from neuronx_distributed_llama3_2_amd.models.llama.modeling_llama import LlamaForCausalLM as cls, llama_config

        make = lambda w: llama_config("tiny", num_hidden_layers=2, hidden_size=256, intermediate_size=512,   # noqa: E731
                                      num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
                                      max_position_embeddings=512, **({"sliding_window": w} if w else {}))
    else:
        from neuronx_distributed_llama3_2_amd.models.mixtral import MixtralForCausalLM as cls, mixtral_config

        make = lambda w: mixtral_config("tiny", hidden_size=512, num_attention_heads=4, num_key_value_heads=2,   # noqa: E731
                                        intermediate_size=256, **({"sliding_window": w} if w else {}))
    torch.manual_seed(0)
    model = cls(make(48), dtype=torch.bfloat16, device=torch.device(DEV))
    plain = cls(make(None), dtype=torch.bfloat16, device=torch.device(DEV))
    plain.load_state_dict(model.state_dict())
    return model, plain


@pytest.mark.parametrize("kind", ["llama", "mixtral"])
def test_windowed_training_matches_reference_ops(monkeypatch, kind):
    """S = 256, W = 48, bf16: loss and qkv-weight gradients of the HIP kernels against the same model
    on the reference ops (NXD_FORCE_REFERENCE=1); gates of the model-level case in
    tests/test_attention_ranges_gpu.py (loss 2e-2 relative, gradient relative norm 5e-2)."""
    model, plain = _training_pair(kind)
    ids = torch.randint(0, 500, (2, 256), generator=torch.Generator().manual_seed(10)).to(DEV)

    def run(m):
        m.zero_grad()
        out = m(ids, labels=ids)
        out.loss.backward()
        return float(out.loss.detach()), {n: p.grad.float().clone() for n, p in m.named_parameters() if "qkv_proj" in n}

    loss, grads = run(model)
    loss_plain, _ = run(plain)
    monkeypatch.setenv("NXD_FORCE_REFERENCE", "1")
    ref_loss, ref_grads = run(model)
    monkeypatch.delenv("NXD_FORCE_REFERENCE")
    print(f"{kind}: loss kernels {loss:.5f} reference ops {ref_loss:.5f}; without the window {loss_plain:.5f}")
    assert grads and loss != loss_plain
    assert abs(loss - ref_loss) < 2e-2 * ref_loss, (loss, ref_loss)
    for n, gr in grads.items():
        rel = ((gr - ref_grads[n]).norm() / ref_grads[n].norm()).item()
        print(f"grad {n}: rel {rel:.3e}")
        assert rel < 5e-2, (n, rel)
