"""Sliding-window attention (`config.sliding_window`, Mistral / Mixtral) on the CPU reference paths:
range intersection, the windowed decode-attention fallback against a direct fp64 masked softmax,
HF parity of the training models and of inference prefill + decode, and the window combined with
document masking.

Window W: a query at absolute position p sees the keys k with p - W < k <= p."""

import socket

import pytest
import torch
import torch.distributed as dist

from neuronx_distributed_llama3_2_amd import ops
from neuronx_distributed_llama3_2_amd.ops import attention_ranges as ar

TOL = dict(atol=2e-4, rtol=2e-4)   # the HF-parity tolerance of tests/test_inference.py
W = 8


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _single_process():
    from neuronx_distributed_llama3_2_amd.parallel_layers import parallel_state as ps

    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    if not ps.model_parallel_is_initialized():
        ps.initialize_model_parallel(1)


# ---------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------

def test_intersect_ranges_is_the_and_of_the_masks():
    B, S = 2, 96
    is_start = torch.zeros(B, S, dtype=torch.bool)
    is_start[0, [0, 30, 31, 70]] = True
    is_start[1, [0, 50]] = True
    docs = ar.ranges_from_document_starts(is_start)
    for w in (1, 5, 40, 200):
        win = ar.ranges_sliding_window(B, S, w)
        both = ops.intersect_ranges(docs, win)
        ar.validate(both)
        assert both._checked
        for causal in (False, True):
            assert torch.equal(both.dense_mask(causal=causal), docs.dense_mask(causal=causal) & win.dense_mask(causal=causal))
        assert torch.equal(ops.intersect_ranges(win, docs).lo, both.lo)
    with pytest.raises(ValueError, match="intersect"):
        ops.intersect_ranges(docs, ar.ranges_sliding_window(B, S - 1, 4))


def _decode_reference(q, kc, vc, seq_len, window):
    """Direct fp64 masked softmax; a row without a visible key is 0."""
    B, T, Hq, D = q.shape
    g = Hq // kc.shape[1]
    L = kc.shape[2]
    out = torch.zeros(B, T, Hq, D, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            lim = int(seq_len[b]) - (T - 1 - t)
            lo = max(0, lim - window) if window and window < L else 0
            if lim <= lo:
                continue
            for h in range(Hq):
                k = kc[b, h // g, lo:lim].double()
                v = vc[b, h // g, lo:lim].double()
                p = torch.softmax(k @ q[b, t, h].double() / D ** 0.5, 0)
                out[b, t, h] = p @ v
    return out


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("window", [1, 5, 64, 96, 500])
def test_cpu_decode_attention_window(T, window):
    L, Hq, Hkv, D = 96, 4, 2, 16
    # seq_len < T (the first new tokens see nothing), < window, == window, == window + 1, ...
    lens = sorted({T - 1, T, window - 1, window, window + 1, window + T, 70, L} & set(range(0, L + 1)))
    B = len(lens)
    g = torch.Generator().manual_seed(window * 10 + T)
    q = torch.randn(B, T, Hq, D, generator=g)
    kc = torch.randn(B, Hkv, L, D, generator=g)
    vc = torch.randn(B, Hkv, L, D, generator=g)
    seq_len = torch.tensor(lens, dtype=torch.int32)
    got = ops.decode_attention(q, kc, vc, seq_len, window=window)
    want = _decode_reference(q, kc, vc, seq_len, window)
    err = (got.double() - want).abs().max().item()
    print(f"T {T} window {window} lengths {lens}: max abs error {err:.3e}")
    # fp32 against fp64 on unit-variance data: a few ulp of the 96-term sums
    torch.testing.assert_close(got.double(), want, atol=1e-5, rtol=1e-5)
    if window >= L:
        assert torch.equal(got, ops.decode_attention(q, kc, vc, seq_len))
    # through a permuting cache_idx
    perm = torch.randperm(B, generator=g)
    got_p = ops.decode_attention(q, kc[torch.argsort(perm)], vc[torch.argsort(perm)], seq_len, perm.to(torch.int32),
                                 window=window)
    assert torch.equal(got_p, got)
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, seq_len, window=-1)


# ---------------------------------------------------------------------------------------------
# HF parity: training models
# ---------------------------------------------------------------------------------------------

def _mistral_cfg(sliding_window):
    from transformers import MistralConfig

    return MistralConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=2, vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5,
                         rope_theta=10000.0, sliding_window=sliding_window, tie_word_embeddings=False, bos_token_id=1,
                         eos_token_id=2, attn_implementation="eager", torch_dtype="float32")


def _mixtral_cfg(sliding_window):
    from transformers import MixtralConfig

    return MixtralConfig(hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=2, vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5,
                         rope_theta=1e6, num_local_experts=4, num_experts_per_tok=2, sliding_window=sliding_window,
                         tie_word_embeddings=False, bos_token_id=1, eos_token_id=2, attn_implementation="eager",
                         torch_dtype="float32")


def _hf_mistral(cfg, seed=0):
    from transformers import MistralForCausalLM

    torch.manual_seed(seed)
    return MistralForCausalLM(cfg).eval()


def _hf_mixtral(cfg, seed=0):
    from transformers import MixtralForCausalLM

    torch.manual_seed(seed)
    m = MixtralForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "experts" in n:
                p.normal_(0.0, 0.1)
    return m


def _ids(n, seed=3, vocab=512, batch=1):
    return torch.randint(3, vocab, (batch, n), generator=torch.Generator().manual_seed(seed))


def _first_difference(a, b):
    """First position (dim 0) at which two [S, V] logits differ by more than the parity tolerance."""
    bad = ((a - b).abs() > TOL["atol"] + TOL["rtol"] * b.abs()).any(-1)
    return int(torch.nonzero(bad)[0]) if bool(bad.any()) else None


def _check_training_parity(make_cfg, make_hf, convert, model_cls):
    _single_process()
    cfg = make_cfg(W)
    hf = make_hf(cfg)
    ids = _ids(40)
    with torch.no_grad():
        ref = hf(ids).logits[0]                                   # [S, V]
        ref_plain = make_hf(make_cfg(None))(ids).logits[0]        # same seed: same weights, no window
    assert _first_difference(ref_plain, ref) == W                 # HF: position W - 1 unchanged, W changes
    sd = convert(hf.state_dict(), cfg)
    logits = {}
    for name, c in (("window", cfg), ("plain", make_cfg(None))):
        model = model_cls(c, dtype=torch.float32, device=torch.device("cpu")).eval()
        model.load_state_dict(sd)
        with torch.no_grad():
            logits[name] = model(ids).logits[:, 0].float()        # [S, V]
    print(f"max |ours - HF| with the window {(logits['window'] - ref).abs().max().item():.3e}, "
          f"without {(logits['plain'] - ref_plain).abs().max().item():.3e}")
    torch.testing.assert_close(logits["window"], ref, **TOL)
    torch.testing.assert_close(logits["plain"], ref_plain, **TOL)
    assert _first_difference(logits["plain"], logits["window"]) == W


def test_llama_training_matches_hf_mistral():
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd
    from neuronx_distributed_llama3_2_amd.models.llama.modeling_llama import LlamaForCausalLM

    _check_training_parity(_mistral_cfg, _hf_mistral, hf_to_nxd, LlamaForCausalLM)


def test_mixtral_training_matches_hf_mixtral():
    from neuronx_distributed_llama3_2_amd.models.mixtral import MixtralForCausalLM
    from neuronx_distributed_llama3_2_amd.models.mixtral.convert import mixtral_hf_to_nxd

    _check_training_parity(_mixtral_cfg, _hf_mixtral, mixtral_hf_to_nxd, MixtralForCausalLM)


def test_mixtral_explicit_key_ranges_and_checkpointing():
    """forward(key_ranges=) on a window-less config is the config's window; activation checkpointing
    carries the ranges."""
    from neuronx_distributed_llama3_2_amd.models.mixtral import MixtralForCausalLM, mixtral_config

    _single_process()
    ids = _ids(40, batch=2)
    torch.manual_seed(0)
    win = MixtralForCausalLM(mixtral_config("tiny", sliding_window=W), dtype=torch.float32, device=torch.device("cpu"))
    plain = MixtralForCausalLM(mixtral_config("tiny"), dtype=torch.float32, device=torch.device("cpu"))
    ckpt = MixtralForCausalLM(mixtral_config("tiny", sliding_window=W, activation_checkpoint="full"), dtype=torch.float32,
                              device=torch.device("cpu"))
    assert win.config.sliding_window == W and getattr(plain.config, "sliding_window", None) is None
    plain.load_state_dict(win.state_dict())
    ckpt.load_state_dict(win.state_dict())
    a = win(ids, labels=ids)
    b = plain(ids, labels=ids, key_ranges=ops.ranges_sliding_window(2, 40, W))
    c = ckpt(ids, labels=ids)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.loss, b.loss) and torch.equal(a.loss, c.loss)
    assert not torch.equal(a.logits, plain(ids).logits)
    a.loss.backward()
    c.loss.backward()
    qkv = [n for n, _ in win.named_parameters() if "qkv_proj" in n]
    ga, gc = dict(win.named_parameters()), dict(ckpt.named_parameters())
    assert qkv and all(ga[n].grad is not None and torch.equal(ga[n].grad, gc[n].grad) for n in qkv)


# ---------------------------------------------------------------------------------------------
# HF parity: inference prefill + decode
# ---------------------------------------------------------------------------------------------

def _inf_model(cfg, hf_sd, **kw):
    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    icfg = InferenceConfig(tp_degree=1, batch_size=1, seq_len=64, max_context_length=32, **kw)
    m = LlamaForCausalLMInference(cfg, icfg, dtype=torch.float32, init_weights=False)
    m._load_full(hf_to_nxd(hf_sd, cfg))
    return m


def _prefill_then_decode(m, ids, prompt, T):
    """Prefill ids[:, :prompt], then teacher-forced decode of the rest in chunks of T through
    forward_tokens.  Returns the logits after every token from prompt - 1 on: [n, V]."""
    m.reset()
    rows = [m._context_encode(ids[:, :prompt])[0]]
    sid = torch.zeros(1, dtype=torch.long)
    for p in range(prompt, ids.shape[1], T):
        pos = torch.arange(p, p + T).view(1, T)
        out = m.model.forward_tokens(ids[:, p:p + T], pos, sid, torch.tensor([p + T], dtype=torch.int32))
        rows.extend(out[0])
    return torch.stack(rows).float()


@pytest.fixture(scope="module")
def mistral_hf():
    cfg = _mistral_cfg(W)
    return cfg, _hf_mistral(cfg)


@pytest.mark.parametrize("T,steps", [(1, 16), (3, 18)])
def test_inference_prefill_and_decode_match_hf(mistral_hf, T, steps):
    """Prefill of 24 tokens (padded to the 32-token bucket), then `steps` teacher-forced tokens in
    chunks of T.  HF is causal, so its logits at position p of one forward over the whole sequence are
    those of a forward over the sequence extended up to p."""
    cfg, hf = mistral_hf
    prompt = 24
    ids = _ids(prompt + steps, seed=5)
    with torch.no_grad():
        ref = hf(ids).logits[0, prompt - 1:]
    m = _inf_model(cfg, hf.state_dict())
    assert m.model.sliding_window == W
    got = _prefill_then_decode(m, ids, prompt, T)
    err = (got - ref).abs().max(-1).values
    print(f"T {T}: max |ours - HF| per step {[f'{e:.1e}' for e in err.tolist()]}")
    torch.testing.assert_close(got, ref, **TOL)


def test_inference_window_not_binding_equals_no_window(mistral_hf):
    _, hf = mistral_hf
    ids = _ids(40, seed=6)
    outs = []
    for w in (64, None):
        m = _inf_model(_mistral_cfg(w), hf.state_dict())
        outs.append(_prefill_then_decode(m, ids, 24, 1))
    assert torch.equal(outs[0], outs[1])
    bound = _prefill_then_decode(_inf_model(_mistral_cfg(W), hf.state_dict()), ids, 24, 1)
    assert not torch.equal(bound, outs[1])


def test_medusa_with_binding_window_not_implemented(mistral_hf):
    from neuronx_distributed_llama3_2_amd.inference.medusa import MedusaDecoder, MedusaHeads

    cfg, hf = mistral_hf
    heads = MedusaHeads(cfg.hidden_size, cfg.vocab_size, 2, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="sliding window"):
        MedusaDecoder(_inf_model(cfg, hf.state_dict()), heads)
    MedusaDecoder(_inf_model(_mistral_cfg(None), hf.state_dict()), heads)
    MedusaDecoder(_inf_model(_mistral_cfg(4096), hf.state_dict()), heads)   # covers the cache: not binding


# ---------------------------------------------------------------------------------------------
# window + document masking
# ---------------------------------------------------------------------------------------------

EOS = 255


def _tiny_llama(**over):
    from neuronx_distributed_llama3_2_amd.models.llama.modeling_llama import LlamaForCausalLM, llama_config

    _single_process()
    cfg = llama_config("tiny", num_hidden_layers=2, hidden_size=128, intermediate_size=256, num_attention_heads=4,
                       num_key_value_heads=2, vocab_size=256, max_position_embeddings=128, **over)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg, dtype=torch.float32, device=torch.device("cpu")).eval()


def _packed_ids(seed=0):
    """Two rows of 96 tokens; row 0 holds documents [0, 30), [30, 31), [31, 70), [70, 96), row 1
    documents [0, 50), [50, 96)."""
    ids = torch.randint(0, EOS, (2, 96), generator=torch.Generator().manual_seed(seed))
    for row, ends in ((0, (29, 30, 69)), (1, (49,))):
        for e in ends:
            ids[row, e] = EOS
    return ids


def test_llama_window_with_document_masking():
    win = 12
    model = _tiny_llama(sliding_window=win, document_masking_eos_token_id=EOS, reset_position_ids=True)
    assert model.config.sliding_window == win
    plain = _tiny_llama()
    plain.load_state_dict(model.state_dict())
    ids = _packed_ids()
    docs = ops.ranges_from_eos(ids, EOS)
    both = ops.intersect_ranges(docs, ops.ranges_sliding_window(2, 96, win))
    # the mask is the intersection, the positions restart with the documents (not with the window)
    kr, pos = model._document_mask(ids, None, None)
    assert torch.equal(kr.lo, both.lo) and torch.equal(kr.hi, both.hi)
    assert torch.equal(pos, ops.positions_from_ranges(docs)) and int(pos.max()) > win
    grads = []
    outs = []
    for m, kw in ((model, {}), (plain, dict(key_ranges=both, position_ids=ops.positions_from_ranges(docs)))):
        m.zero_grad()
        out = m(ids, labels=ids, **kw)
        out.loss.backward()
        outs.append(out)
        grads.append(m.model.embed_tokens.weight.grad.clone())
    assert torch.equal(outs[0].loss, outs[1].loss) and torch.equal(outs[0].logits, outs[1].logits)
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0
    # either mask alone gives something else
    with torch.no_grad():
        assert not torch.equal(outs[0].logits, _with_state(model, document_masking_eos_token_id=EOS,
                                                           reset_position_ids=True)(ids).logits)
        assert not torch.equal(outs[0].logits, _with_state(model, sliding_window=win)(ids).logits)


def _with_state(model, **over):
    other = _tiny_llama(**over)
    other.load_state_dict(model.state_dict())
    return other


def test_llama_window_not_binding_is_the_plain_path():
    model = _tiny_llama(sliding_window=96)
    assert model._document_mask(_packed_ids(), None, None) == (None, None)
    assert model._document_mask(_packed_ids()[:, :40], None, None) == (None, None)
    kr, pos = _tiny_llama(sliding_window=95)._document_mask(_packed_ids(), None, None)
    assert pos is None and torch.equal(kr.lo, ops.ranges_sliding_window(2, 96, 95).lo)


def test_llama_pipeline_parallel_window_not_implemented(monkeypatch):
    from neuronx_distributed_llama3_2_amd.models.llama import modeling_llama

    model = _tiny_llama(sliding_window=12)
    wide = _tiny_llama(sliding_window=96)
    monkeypatch.setattr(modeling_llama, "get_pipeline_model_parallel_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="pipeline"):
        model(_packed_ids())
    assert wide._document_mask(_packed_ids(), None, None) == (None, None)   # not binding: nothing to carry


def test_mistral_preset():
    from neuronx_distributed_llama3_2_amd.models.llama.modeling_llama import llama_config

    cfg = llama_config("mistral-7b")
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers) == (4096, 14336, 32)
    assert (cfg.num_attention_heads, cfg.num_key_value_heads, cfg.vocab_size) == (32, 8, 32000)
    assert (cfg.max_position_embeddings, cfg.sliding_window, cfg.rms_norm_eps) == (32768, 4096, 1e-5)
    inv_freq = ops.inv_freq_from_config(cfg, 128)                 # rope_theta 10000, no scaling
    torch.testing.assert_close(inv_freq.float(), 10000.0 ** (-torch.arange(0, 128, 2).float() / 128))
    assert llama_config("tiny", sliding_window=7).sliding_window == 7
    assert getattr(llama_config("tiny"), "sliding_window", None) is None
