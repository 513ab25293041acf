"""csrc/tree_attn.hip on MI355X: per element against fp64, graph replay, fallback, refusals, forward_tree of a tiny Llama."""

import functools
import math

import pytest
import torch

import neuronx_distributed_llama3_2_amd.ops as ops
from neuronx_distributed_llama3_2_amd.ops import _ext

pytestmark = pytest.mark.gpu

DEV, SENTINEL = "cuda", 777.0
LMAX = 2368          # 37 chunks of 64 keys, 10 splits of 256 at the test shapes
PREFIXES = [0, 1, 63, 64, 65, 1100, 2304]   # 256-key splits: 1,100 ends inside split 4, 2,304 is a split boundary


def _tree_mask(N, gen, arbitrary=False):
    if arbitrary:   # only the diagonal guaranteed
        return (torch.rand(N, N, generator=gen) < 0.5) | torch.eye(N, dtype=torch.bool)
    mask = torch.eye(N, dtype=torch.bool)
    for j in range(1, N):
        mask[j] |= mask[int(torch.randint(0, j, (1,), generator=gen))]
    return mask


@functools.lru_cache(maxsize=None)
def _cache_rows(Hkv, D):   # valid K / V rows of one sequence, bf16 [2, Hkv, LMAX, D] on the CPU: made once, never changed
    return torch.randn(2, Hkv, LMAX, D, generator=torch.Generator().manual_seed(Hkv * 1000 + D)).to(torch.bfloat16)


def _inputs(B, N, Hq, Hkv, D, seed):   # q / k_tree / v_tree as views of a wider QKV-shaped buffer (CPU bf16, N(0, 1))
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, Hq + 2 * Hkv + 1, D, generator=gen).to(torch.bfloat16)
    return qkv[:, :, :Hq], qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:Hq + 2 * Hkv], gen


def _caches(rows, prefix, cidx):   # device caches: sequence b's first prefix[b] rows in cache row cidx[b], bf16 NaN elsewhere
    kv = torch.full((2, max(cidx) + 1) + tuple(rows.shape[1:]), float("nan"), dtype=torch.bfloat16, device=DEV)
    for P, cb in zip(prefix, cidx):
        kv[:, cb, :, :P] = rows[:, :, :P].to(DEV)
    return kv[0], kv[1]


def _ref64(q, k, v, mask, rows, P):
    """fp64 softmax attention of one sequence on the CPU -> (out, sum_j p_j |v_jd|), both [N, Hq, D]."""
    (N, Hq, D), G = q.shape, q.shape[1] // k.shape[1]
    keys = torch.cat([rows[0, :, :P], k.permute(1, 0, 2)], 1).double().repeat_interleave(G, 0)   # [Hq, P + N, D]
    vals = torch.cat([rows[1, :, :P], v.permute(1, 0, 2)], 1).double().repeat_interleave(G, 0)
    s = torch.einsum("nhd,hkd->hnk", q.double(), keys) / math.sqrt(D)
    vis = torch.cat([torch.ones(N, P, dtype=torch.bool), mask], 1)
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
    return torch.einsum("hnk,hkd->nhd", p, vals), torch.einsum("hnk,hkd->nhd", p, vals.abs())


def _run_and_check(q, k, v, mask, rows, prefix, cidx, what):
    """The op on non-contiguous q / k / v views with `out` a view inside a buffer of sentinels that must stay
    untouched; every element within 2^-8 |ref| + 2^-8 sum_j p_j |v_jd| of the fp64 reference."""
    (B, N, Hq, D), Hkv = q.shape, k.shape[2]
    kc, vc = _caches(rows, prefix, cidx)
    buf = torch.full((B, N + 2, Hq + 2, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = buf[:, 1:N + 1, 1:Hq + 1]
    qkv = torch.cat([q, k, v], 2).to(DEV)
    ops.tree_attention(qkv[:, :, :Hq], qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:], mask.to(DEV), kc, vc,
                       torch.tensor(prefix, dtype=torch.int32, device=DEV),
                       torch.tensor(cidx, dtype=torch.int32, device=DEV), out=out)
    got = out.double().cpu()
    out.fill_(SENTINEL)
    assert bool((buf == SENTINEL).all()), "the op wrote outside out"
    for b, P in enumerate(prefix):
        ref, mag = _ref64(q[b], k[b], v[b], mask, rows, P)
        err = (got[b] - ref).abs()
        worst = (err / (2.0 ** -8 * ref.abs() + 2.0 ** -8 * mag).clamp_min(1e-30)).max().item()
        print(f"{what} prefix {P}: max |err| {err.max().item():.3e}, worst err / bound {worst:.3f}")
        assert torch.isfinite(got[b]).all() and worst <= 1.0, (what, P)


@pytest.mark.parametrize("N", [1, 11, 17, 64])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_tree_attention_matches_fp64(D, Hq, Hkv, N):
    q, k, v, gen = _inputs(1, N, Hq, Hkv, D, seed=N)
    for P in PREFIXES:   # the sequence sits in cache row 1 of 2
        _run_and_check(q, k, v, _tree_mask(N, gen), _cache_rows(Hkv, D), [P], [1], f"D {D} {Hq}/{Hkv} N {N} tree")
    _run_and_check(q, k, v, _tree_mask(N, gen, arbitrary=True), _cache_rows(Hkv, D), [65], [1], f"D {D} {Hq}/{Hkv} N {N} arbitrary")


def test_tree_attention_batch_and_cache_rows():
    q, k, v, gen = _inputs(2, 11, 8, 2, 64, seed=5)
    _run_and_check(q, k, v, _tree_mask(11, gen), _cache_rows(2, 64), [65, 1100], [1, 0], "batch 2")


@pytest.mark.parametrize("N,D", [(65, 64), (11, 32)])
def test_tree_attention_falls_back_outside_the_kernel(N, D):
    q, k, v, gen = _inputs(1, N, 8, 2, D, seed=3)
    rows = torch.randn(2, 2, 128, D, generator=gen).to(torch.bfloat16)
    _run_and_check(q, k, v, _tree_mask(N, gen), rows, [65], [0], f"fallback N {N} D {D}")


def test_tree_attention_graph_replay_follows_prefix_len():
    N, Hq, Hkv, D = 17, 8, 2, 128
    q, k, v, gen = _inputs(1, N, Hq, Hkv, D, seed=9)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    words = ops.pack_tree_mask(_tree_mask(N, gen)).to(DEV)
    kc, vc = _caches(_cache_rows(Hkv, D), [1100], [0])
    plen = torch.tensor([65], dtype=torch.int32, device=DEV)
    out = torch.empty(1, N, Hq, D, dtype=torch.bfloat16, device=DEV)
    ops.tree_attention(q, k, v, words, kc, vc, plen, out=out)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.tree_attention(q, k, v, words, kc, vc, plen, out=out)
    for P in (65, 1100, 65, 1100):
        plen.fill_(P)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.tree_attention(q, k, v, words, kc, vc, plen)), P


@pytest.mark.parametrize("bad", ["mask_len", "prefix_dtype", "head_dim", "cache_batch"])
def test_tree_attn_binding_refuses(bad):
    B, N, Hq, Hkv, D = 2, 11, 8, 2, 64
    z = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=DEV)   # noqa: E731
    a = dict(q=z(B, N, Hq, D), k_tree=z(B, N, Hkv, D), v_tree=z(B, N, Hkv, D),
             mask_words=torch.ones(N, dtype=torch.int64, device=DEV), k_cache=z(B, Hkv, 128, D), v_cache=z(B, Hkv, 128, D),
             cache_idx=None, prefix_len=torch.zeros(B, dtype=torch.int32, device=DEV),
             out=torch.full((B, N, Hq, D), SENTINEL, dtype=torch.bfloat16, device=DEV), scale=0.125)
    a.update({"mask_len": dict(mask_words=torch.ones(N + 1, dtype=torch.int64, device=DEV)),
              "prefix_dtype": dict(prefix_len=a["prefix_len"].long()),
              "head_dim": dict(k_cache=z(B, Hkv, 128, 128), v_cache=z(B, Hkv, 128, 128)),
              "cache_batch": dict(k_cache=z(1, Hkv, 128, D), v_cache=z(1, Hkv, 128, D))}[bad])
    with pytest.raises(RuntimeError):
        _ext.ext().tree_attn(**a)
    assert bool((a["out"] == SENTINEL).all())


def _llama(dtype, dev, prefill=0):
    from transformers import LlamaConfig
    from transformers import LlamaForCausalLM as HF

    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, LlamaForCausalLMInference
    from neuronx_distributed_llama3_2_amd.models.llama.convert import hf_to_nxd

    cfg = LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=2, vocab_size=1000, max_position_embeddings=1024, rms_norm_eps=1e-5,
                      rope_theta=500000.0, tie_word_embeddings=True, eos_token_id=2)
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in HF(cfg).state_dict().items()}
    icfg = InferenceConfig(batch_size=2, seq_len=256, max_context_length=128, use_hip_graphs=False, decode_graph_steps=1)
    m = LlamaForCausalLMInference(cfg, icfg, dtype=dtype, device=torch.device(dev), init_weights=False)
    m._load_full(hf_to_nxd(sd, cfg))
    if prefill:
        ids = torch.randint(3, 1000, (1, prefill), generator=torch.Generator().manual_seed(2)).to(dev)
        m.model.forward_tokens(ids, torch.arange(prefill, device=dev).view(1, -1), torch.zeros(1, dtype=torch.long, device=dev),
                               last_index=torch.tensor([prefill - 1], device=dev), prefill=True)
    return m.model


def test_forward_tree_kernel_route_against_fp32_cpu(monkeypatch):
    """Kernel route and NXD_TREE_ATTN=0 route against the fp32 CPU model on the same weights and cache bytes: the
    kernel's error is at most twice the other's (both share the bf16 projections; P is bf16 in the kernel)."""
    from neuronx_distributed_llama3_2_amd.inference.medusa import DEFAULT_MEDUSA_CHOICES, medusa_tree_buffers

    P = 70
    bufs = medusa_tree_buffers(DEFAULT_MEDUSA_CHOICES)
    mask, depth = bufs["attn_mask"].bool(), bufs["position_ids"]
    toks = torch.randint(3, 1000, (mask.shape[0],), generator=torch.Generator().manual_seed(4))
    g = _llama(torch.bfloat16, DEV, prefill=P)
    c = _llama(torch.float32, "cpu")
    c.kv_cache.copy_(g.kv_cache.float().cpu())
    ref = c.forward_tree(toks, P + depth, mask, P)[0].float()
    errs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("NXD_TREE_ATTN", knob)
        lg = g.forward_tree(toks.to(DEV), (P + depth).to(DEV), mask.to(DEV), P)[0].float().cpu()
        errs[knob] = ((lg - ref).abs().max() / ref.abs().max()).item()
    print(f"forward_tree vs fp32 cpu: kernel {errs['1']:.3e}, NXD_TREE_ATTN=0 {errs['0']:.3e}")
    assert errs["1"] <= 2 * errs["0"], errs


def test_forward_tree_chain_kv_equals_forward_tokens(monkeypatch):
    """A chain-shaped tree against a 4-token decode of the same tokens.  Layer 0's K / V rows depend on no attention: equal
    bit for bit.  Later layers follow attention from two different kernels and are not (nor are the NXD_TREE_ATTN=0 route's:
    printed); there the kernel route's error against the fp32 CPU model on the same cache bytes is at most twice the decode's.
    Every causal bit exactly: with token j changed, rows before j keep their bits in every layer and, past layer 0, rows from
    j on change (row r's layer-1 K / V depend on token j < r only through bit (r, j) of layer 0's attention)."""
    P, T = 70, 4
    g, c = _llama(torch.bfloat16, DEV, prefill=P), _llama(torch.float32, "cpu")
    c.kv_cache.copy_(g.kv_cache.float().cpu())
    toks = torch.randint(3, 1000, (T,), generator=torch.Generator().manual_seed(6))
    pos, chain = P + torch.arange(T), torch.tril(torch.ones(T, T)).bool()

    def rows(m, t, dev):   # per layer (K, V) [T, Hkv, D] as fp32 on the CPU
        return [[x.float().cpu() for x in kv] for kv in m.forward_tree(t.to(dev), pos.to(dev), chain.to(dev), P)[2]]
    ref, kvs = rows(c, toks, "cpu"), rows(g, toks, DEV)
    monkeypatch.setenv("NXD_TREE_ATTN", "0")
    kvs0 = rows(g, toks, DEV)
    monkeypatch.setenv("NXD_TREE_ATTN", "1")
    for j in range(T):
        other = toks.clone()
        other[j] = 3 + (toks[j] - 2) % 997
        for i, (a, b) in enumerate(zip(rows(g, other, DEV), kvs)):
            for x, y in zip(a, b):
                same = [torch.equal(x[r], y[r]) for r in range(T)]
                assert same == [r < j or (i == 0 and r > j) for r in range(T)], (j, i, same)
    g.forward_tokens(toks.view(1, T).to(DEV), pos.view(1, T).to(DEV), torch.zeros(1, dtype=torch.long, device=DEV),
                     torch.tensor([P + T], dtype=torch.int32, device=DEV))
    for i in range(len(kvs)):
        for j, name in enumerate("KV"):
            want = g.kv_cache[i, j, 0, :, P:P + T].transpose(0, 1).float().cpu()
            err = [(x - ref[i][j]).abs().max().item() for x in (kvs[i][j], kvs0[i][j], want)]
            print(f"layer {i} {name}: equal to decode: kernel {torch.equal(kvs[i][j], want)}, NXD_TREE_ATTN=0 {torch.equal(kvs0[i][j], want)}; "
                  f"max error against fp32: kernel {err[0]:.3e}, NXD_TREE_ATTN=0 {err[1]:.3e}, decode {err[2]:.3e}")
            assert torch.equal(kvs[i][j], want) if i == 0 else err[0] <= 2 * err[2], f"layer {i} {name}"
