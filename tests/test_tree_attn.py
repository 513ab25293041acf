"""ops.tree_attention off the GPU: the arithmetic forward_tree ran before the op existed, bit for bit."""

import math

import pytest
import torch

import neuronx_distributed_llama3_2_amd.ops as ops


def _case(N, seed, Hq=4, Hkv=2, D=16, L=12):
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(1, N, Hq + 2 * Hkv, D, generator=gen)
    cache = torch.randn(2, 3, Hkv, L, D, generator=gen)   # [k | v, cache row, ...]
    mask = torch.eye(N, dtype=torch.bool)
    for j in range(1, N):   # a random tree: self + ancestors
        mask[j] |= mask[int(torch.randint(0, j, (1,), generator=gen))]
    return qkv[:, :, :Hq], qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:], mask, cache[0], cache[1]


def _forward_tree_arithmetic(q, k, v, tree_mask, kcache, vcache, prefix_len, seq_id):
    """The attention lines of forward_tree as they stood (q / k / v [N, heads, D] of one sequence)."""
    (N, nq, D), nkv = q.shape, k.shape[1]
    g, scale = nq // nkv, 1.0 / math.sqrt(D)
    tree_bias = torch.zeros((N, N), dtype=torch.float32).masked_fill(~tree_mask, float("-inf"))
    kc = kcache[seq_id, :, :prefix_len].float()
    vc = vcache[seq_id, :, :prefix_len].float()
    qf = q.float().permute(1, 0, 2).reshape(nkv, g * N, D)
    s_c = torch.matmul(qf, kc.transpose(1, 2)) * scale
    s_t = torch.matmul(qf, k.float().permute(1, 2, 0)) * scale
    s_t = s_t.view(nkv, g, N, N) + tree_bias
    s = torch.cat([s_c.view(nkv, g, N, prefix_len), s_t], -1)
    p_ = torch.softmax(s, -1)
    o = torch.matmul(p_[..., :prefix_len].reshape(nkv, g * N, prefix_len), vc) + \
        torch.matmul(p_[..., prefix_len:].reshape(nkv, g * N, N), v.float().permute(1, 0, 2))
    return o.view(nq, N, D).permute(1, 0, 2).reshape(1, N, nq * D).to(q.dtype)


@pytest.mark.parametrize("P", [0, 7])
@pytest.mark.parametrize("packed", [False, True])
def test_tree_attention_cpu_is_forward_tree_arithmetic(P, packed):
    N = 9
    q, k, v, mask, kc, vc = _case(N, seed=P)
    want = _forward_tree_arithmetic(q[0], k[0], v[0], mask, kc, vc, P, seq_id=2)
    got = ops.tree_attention(q, k, v, ops.pack_tree_mask(mask) if packed else mask, kc, vc,
                             torch.tensor([P], dtype=torch.int32), cache_idx=torch.tensor([2]))
    assert got.shape == q.shape and torch.equal(got.reshape(1, N, -1), want)
    assert torch.equal(ops.tree_attention(q, k, v, mask, kc[2:], vc[2:], P), got)   # int prefix_len, identity rows


def test_tree_attention_refuses_mxfp8_caches():
    q, k, v, mask, kc, vc = _case(4, seed=1, D=32)
    with pytest.raises(TypeError):
        ops.tree_attention(q, k, v, mask, kc.to(torch.uint8), vc.to(torch.uint8), 3)
