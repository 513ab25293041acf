"""Interval-masked attention on the CPU reference path: the range constructors against a dense
brute-force mask, the fp32 reference with `key_ranges`, and the Llama model with document masking
(ops/attention_ranges.py, ops/flash_attn.py, models/llama/modeling_llama.py)."""

import os
import tempfile

import pytest
import torch
import torch.distributed as dist

import neuronx_distributed_llama3_2_amd.ops as ops
from neuronx_distributed_llama3_2_amd.ops import attention_ranges as ar

from dist_utils import _free_port, run_distributed

S = 640
BOUNDS = [0, 1, 2, 65, 256, 300, 513, 640]   # document boundaries of row 0


def _starts(bounds, S):
    m = torch.zeros(S, dtype=torch.bool)
    m[torch.tensor([b for b in bounds if b < S])] = True
    return m


def _doc_id(bounds, S):
    d = torch.zeros(S, dtype=torch.long)
    for i, b in enumerate(bounds[:-1]):
        d[b:bounds[i + 1]] = i
    return d


def _doc_mask(bounds, S):
    """Brute force: q sees k iff they are in the same document (the causal part is applied apart)."""
    d = _doc_id(bounds, S)
    return d[:, None] == d[None, :]


def _transposed_mask(r):
    q_lo, q_hi = r.transposed()
    qi = torch.arange(r.num_queries)[None, :, None]
    return (qi >= q_lo[:, None, :]) & (qi < q_hi[:, None, :])


def _causal(Sq, Sk, off=None):
    off = Sk - Sq if off is None else off
    return torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None] + off


def _two_rows():
    return torch.stack([_starts(BOUNDS, S), _starts([0], S)])


def test_document_starts_match_dense_mask():
    r = ar.ranges_from_document_starts(_two_rows())
    ar.validate(r)
    assert r.lo.dtype == torch.int32 and r.hi.dtype == torch.int32
    want = torch.stack([_doc_mask(BOUNDS, S), _doc_mask([0, S], S)]) & _causal(S, S)
    assert torch.equal(r.dense_mask(causal=True), want)
    # the transposed pair describes the same interval mask (before the causal cut)
    assert torch.equal(_transposed_mask(r), r.dense_mask())
    assert torch.equal(ar.positions_from_ranges(r)[0, 63:67].long(), torch.tensor([61, 62, 0, 1]))


def test_eos_and_cu_seqlens_match_document_starts():
    want = ar.ranges_from_document_starts(_two_rows())
    ids = torch.randint(1, 100, (2, S))
    for b in BOUNDS[1:-1]:
        ids[0, b - 1] = 0          # a document ends with EOS, the next token starts a new one
    ids[1, S - 1] = 0              # EOS in the last position starts nothing
    r = ar.ranges_from_eos(ids, 0)
    assert torch.equal(r.lo, want.lo) and torch.equal(r.hi, want.hi)
    cu = torch.tensor(BOUNDS + [2 * S])
    r = ar.ranges_from_cu_seqlens(cu, 2, S)
    assert torch.equal(r.lo, want.lo) and torch.equal(r.hi, want.hi)
    # a document crossing the row boundary is cut by it
    r = ar.ranges_from_cu_seqlens(torch.tensor([0, 600, 700, 2 * S]), 2, S)
    assert r.lo[0, 599] == 0 and r.lo[0, 600] == 600 and r.lo[1, 0] == 0 and r.lo[1, 59] == 0 and r.lo[1, 60] == 60


@pytest.mark.parametrize("empty", [False, True])
def test_lengths_match_dense_mask(empty):
    lens = torch.tensor([S, 1, 129, 0])
    r = ar.ranges_from_lengths(lens, S, S, empty_padded_queries=empty)
    ar.validate(r)
    k = torch.arange(S)[None, None, :]
    q = torch.arange(S)[None, :, None]
    want = (k < lens[:, None, None]).expand(4, S, S)
    if empty:
        want = want & (q < lens[:, None, None])
    assert torch.equal(r.dense_mask(), want)
    assert torch.equal(_transposed_mask(r), want)
    # cross lengths: 100 queries over 300 keys
    r = ar.ranges_from_lengths(torch.tensor([300, 7]), 100, 300)
    assert r.lo.shape == (2, 100) and r.num_keys == 300
    assert torch.equal(_transposed_mask(r), r.dense_mask())


def test_sliding_window_matches_dense_mask():
    r = ar.ranges_sliding_window(2, S, 100)
    ar.validate(r)
    q = torch.arange(S)[:, None]
    k = torch.arange(S)[None, :]
    want = ((k <= q) & (k > q - 100)).expand(2, S, S)
    assert torch.equal(r.dense_mask(), want)
    assert torch.equal(r.dense_mask(causal=True), want)
    assert torch.equal(_transposed_mask(r), want)


def test_random_ranges_transpose_exactly():
    g = torch.Generator().manual_seed(3)
    for _ in range(20):
        cuts = sorted(set([0, S] + torch.randint(1, S, (7,), generator=g).tolist()))
        docs = ar.ranges_from_document_starts(_starts(cuts, S)[None])
        win = int(torch.randint(1, 200, (1,), generator=g))
        ln = int(torch.randint(0, S + 1, (1,), generator=g))
        q = torch.arange(S, dtype=torch.int32)[None]
        lo = torch.maximum(docs.lo, (q - win + 1).clamp(min=0))   # documents and a window
        hi = torch.minimum(q + 1, torch.full_like(q, ln))          # causal and right padding: empty rows past ln
        r = ar.KeyRanges(lo, hi, S)
        ar.validate(r)
        assert torch.equal(_transposed_mask(r), r.dense_mask())


def test_validate_raises():
    lo = torch.zeros(1, 8, dtype=torch.int32)
    hi = torch.full((1, 8), 8, dtype=torch.int32)
    bad = lo.clone()
    bad[0, 3] = 2                  # lo goes 0 0 0 2 0 ...: not monotone
    with pytest.raises(ValueError, match="non-decreasing"):
        ar.validate(ar.KeyRanges(bad, hi, 8))
    with pytest.raises(ValueError, match="hi <= 7"):
        ar.validate(ar.KeyRanges(lo, hi, 7))
    ar.validate(ar.KeyRanges(lo, hi, 8))
    q = torch.randn(1, 8, 2, 16)
    with pytest.raises(ValueError, match="non-decreasing"):
        ops.flash_attn_func(q, q, q, key_ranges=ar.KeyRanges(bad, hi, 8))
    with pytest.raises(ValueError, match="attention is"):
        ops.flash_attn_func(q, q, q, key_ranges=ar.KeyRanges(lo[:, :4], hi[:, :4], 8))


def _dense_attention(q, k, v, mask, scale):
    """fp32 softmax over a dense bool mask [B, Sq, Sk] (True = visible); empty rows give 0 / -inf."""
    g = q.shape[2] // k.shape[2]
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(~mask[:, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return (p @ vf).permute(0, 2, 1, 3), torch.logsumexp(s, dim=-1)


def test_reference_with_ranges_equals_dense_masked_softmax():
    torch.manual_seed(0)
    B, Sq, Hq, Hkv, D = 2, 96, 4, 2, 32
    q, k, v = torch.randn(B, Sq, Hq, D), torch.randn(B, Sq, Hkv, D), torch.randn(B, Sq, Hkv, D)
    r = ar.ranges_from_document_starts(torch.stack([_starts([0, 1, 2, 65], Sq), _starts([0], Sq)]))
    want_mask = torch.stack([_doc_mask([0, 1, 2, 65, Sq], Sq), _doc_mask([0, Sq], Sq)]) & _causal(Sq, Sq)
    assert torch.equal(r.dense_mask(causal=True), want_mask)
    o, lse = ops.attention_reference(q, k, v, causal=True, key_ranges=r)
    ro, rlse = _dense_attention(q, k, v, want_mask, 1.0 / D ** 0.5)
    torch.testing.assert_close(o, ro)
    torch.testing.assert_close(lse, rlse)
    # forward-only entry point on CPU tensors takes the same path
    o2, lse2 = ops.flash_attn_fwd_lse(q, k, v, causal=True, key_ranges=r)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)


def test_empty_rows_and_gradients_on_cpu():
    torch.manual_seed(1)
    B, Sq, H, D = 3, 40, 2, 16
    q, k, v = (torch.randn(B, Sq, H, D, requires_grad=True) for _ in range(3))
    lens = torch.tensor([40, 1, 17])
    r = ar.ranges_from_lengths(lens, Sq, Sq, empty_padded_queries=True)
    o, lse = ops.attention_reference(q, k, v, causal=False, key_ranges=r)
    pad = torch.arange(Sq)[None, :] >= lens[:, None]                   # [B, Sq]
    assert torch.equal(o[pad], torch.zeros_like(o[pad]))
    assert torch.isneginf(lse.transpose(1, 2)[pad]).all() and torch.isfinite(lse.transpose(1, 2)[~pad]).all()
    # flash_attn_func on CPU tensors differentiates through the reference
    out = ops.flash_attn_func(q, k, v, causal=False, key_ranges=r)
    assert torch.equal(out, o)
    out.backward(torch.randn_like(out))
    for t in (q, k, v):
        assert torch.isfinite(t.grad).all()
    assert torch.equal(q.grad[pad], torch.zeros_like(q.grad[pad]))
    kpad = pad   # keys past the length are seen by nobody
    assert torch.equal(k.grad[kpad], torch.zeros_like(k.grad[kpad]))
    assert torch.equal(v.grad[kpad], torch.zeros_like(v.grad[kpad]))
    assert q.grad[~pad].abs().max() > 0


def test_dropout_with_ranges_raises_on_cpu():
    q = torch.randn(1, 8, 2, 16)
    with pytest.raises(ValueError, match="dropout"):
        ops.flash_attn_func(q, q, q, dropout_p=0.1, seed=1, key_ranges=ar.ranges_sliding_window(1, 8, 3))


# ---------------------------------------------------------------------------------------------
# Llama model
# ---------------------------------------------------------------------------------------------

EOS = 255


def _tiny_llama(**over):
    from neuronx_distributed_llama3_2_amd.models.llama.modeling_llama import LlamaForCausalLM, llama_config
    from neuronx_distributed_llama3_2_amd.parallel_layers import parallel_state as ps

    if not dist.is_initialized():
        # an explicit address on a free port: nothing is left in os.environ for later tests
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    if not ps.model_parallel_is_initialized():
        ps.initialize_model_parallel(1)
    cfg = llama_config("tiny", num_hidden_layers=2, hidden_size=128, intermediate_size=256, num_attention_heads=4,
                       num_key_value_heads=2, vocab_size=256, max_position_embeddings=128, **over)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg, dtype=torch.float32, device=torch.device("cpu")).eval()


def _packed_ids(seed=0):
    """Two rows of 96 tokens; row 0 holds documents [0, 30), [30, 31), [31, 70), [70, 96), row 1
    documents [0, 50), [50, 96).  No EOS inside a document."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, EOS, (2, 96), generator=g)
    for row, ends in ((0, (29, 30, 69)), (1, (49,))):
        for e in ends:
            ids[row, e] = EOS
    return ids


def test_llama_documents_are_independent():
    """With document masking and position reset, what stands in an earlier document cannot reach a
    later one: the later logits are bitwise equal.  Without masking they change."""
    model = _tiny_llama(document_masking_eos_token_id=EOS, reset_position_ids=True)
    ids = _packed_ids()
    other = ids.clone()
    g = torch.Generator().manual_seed(9)
    other[0, :29] = torch.randint(0, EOS, (29,), generator=g)   # new first document in row 0,
    other[1, :49] = torch.randint(0, EOS, (49,), generator=g)   # and in row 1 (EOS tokens stay)
    assert not torch.equal(ids, other)
    with torch.no_grad():
        a = model(ids).logits          # [S, B, V]
        b = model(other).logits
    assert a.shape == b.shape == (96, 2, 256)
    assert torch.equal(a[30:, 0], b[30:, 0]) and torch.equal(a[50:, 1], b[50:, 1])
    assert not torch.equal(a[:29, 0], b[:29, 0])
    # masked probabilities are exactly 0: the mask of the derived ranges is the document mask
    r = ops.ranges_from_eos(ids, EOS)
    want = torch.stack([_doc_mask([0, 30, 31, 70, 96], 96), _doc_mask([0, 50, 96], 96)]) & _causal(96, 96)
    assert torch.equal(r.dense_mask(causal=True), want)
    # the same replacement with masking off reaches the later documents
    plain = _tiny_llama()
    plain.load_state_dict(model.state_dict())
    with torch.no_grad():
        a = plain(ids).logits
        b = plain(other).logits
    assert not torch.equal(a[30:, 0], b[30:, 0]) and not torch.equal(a[50:, 1], b[50:, 1])
    # an explicit key_ranges= / position_ids= pair gives what the config switches derive
    with torch.no_grad():
        c = plain(ids, key_ranges=r, position_ids=ops.positions_from_ranges(r)).logits
        d = model(ids).logits
    assert torch.equal(c, d)


def test_llama_document_span_equals_standalone_forward():
    """The logits on a document's span equal a forward of that document alone.

    Gate: torch.testing.assert_close fp32 defaults (rtol 1.3e-6, atol 1e-5).  Measured on this
    model (fp32 CPU reference path): max |packed - standalone| = 0 on all three documents, as is
    the difference between the same standalone document run at batch 1 and at batch 2 (the same
    math with different blocking), so the default gate holds with room and no wider gate derived
    from the blocking noise is needed.  The figures are printed before the assertion."""
    model = _tiny_llama(document_masking_eos_token_id=EOS, reset_position_ids=True)
    ids = _packed_ids()
    with torch.no_grad():
        packed = model(ids).logits
        for row, (a, b) in ((0, (31, 70)), (1, (50, 96)), (0, (0, 30))):
            doc = ids[row:row + 1, a:b]
            alone = model(doc).logits[:, 0]
            twice = model(doc.repeat(2, 1)).logits[:, 1]
            print(f"row {row} [{a}, {b}): packed vs standalone {(packed[a:b, row] - alone).abs().max().item():.3e}, "
                  f"batch 1 vs batch 2 {(alone - twice).abs().max().item():.3e}")
            torch.testing.assert_close(packed[a:b, row], alone)


def test_llama_pipeline_parallel_masking_not_implemented(monkeypatch):
    from neuronx_distributed_llama3_2_amd.models.llama import modeling_llama

    model = _tiny_llama(document_masking_eos_token_id=EOS)
    monkeypatch.setattr(modeling_llama, "get_pipeline_model_parallel_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="pipeline"):
        model(_packed_ids())


def _interleave_worker(rank, world, streams, out):
    from neuronx_distributed_llama3_2_amd.models.llama.modeling_llama import LlamaForCausalLM, llama_config
    from neuronx_distributed_llama3_2_amd.optimizer.flat_optimizer import FlatMixedPrecisionAdamW
    from neuronx_distributed_llama3_2_amd.parallel.grad_buffer import find_shared_params
    from neuronx_distributed_llama3_2_amd.parallel_layers import parallel_state as ps
    from neuronx_distributed_llama3_2_amd.parallel_layers import stream_split

    stream_split.set_enabled(streams >= 2, streams)
    stream_split.set_stagger(0)
    ps.initialize_model_parallel(world)
    eos = 1023
    cfg = llama_config("tiny8", sequence_parallel_enabled=True, max_position_embeddings=128, num_hidden_layers=2,
                       document_masking_eos_token_id=eos, reset_position_ids=True)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg, dtype=torch.float32, device=torch.device("cpu"))
    model.train()
    opt = FlatMixedPrecisionAdamW(model.parameters(), lr=1e-3, grad_clipping=True, max_grad_norm=1.0,
                                  shared_param_ids=find_shared_params(model))
    torch.manual_seed(5)
    ids = torch.randint(0, eos, (4, 128))
    for row, ends in enumerate(((40, 41, 99), (63,), (), (5, 127))):   # different documents per row
        for e in ends:
            ids[row, e] = eos
    calls = []
    orig = LlamaForCausalLM._forward_interleaved

    def spy(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    LlamaForCausalLM._forward_interleaved = spy
    loss = model(ids, labels=ids).loss
    loss.backward()
    cfg.document_masking_eos_token_id = None
    with torch.no_grad():
        unmasked = model(ids, labels=ids).loss    # same weights, masking off (one pass: no grad)
    opt.step()
    gn = opt.grad_norm
    LlamaForCausalLM._forward_interleaved = orig
    if rank == 0:
        torch.save({"loss": float(loss), "gn": float(gn), "unmasked": float(unmasked), "interleaved": len(calls)}, out)


def test_llama_interleaved_parts_match_one_pass_with_masking():
    d = tempfile.mkdtemp()
    res = []
    for streams in (1, 2):
        run_distributed(_interleave_worker, 2, streams, os.path.join(d, f"r{streams}.pt"))
        res.append(torch.load(os.path.join(d, f"r{streams}.pt")))
    a, b = res
    assert a["interleaved"] == 0 and b["interleaved"] == 1
    assert abs(a["loss"] - b["loss"]) < 1e-4 * abs(a["loss"]), (a, b)       # the gates of tests/test_stream_split.py
    assert abs(a["gn"] - b["gn"]) < 1e-3 * a["gn"], (a, b)
    assert abs(a["loss"] - a["unmasked"]) > 1e-4 * abs(a["loss"]), a         # the mask is in effect
