"""The fp64 attention references and bounds of attention_refs.py, checked without a GPU:

* the references agree with ops.attention_reference and DropoutAttentionFunc (fp32, CPU) within
  those functions' own fp32 error;
* a plain-torch fp32 emulation of the kernels' arithmetic (64-key tiles, deferred rescale at 8
  log2 units, bf16 P and dS, 256-key backward blocks with chunked item slabs summed in item order,
  bf16 outputs) stays inside every bound on every case -- the bounds are loose enough for a
  correct kernel, established without consulting the kernel;
* the same emulation with one planted bug each fails on the cases named in PLANTED -- the suite
  would notice a subtly wrong kernel;
* the census sensitivity condition: flipping any single boundary pair moves a reference output by
  at least 4 bounds;
* the case tables are valid interval masks within the size cap.
"""

import math

import pytest
import torch

from neuronx_distributed_llama3_2_amd.ops.attention_dropout import DropoutAttentionFunc, dropout_keep_mask
from neuronx_distributed_llama3_2_amd.ops.attention_ranges import validate
from neuronx_distributed_llama3_2_amd.ops.flash_attn import attention_reference

import attention_refs as A
from attention_refs import BF16, F32

LOG2E = torch.tensor(1.4426950408889634, dtype=F32)
LN2 = torch.tensor(0.69314718055994531, dtype=F32)

FWD = A.forward_cases() + A.range_cases() + A.dropout_cases()
BWD = A.backward_cases()
BY_NAME = {c.name: c for c in FWD + BWD}


# ------------------------------------------------------------------------------------------------
# the emulation
# ------------------------------------------------------------------------------------------------

def _rb(x):
    return x.to(BF16).to(F32)


def _heads(t, G=1):
    t = t.to(F32).permute(0, 2, 1, 3)
    return t if G == 1 else t.repeat_interleave(G, dim=1)


def _emu_keep(c, bug):
    if c.drop is None:
        return None, 1.0
    p, seed, ho = c.drop
    keep = dropout_keep_mask(seed, c.B, c.Hq, torch.arange(c.Sq), c.Sk, p, 0 if bug == "keep_local_head" else ho)
    return keep, float(torch.tensor(1.0 / (1.0 - p), dtype=F32))


def emu_fwd(c, t, bug=None):
    """flash_attn_fwd.hip in fp32 torch: one pass over 64-key tiles with a stale running max."""
    vis = A.visibility(c, bug=bug).expand(c.B, c.Hq, c.Sq, c.Sk)
    keep, dscale = _emu_keep(c, bug)
    q, k, v = _heads(t["q"]), _heads(t["k"], c.G), _heads(t["v"], c.G)
    cl2 = torch.tensor(c.softmax_scale, dtype=F32) * LOG2E
    m = torch.full((c.B, c.Hq, c.Sq), -math.inf)
    l = torch.zeros_like(m)
    acc = torch.zeros(c.B, c.Hq, c.Sq, c.D)
    ntiles = (c.Sk + A.TILE_N - 1) // A.TILE_N
    if bug == "tail_tile_dropped" and c.Sk % A.TILE_N:
        ntiles -= 1
    for tix in range(ntiles):
        ksl = slice(tix * A.TILE_N, min(c.Sk, (tix + 1) * A.TILE_N))
        s = q @ k[:, :, ksl].transpose(-1, -2)
        s = torch.where(vis[..., ksl], s, torch.full_like(s, -math.inf))
        tmax = s.max(-1).values * cl2
        first = torch.isinf(m)
        resc = (tmax > m + A.RESCALE_LOG2) | first
        m_new = torch.where(resc, torch.maximum(m, tmax), m)
        alpha = torch.where(first, torch.zeros_like(m), torch.exp2(m - m_new))
        if bug == "rescale_skipped":
            alpha = torch.where(first, alpha, torch.ones_like(alpha))
        l = torch.where(resc, l * alpha, l)
        acc = torch.where(resc[..., None], acc * alpha[..., None], acc)
        m = m_new
        m_use = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        p = torch.exp2(s * cl2 - m_use[..., None])
        l = l + p.sum(-1)
        if keep is not None:
            p = torch.where(keep[..., ksl], p * (1.0 if bug == "drop_scale_missing" else dscale), torch.zeros_like(p))
        acc = acc + _rb(p) @ v[:, :, ksl]
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    lse = torch.where(l > 0, (m + torch.log2(torch.where(l > 0, l, torch.ones_like(l)))) * LN2, torch.full_like(l, -math.inf))
    return dict(o=(acc * inv[..., None]).to(BF16).permute(0, 2, 1, 3), lse=lse)


def kb_iters(kb, Sq, G, causal, off):
    qstart = max(0, kb * A.BLOCK_K - off) if causal else 0
    qstart = qstart // A.BLOCK_Q * A.BLOCK_Q
    return (G * ((Sq - qstart + A.BLOCK_Q - 1) // A.BLOCK_Q) if qstart < Sq else 0), qstart


def emu_bwd(c, t, bug=None):
    """flash_attn_bwd.hip in fp32 torch: 256-key blocks, (q head x 32-row tile) iterations cut into
    items of at most `chunk`, each item's dK / dV in a slab of its own, slabs summed in item order."""
    vis = A.visibility(c, bug=bug).expand(c.B, c.Hq, c.Sq, c.Sk)
    keep, dscale = _emu_keep(c, bug)
    G, D = c.G, c.D
    q, k, v, o, do = _heads(t["q"]), _heads(t["k"]), _heads(t["v"]), _heads(t["o"]), _heads(t["do"])
    scale = torch.tensor(c.softmax_scale, dtype=F32)
    cl2 = scale * LOG2E
    lse = t["lse"]
    nlse = torch.where(torch.isinf(lse), torch.full_like(lse, -math.inf), -lse * (1.0 / scale))
    ndelta = torch.zeros_like(lse) if bug == "delta_omitted" else -(o * do).sum(-1)
    dq_acc = torch.zeros(c.B, c.Hq, c.Sq, D)
    dk = torch.zeros(c.B, c.Hkv, c.Sk, D)
    dv = torch.zeros_like(dk)
    chunk = c.chunk if c.chunk else 24
    heads = torch.arange(c.Hkv) * G
    for kb in range((c.Sk + A.BLOCK_K - 1) // A.BLOCK_K):
        ksl = slice(kb * A.BLOCK_K, min(c.Sk, (kb + 1) * A.BLOCK_K))
        n_it, qstart = kb_iters(kb, c.Sq, G, c.causal, c.offset)
        if n_it == 0:
            continue
        n_qt = n_it // G
        nc = (n_it + chunk - 1) // chunk
        per = (n_it + nc - 1) // nc
        kb_k, kb_v = k[:, :, ksl], v[:, :, ksl]
        sum_dk = torch.zeros(c.B, c.Hkv, ksl.stop - ksl.start, D)
        sum_dv = torch.zeros_like(sum_dk)
        for item in range(nc):
            acc_dk, acc_dv = torch.zeros_like(sum_dk), torch.zeros_like(sum_dk)
            for it in range(item * per, min(n_it, (item + 1) * per)):
                g, qt0 = it // n_qt, qstart + (it % n_qt) * A.BLOCK_Q
                if bug == "group_head_dropped" and G > 1 and g == G - 1:
                    continue
                hq = heads + g
                qsl = slice(qt0, min(c.Sq, qt0 + A.BLOCK_Q))
                qt, dot = q[:, hq, qsl], do[:, hq, qsl]
                s = nlse[:, hq, qsl, None] + qt @ kb_k.transpose(-1, -2)
                p = torch.where(vis[:, hq, qsl, ksl], torch.exp2(s * cl2), torch.zeros_like(s))
                dp = dot @ kb_v.transpose(-1, -2)
                if keep is None:
                    pd, ds = p, p * (dp + ndelta[:, hq, qsl, None])
                else:
                    mk = keep[:, hq, qsl, ksl].to(F32) * dscale
                    pd, ds = p * (keep[:, hq, qsl, ksl].to(F32) if bug == "drop_scale_missing" else mk), \
                        p * (mk * dp + ndelta[:, hq, qsl, None])
                pd, ds = _rb(pd), _rb(ds)
                acc_dv += pd.transpose(-1, -2) @ dot
                acc_dk += ds.transpose(-1, -2) @ qt
                dq_acc[:, hq, qsl] += ds @ kb_k
            if not (bug == "item_slab_dropped" and nc > 1 and item == nc - 1):
                sum_dk, sum_dv = sum_dk + acc_dk, sum_dv + acc_dv
        dk[:, :, ksl], dv[:, :, ksl] = sum_dk * scale, sum_dv
    dq = dq_acc if bug == "dq_scale_missing" else dq_acc * scale
    pm = lambda x: x.to(BF16).permute(0, 2, 1, 3)
    return dict(dq=pm(dq), dk=pm(dk), dv=pm(dv))


def emulate(c, t, bug=None):
    return emu_fwd(c, t, bug) if c.kind == "fwd" else emu_bwd(c, t, bug)


_CACHE = {}


def prepared(c):
    """Inputs and reference of a case, computed once and shared (never modified)."""
    if c.name not in _CACHE:
        t = A.make_inputs(c)
        ref = A.reference(c, t)
        _CACHE[c.name] = (t, {k: v for k, v in ref.items() if k not in ("P", "PD", "dS", "dpraw")})   # [B,Hq,Sq,Sk] tensors
    return _CACHE[c.name]


def test_bf16_unit_roundoff():
    """Round-to-nearest to bf16 costs up to 2^-8 relative (8 significant bits), not 2^-9: the
    witness quoted in attention_refs.py, and the bound itself over a dense sample."""
    x = torch.tensor(0.3310, dtype=torch.float64)
    assert float((x.to(BF16).double() - x).abs() / x) > 1.4 * 2.0 ** -9
    xs = torch.logspace(-3, 3, 200001, dtype=torch.float64)
    assert float(((xs.to(BF16).double() - xs).abs() / xs).max()) <= A.P_RND


# ------------------------------------------------------------------------------------------------
# case-table sanity
# ------------------------------------------------------------------------------------------------

def test_case_tables_are_valid_and_small():
    cases = A.all_cases()
    assert len({c.name for c in cases}) == len(cases), "case names must be unique"
    for c in cases:
        assert c.D in (64, 128) and c.Hq % c.Hkv == 0 and 1 <= c.Sk <= A.MAX_KEYS and 1 <= c.Sq <= A.MAX_KEYS, str(c)
        assert c.layout == "pad" or c.Sq == c.Sk, f"{c}: the fused layout needs Sq == Sk"
        assert not (c.ranges is not None and c.drop is not None), f"{c}: no RANGE + DROP kernel"
        kr = A.key_ranges(c)
        if kr is not None:
            validate(kr)
            assert kr._checked


def test_case_tables_reach_the_guards():
    fwd = A.forward_cases()
    assert {c.Sq for c in fwd} >= set(A.FWD_SQ) and {c.Sk for c in fwd} >= set(A.FWD_SK)
    assert {c.G for c in fwd} >= {1, 4, 8}
    w8 = lambda c: ((c.Sq + 255) // 256) * c.B * c.Hq >= 512
    for tab in (fwd, A.range_cases(), A.dropout_cases()):
        assert any(w8(c) for c in tab) and any(not w8(c) and c.B == 7 for c in tab)
    bwd = A.backward_cases()
    assert {c.Sq for c in bwd} >= set(A.BWD_SQ) and {c.Sk for c in bwd} >= set(A.BWD_SK) and {c.G for c in bwd} >= {1, 4}
    assert {c.chunk for c in bwd} >= {0, 8, A.ONE_ITEM}
    for c in bwd:
        if c.chunk == A.ONE_ITEM:
            assert all(kb_iters(kb, c.Sq, c.G, c.causal, c.offset)[0] <= c.chunk for kb in range(4))
    # rows without keys and keys without rows exist where the tables say so
    c = next(c for c in bwd if c.Sq == 100 and c.Sk == 600 and c.inputs == "rand")
    assert bool(prepared(c)[1]["k_dead"][:, :, 256:].all()) and not bool(prepared(c)[1]["k_dead"][:, :, :100].any())
    c = next(c for c in fwd if c.Sq > c.Sk and c.causal and c.inputs == "rand")
    assert bool((~prepared(c)[1]["live"]).any())


# ------------------------------------------------------------------------------------------------
# agreement with the project's fp32 references
# ------------------------------------------------------------------------------------------------

def _fp32_tol(ref):
    """A few hundred fp32 roundings of O(max|ref|) quantities."""
    return 1e-4 * (1.0 + float(ref.abs().max()))


@pytest.mark.parametrize("c", [c for c in FWD if c.variant != "drop" and not c.census], ids=str)
def test_forward_reference_agrees_with_attention_reference(c):
    t, ref = prepared(c)
    o, lse = attention_reference(t["q"], t["k"], t["v"], c.causal, c.softmax_scale, c.offset, key_ranges=A.key_ranges(c))
    assert float((o.double() - ref["o"]).abs().max()) <= _fp32_tol(ref["o"])
    live = ref["live"]
    assert bool(torch.isneginf(lse[~live]).all())
    assert float((lse[live].double() - ref["lse"][live]).abs().max()) <= _fp32_tol(ref["lse"][live])


@pytest.mark.parametrize("c", [c for c in A.dropout_cases() + BWD if c.drop is not None and c.inputs == "rand"
                               and c.off is None and ((c.Sq + 255) // 256) * c.B * c.Hq < 512], ids=str)
def test_dropout_reference_agrees_with_dropout_attention_func(c):
    t, ref = prepared(c)
    bhsd = lambda x: x.float().permute(0, 2, 1, 3).contiguous()
    q, k, v = (bhsd(t[n]).requires_grad_(True) for n in ("q", "k", "v"))
    p, seed, ho = c.drop
    o = DropoutAttentionFunc.apply(q, k, v, c.causal, c.softmax_scale, p, seed, ho)
    if c.kind == "fwd":
        assert float((o.detach().permute(0, 2, 1, 3).double() - ref["o"]).abs().max()) <= _fp32_tol(ref["o"])
        return
    # backward: DropoutAttentionFunc differentiates at its own fp32 o (and lse), so the fp64 backward
    # is taken at that o, not at the case's bf16-rounded one
    o.backward(bhsd(t["do"]))
    fwd = A.fwd_ref(t["q"], t["k"], t["v"], c.softmax_scale, A.visibility(c), A.keep_scale(c))
    ref = A.bwd_ref(t["q"], t["k"], t["v"], o.detach().permute(0, 2, 1, 3), fwd["lse"], t["do"], c.softmax_scale,
                    A.visibility(c), A.keep_scale(c))
    for n, g in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        r = ref[n].permute(0, 2, 1, 3)
        assert float((g.double() - r).abs().max()) <= _fp32_tol(r), n


# ------------------------------------------------------------------------------------------------
# the emulation stays inside every bound
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cases", A.group(FWD + BWD, 12), ids=lambda cs: cs[0].name)
def test_emulation_within_bounds(cases):
    for c in cases:
        t, ref = prepared(c)
        ratios = A.check_outputs(c, emulate(c, t), ref, " (emulation)")
        assert all(r <= 1.0 for r in ratios.values())


def test_spike_cases_take_the_paths_they_are_named_for():
    for name, lo, hi in (("spike_over", A.RESCALE_LOG2, 64.0), ("spike_under", 4.0, A.RESCALE_LOG2)):
        c = next(c for c in FWD if c.inputs == name and not c.causal and c.D == 128)
        t, _ = prepared(c)
        x = (t["q"].double().permute(0, 2, 1, 3) @ t["k"].double().permute(0, 2, 3, 1).repeat_interleave(c.G, 1))
        x = x * c.softmax_scale * 1.4426950408889634
        jump = x[..., c.Sk - 2] - x[..., :64].max(-1).values      # spike over the first tile's max, log2 units
        assert lo < float(jump.min()) and float(jump.max()) < hi, (name, float(jump.min()), float(jump.max()))
    c = next(c for c in FWD if c.inputs == "big")
    t, ref = prepared(c)
    assert float(ref["lse"][ref["live"]].abs().max()) > 50.0


# ------------------------------------------------------------------------------------------------
# planted bugs: each must be caught by the named cases
# ------------------------------------------------------------------------------------------------

def _pick(kind, **kw):
    tabs = FWD if kind == "fwd" else BWD
    hit = [c for c in tabs if all((v(c) if callable(v) else getattr(c, k) == v) for k, v in kw.items())]
    assert hit, (kind, kw)
    return hit[0].name


# bug -> the cases that must catch it.  In the order of the list this file was written against:
# causal >= instead of > (one key too few at the diagonal); hi inclusive; lo off by one; last
# partial key tile dropped; rescale skipped when the max jumps (m moves, l and the accumulators
# keep their old scale); the dropout scale 1 / (1 - p) left off the bf16 P operand of P.V and
# P^T dO; one query head left out of the dK / dV group sum; one item slab left out of the slab sum;
# keep mask hashed with the local head instead of head_offset + head; delta omitted; dQ missing scale.
PLANTED = {
    "causal_ge": [_pick("fwd", inputs="census", variant="plain", Sq=129, Sk=65),
                  _pick("fwd", inputs="rand", variant="plain", causal=True, Sq=193),
                  _pick("bwd", inputs="census_q", variant="plain", Sk=513, chunk=0)],
    "hi_inclusive": [_pick("fwd", inputs="census", variant="range", Sk=193), _pick("fwd", inputs="rand", variant="range", Sk=321),
                     _pick("bwd", inputs="census_k", variant="range", Sq=33)],
    "lo_off_by_one": [_pick("fwd", inputs="census", variant="range", Sk=321), _pick("fwd", inputs="rand", variant="range", Sk=193),
                      _pick("bwd", inputs="census_q", variant="range", chunk=8)],
    "tail_tile_dropped": [_pick("fwd", inputs="census", variant="plain", Sk=65), _pick("fwd", inputs="rand", variant="plain", Sk=129),
                          _pick("fwd", inputs="census", variant="drop", Sk=193)],
    "rescale_skipped": [_pick("fwd", inputs="spike_over", causal=False, D=64), _pick("fwd", inputs="spike_over", causal=True, D=128)],
    "drop_scale_missing": [_pick("fwd", inputs="census", variant="drop", Sk=193), _pick("fwd", inputs="rand", variant="drop", Sk=129),
                           _pick("bwd", inputs="rand", variant="drop", Sk=257)],
    "group_head_dropped": [_pick("bwd", inputs="census_k", variant="plain", Sk=513, chunk=8, G=4),
                           _pick("bwd", inputs="rand", variant="plain", Sk=513, chunk=0, G=4)],
    "item_slab_dropped": [_pick("bwd", inputs="census_q", variant="plain", Sk=513, chunk=8),
                          _pick("bwd", inputs="rand", variant="plain", Sk=513, chunk=8)],
    "keep_local_head": [_pick("fwd", inputs="census", variant="drop", drop=lambda c: c.drop[2] == 4),
                        _pick("bwd", inputs="census_q", variant="drop", drop=lambda c: c.drop[2] == 4)],
    "delta_omitted": [_pick("bwd", inputs="census_q", variant="plain", Sk=257), _pick("bwd", inputs="rand", variant="plain", Sk=257)],
    "dq_scale_missing": [_pick("bwd", inputs="census_q", variant="plain", Sk=255), _pick("bwd", inputs="rand", variant="plain", Sk=255)],
}


@pytest.mark.parametrize("bug,name", [(b, n) for b, names in PLANTED.items() for n in names])
def test_planted_bug_is_caught(bug, name):
    c = BY_NAME[name]
    t, ref = prepared(c)
    A.check_outputs(c, emulate(c, t), ref, " (emulation)")            # the unplanted emulation passes this case
    with pytest.raises(AssertionError):
        A.check_outputs(c, emulate(c, t, bug), ref, f" (emulation, {bug})")


# ------------------------------------------------------------------------------------------------
# census sensitivity
# ------------------------------------------------------------------------------------------------

CENSUS = [c for c in FWD + BWD if c.census]


@pytest.mark.parametrize("cases", A.group(CENSUS, 12), ids=lambda cs: cs[0].name)
def test_census_sensitivity(cases):
    for c in cases:
        res = A.census_sensitivity(c, prepared(c)[0])
        assert res, f"{c}: no boundary pair at all"
        for boundary, (worst, rows) in res.items():
            assert worst >= A.SENS, f"{c}: flipping a {boundary} pair moves the outputs by only {worst:.3g} bounds ({rows} rows)"


def test_census_boundaries_are_all_exercised():
    seen = {}
    for c in CENSUS:
        for name, m in A.boundary_pairs(c).items():
            seen[(c.kind, name)] = seen.get((c.kind, name), 0) + int(m.any(-1).sum())
    for kind in ("fwd", "bwd"):
        for name in ("causal-in", "causal-out", "lo-in", "lo-out", "hi-in", "hi-out", "Sk-in"):
            assert seen.get((kind, name), 0) > 0, (kind, name)
        assert seen.get((kind, "keep"), 0) > 0
