"""Per-element checks of the flash-attention kernels (_C.flash_attn_fwd / _C.flash_attn_bwd: plain,
DROP and RANGE instantiations, 4- and 8-wave forward, every backward item plan) against the fp64
references of attention_refs.py, at the shapes that reach their guards.

The bindings are called directly: every output (o, lse, dq, dk, dv) is a strided view inside a
larger buffer pre-filled with a NaN bit pattern, and the pads of q, k, v, dO hold NaNs too -- an
over-read poisons the result, a stray write shows as a changed bit, an unwritten element as NaN.
Census cases are held to the tight bounds, random cases to the a-priori bounds derived in
attention_refs.py; exact zeros and -inf are asserted bit for bit.  The backward is fed o and lse
rounded from the fp64 forward reference, so it is judged on its own; every backward case is run
twice and must give bit-equal dk / dv (dq goes through atomics and is excluded).

Every test records its worst err / bound ratio per variant and output (record_property
"worst_<variant>_<output>").
"""

from dataclasses import replace

import pytest
import torch

import neuronx_distributed_llama3_2_amd.ops as ops
from neuronx_distributed_llama3_2_amd.ops import _ext
from neuronx_distributed_llama3_2_amd.ops.attention_dropout import attention_with_dropout

import attention_refs as A
from attention_refs import BF16, F32, Case, Slot
from rowwise_refs import assert_bit_equal

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True)
def _native():
    assert _ext.ext_available(), "HIP extension must be built for GPU tests"
    yield


@pytest.fixture
def worst(record_property):
    seen = {}

    def note(c, ratios):
        for k, r in ratios.items():
            name = f"{c.variant}_{'census' if c.census else 'rand'}_{k}"
            seen[name] = max(seen.get(name, 0.0), float(r))

    yield note
    for k, v in seen.items():
        record_property("worst_" + k, round(v, 4))


def _drop_args(c):
    return (0.0, 0, 0) if c.drop is None else (float(c.drop[0]), int(c.drop[1]), int(c.drop[2]))


def _slots(c, names):
    """Sentinel slots for the named tensors in the case's layout."""
    shapes = dict(q=(c.B, c.Sq, c.Hq, c.D), k=(c.B, c.Sk, c.Hkv, c.D), v=(c.B, c.Sk, c.Hkv, c.D))
    shapes.update(o=shapes["q"], do=shapes["q"], dq=shapes["q"], dk=shapes["k"], dv=shapes["k"])
    out = {}
    if c.layout == "fused":
        out.update(zip("qkv", A.fused_slots(c.Sq, c.B, (c.Hq, c.Hkv, c.Hkv), c.D, DEV)))
        out["o"] = A.fused_slots(c.Sq, c.B, (c.Hq,), c.D, DEV)[0]
        out["do"] = A.fused_slots(c.Sq, c.B, (c.Hq,), c.D, DEV)[0]
        out.update(zip(("dq", "dk", "dv"), A.fused_slots(c.Sq, c.B, (c.Hq, c.Hkv, c.Hkv), c.D, DEV)))
    else:
        # dO and dk non-contiguous in their leading dims; o alternates between the two layouts
        kinds = dict(q="pad", k="sbhd", v="pad", o=("sbhd" if c.D == 64 else "pad"), do="sbhd", dq="pad", dk="sbhd", dv="pad")
        for n in shapes:
            out[n] = Slot.make(shapes[n], DEV, kinds[n])
    return {n: out[n] for n in names}


def run_forward(C, c, t):
    s = _slots(c, ("q", "k", "v", "o"))
    for n in "qkv":
        s[n].fill(t[n].to(DEV))
    lse = A.flat_slot((c.B, c.Hq, c.Sq), DEV)
    s["o"].snapshot()
    lse.snapshot()
    kr = A.key_ranges(c, DEV)
    extra = () if kr is None else (kr.lo, kr.hi)
    C.flash_attn_fwd(s["q"].view, s["k"].view, s["v"].view, s["o"].view, lse.view, float(c.softmax_scale), bool(c.causal),
                     int(c.offset), *_drop_args(c), *extra)
    torch.cuda.synchronize()
    s["o"].assert_outside_untouched(f"{c} o")
    lse.assert_outside_untouched(f"{c} lse")
    return dict(o=s["o"].view, lse=lse.view)


def run_backward(C, c, t):
    s = _slots(c, ("q", "k", "v", "o", "do", "dq", "dk", "dv"))
    for n in ("q", "k", "v", "o", "do"):
        s[n].fill(t[n].to(DEV))
    lse = t["lse"].to(DEV).contiguous()
    kr = A.key_ranges(c, DEV)
    extra = () if kr is None else (kr.lo, kr.hi, *kr.transposed())
    outs = ("dq", "dk", "dv")
    for n in outs:
        s[n].snapshot()
    try:
        if c.chunk:
            C.flash_attn_set_knob(1, c.chunk)
        got = []
        for _ in range(2):
            for n in outs:
                s[n].buf.copy_(s[n].pristine)
            C.flash_attn_bwd(s["q"].view, s["k"].view, s["v"].view, s["o"].view, s["do"].view, lse, s["dq"].view, s["dk"].view,
                             s["dv"].view, float(c.softmax_scale), bool(c.causal), int(c.offset), *_drop_args(c), *extra)
            torch.cuda.synchronize()
            got.append({n: s[n].view.clone() for n in outs})
    finally:
        C.flash_attn_set_knob(1, -1)
    if c.layout == "fused":                       # dq / dk / dv share one buffer: its only outside is the two NaN rows
        inside = torch.zeros(s["dq"].buf.shape, dtype=torch.bool, device=DEV)
        inside[1:-1] = True
        assert_bit_equal(s["dq"].buf.view(torch.int16)[~inside], s["dq"].pristine.view(torch.int16)[~inside],
                         f"{c} dqkv: bytes outside the output views")
    else:
        for n in outs:
            s[n].assert_outside_untouched(f"{c} {n}")
    for n in ("dk", "dv"):
        assert_bit_equal(got[0][n], got[1][n], f"{c} {n}: two calls")
    return got[1]


def _sweep(cases, worst):
    C = _ext.ext()
    for c in cases:
        t = A.make_inputs(c)
        ref = A.reference(c, t, DEV)
        got = (run_forward if c.kind == "fwd" else run_backward)(C, c, t)
        worst(c, A.check_outputs(c, got, ref))


_ids = lambda cs: cs[0].name


@pytest.mark.parametrize("cases", A.group(A.forward_cases(), 16), ids=_ids)
def test_forward(cases, worst):
    _sweep(cases, worst)


@pytest.mark.parametrize("cases", A.group(A.range_cases(), 12), ids=_ids)
def test_forward_ranges(cases, worst):
    _sweep(cases, worst)


@pytest.mark.parametrize("cases", A.group(A.dropout_cases(), 12), ids=_ids)
def test_forward_dropout(cases, worst):
    _sweep(cases, worst)


@pytest.mark.parametrize("cases", A.group(A.backward_cases(), 10), ids=_ids)
def test_backward(cases, worst):
    _sweep(cases, worst)


# ---- the Python entry points ---------------------------------------------------------------------

def _dev_inputs(c):
    return {n: x.to(DEV) for n, x in A.make_inputs(c).items()}


def _bwd_ref_from_kernel(c, t, o, lse, do):
    t = dict(t, o=o.detach(), lse=lse.detach(), do=do)
    return A.reference(replace(c, kind="bwd"), t, DEV)


def test_flash_attn_func_end_to_end(worst):
    c = Case("fwd", D=128, B=2, Sq=129, Sk=193, Hq=4, Hkv=1, ranges=(A.R_SMALL, ("window", 65)))
    t = _dev_inputs(c)
    kr = A.key_ranges(c, DEV)
    q, k, v = (t[n].clone().requires_grad_(True) for n in "qkv")
    o = ops.flash_attn_func(q, k, v, causal=True, key_ranges=kr)
    lse = ops.flash_attn_fwd_lse(t["q"], t["k"], t["v"], causal=True, key_ranges=kr)[1]
    worst(c, A.check_outputs(c, dict(o=o, lse=lse), A.reference(c, t, DEV)))
    do = torch.randn(o.shape, generator=torch.Generator().manual_seed(5), dtype=F32).to(BF16).to(DEV)
    o.backward(do)
    cb = replace(c, kind="bwd")
    worst(cb, A.check_outputs(cb, dict(dq=q.grad, dk=k.grad, dv=v.grad), _bwd_ref_from_kernel(c, t, o, lse, do)))


def test_flash_attn_fwd_lse_into_given_output(worst):
    c = Case("fwd", D=64, B=2, Sq=65, Sk=129, Hq=8, Hkv=1, off=3, scale=0.2)
    t = _dev_inputs(c)
    out = Slot.make((c.B, c.Sq, c.Hq, c.D), DEV, "sbhd")
    out.snapshot()
    o, lse = ops.flash_attn_fwd_lse(t["q"], t["k"], t["v"], causal=True, softmax_scale=0.2, causal_offset=3, out=out.view)
    assert o.data_ptr() == out.view.data_ptr()
    out.assert_outside_untouched("flash_attn_fwd_lse out")
    worst(c, A.check_outputs(c, dict(o=o, lse=lse), A.reference(c, t, DEV)))


def test_attention_with_dropout_end_to_end(worst):
    c = Case("fwd", D=64, B=2, Sq=65, Sk=129, Hq=4, Hkv=2, drop=(0.1, 4242, 4))
    t = _dev_inputs(c)
    q, k, v = (t[n].transpose(1, 2).clone().requires_grad_(True) for n in "qkv")          # bhsd
    o = attention_with_dropout(q, k, v, 0.1, causal=True, seed=4242, head_offset=4)
    lse = torch.empty(c.B, c.Hq, c.Sq, dtype=F32, device=DEV)
    o2 = torch.empty_like(t["q"])
    _ext.ext().flash_attn_fwd(t["q"], t["k"], t["v"], o2, lse, c.softmax_scale, True, c.offset, 0.1, 4242, 4)
    assert_bit_equal(o.transpose(1, 2), o2, "attention_with_dropout against the binding")
    worst(c, A.check_outputs(c, dict(o=o.transpose(1, 2), lse=lse), A.reference(c, t, DEV)))
    do = torch.randn(o2.shape, generator=torch.Generator().manual_seed(6), dtype=F32).to(BF16).to(DEV)
    o.backward(do.transpose(1, 2))
    cb = replace(c, kind="bwd")
    got = dict(dq=q.grad.transpose(1, 2), dk=k.grad.transpose(1, 2), dv=v.grad.transpose(1, 2))
    worst(cb, A.check_outputs(cb, got, _bwd_ref_from_kernel(c, t, o2, lse, do)))


def test_rope_attention_end_to_end(worst):
    """Identity rotation (cos = 1, sin = 0): RoPE is exact, so the fused-QKV plumbing of
    rope_attention (strided q / k / v views, o into [S, B, Hq D], one fused dQKV) is what is judged."""
    c = Case("fwd", D=128, B=2, Sq=161, Sk=161, Hq=4, Hkv=2, layout="fused")
    t = _dev_inputs(c)
    S, B, D = c.Sq, c.B, c.D
    qkv0 = torch.cat([t[n].permute(1, 0, 2, 3).reshape(S, B, -1) for n in "qkv"], dim=-1).contiguous()
    leaf = qkv0.clone().requires_grad_(True)
    cos_t, sin_t = torch.ones(S, D // 2, device=DEV), torch.zeros(S, D // 2, device=DEV)
    o = ops.rope_attention(leaf.clone(), cos_t, sin_t, c.Hq, c.Hkv, D)
    o4 = o.view(S, B, c.Hq, D).permute(1, 0, 2, 3)
    lse = ops.flash_attn_fwd_lse(t["q"], t["k"], t["v"], causal=True)[1]
    worst(c, A.check_outputs(c, dict(o=o4, lse=lse), A.reference(c, t, DEV)))
    do = torch.randn(o.shape, generator=torch.Generator().manual_seed(7), dtype=F32).to(BF16).to(DEV)
    o.backward(do)
    g = leaf.grad.view(S, B, c.Hq + 2 * c.Hkv, D).permute(1, 0, 2, 3)
    got = dict(dq=g[:, :, :c.Hq], dk=g[:, :, c.Hq:c.Hq + c.Hkv], dv=g[:, :, c.Hq + c.Hkv:])
    cb = replace(c, kind="bwd")
    worst(cb, A.check_outputs(cb, got, _bwd_ref_from_kernel(c, t, o4, lse, do.view(S, B, c.Hq, D).permute(1, 0, 2, 3))))
