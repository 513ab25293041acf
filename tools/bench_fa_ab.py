"""FA forward and backward TFLOP/s at the bench's attention shapes, for A/B of kernel builds: --root
picks the directory the package is imported from (e.g. a copy built from another commit).  One JSON
line per shape: median (and min / max) over rounds of the mean of `reps` launches, the relative error
of o / dq / dk / dv against an fp32 reference of the last 64 query rows, and a digest of the dK / dV
bits of the timed backward (seeded inputs: two builds with the same arithmetic order agree)."""
import argparse
import hashlib
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=".")
ap.add_argument("--tag", default="")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: E402

import neuronx_distributed_llama3_2_amd.ops as ops  # noqa: E402

assert os.path.abspath(ops.__file__).startswith(os.path.abspath(a.root)), ops.__file__


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def rel(x, ref):
    return round(((x.float() - ref).abs().max() / ref.abs().max()).item(), 5)


def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.contiguous().view(torch.int16).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


torch.manual_seed(0)
# (B, S, Hq, Hkv, D): the TP=1 bench micro-step (2 x 8192, 32 / 8 heads), the TP=8 rank (8 x 8192, 4 / 1),
# Llama-3.2-1B prefill (D = 64)
for (B, S, H, Hkv, D) in [(2, 8192, 32, 8, 128), (8, 8192, 4, 1, 128), (1, 8192, 32, 8, 64)]:
    q = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    fl = 4.0 * B * H * S * S * D * 0.5
    o = ops.flash_attn_func(q, k, v, causal=True)
    # fp32 check of the last 64 query rows (the longest sweeps); with dO zero on every other row they
    # are also the only rows that reach dK / dV
    ref_rows = slice(S - 64, S)
    do_tail = torch.zeros_like(do)
    do_tail[:, ref_rows] = do[:, ref_rows]
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do_tail, retain_graph=True)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q[:, ref_rows], k, v))
    sc = torch.einsum("bqhd,bkhd->bhqk", qr, kr.repeat_interleave(H // Hkv, dim=2)) * D ** -0.5
    pos_q = torch.arange(S - 64, S, device="cuda")[:, None]
    sc = sc.masked_fill(torch.arange(S, device="cuda")[None, :] > pos_q, float("-inf"))
    ref = torch.einsum("bhqk,bkhd->bqhd", sc.softmax(-1), vr.repeat_interleave(H // Hkv, dim=2))
    rdq, rdk, rdv = torch.autograd.grad(ref, (qr, kr, vr), do[:, ref_rows].float())
    errs = {"rel_err": rel(o[:, ref_rows], ref.detach()), "dq_err": rel(dq[:, ref_rows], rdq), "dk_err": rel(dk, rdk),
            "dv_err": rel(dv, rdv)}
    del sc, ref, rdq, rdk, rdv, qr, kr, vr

    def bwd():
        return torch.autograd.grad(o, (q, k, v), do, retain_graph=True)

    tf_ = [timed(lambda: ops.flash_attn_fwd_lse(q, k, v, causal=True), a.reps) for _ in range(a.rounds)]
    tb_ = [timed(bwd, a.reps) for _ in range(a.rounds)]
    _, dk, dv = bwd()
    ms, mb = statistics.median(tf_), statistics.median(tb_)
    print(json.dumps({"tag": a.tag, "B": B, "S": S, "H": H, "Hkv": Hkv, "D": D, "fwd_ms": round(ms, 4),
                      "fwd_tf": round(fl / ms / 1e9, 1), "bwd_ms": round(mb, 4), "bwd_min": round(min(tb_), 4),
                      "bwd_max": round(max(tb_), 4), "bwd_tf": round(2.5 * fl / mb / 1e9, 1), **errs,
                      "dkdv_sha": digest(dk, dv)}), flush=True)
