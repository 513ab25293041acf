"""Flash attention forward / backward time of plain causal attention against packed documents
(interval mask, ops/attention_ranges.py) at the headline shape: B=2, S=8192, 32 / 8 heads, D=128.
One JSON line per case; the cases are interleaved round by round so they share the machine's state.

    python tools/bench_attention_ranges.py [--cases causal,docs512,docs1024,docs2048] [--rounds 7] [--label X]

`--cases causal` runs on an extension built before the interval mask existed (the baseline side of
the "existing path did not slow down" comparison).  live_frac is the share of the causal triangle's
(query, key) pairs that the mask keeps: the ideal time ratio against plain causal.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuronx_distributed_llama3_2_amd import ops  # noqa: E402

B, S, HQ, HKV, D = 2, 8192, 32, 8, 128
INNER = 10


def _ranges(case, dev):
    if case == "causal":
        return None
    n = int(case[len("docs"):])
    st = torch.zeros(B, S, dtype=torch.bool, device=dev)
    st[:, ::n] = True
    return ops.ranges_from_document_starts(st)


def _timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / INNER


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="causal,docs512,docs1024,docs2048")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda"
    ext = ops.ext()
    cases = a.cases.split(",")
    torch.manual_seed(0)
    q = torch.randn(B, S, HQ, D, device=dev, dtype=torch.bfloat16)
    k = torch.randn(B, S, HKV, D, device=dev, dtype=torch.bfloat16)
    v = torch.randn(B, S, HKV, D, device=dev, dtype=torch.bfloat16)
    do = torch.randn_like(q)
    scale = D ** -0.5
    state = {}
    for c in cases:
        kr = _ranges(c, dev)
        extra_f = () if kr is None else (0.0, 0, 0, kr.lo, kr.hi)
        extra_b = () if kr is None else (0.0, 0, 0, kr.lo, kr.hi, kr.q_lo, kr.q_hi)
        o = torch.empty_like(q)
        lse = torch.empty(B, HQ, S, dtype=torch.float32, device=dev)
        ext.flash_attn_fwd(q, k, v, o, lse, scale, True, 0, *extra_f)
        grads = (torch.empty_like(q), torch.empty_like(k), torch.empty_like(v))
        live = 1.0 if kr is None else float(kr.dense_mask(causal=True)[0].sum()) / (S * (S + 1) / 2)
        state[c] = dict(o=o, lse=lse, grads=grads, extra_f=extra_f, extra_b=extra_b, live=live, fwd=[], bwd=[])
    for _ in range(a.rounds + 1):       # the first round is warm-up
        for c in cases:
            st = state[c]
            st["fwd"].append(_timed(lambda: ext.flash_attn_fwd(q, k, v, st["o"], st["lse"], scale, True, 0, *st["extra_f"])))
            st["bwd"].append(_timed(lambda: ext.flash_attn_bwd(q, k, v, st["o"], do, st["lse"], *st["grads"], scale, True, 0,
                                                               *st["extra_b"])))
    for c in cases:
        st = state[c]
        rec = {"case": c, "label": a.label, "B": B, "S": S, "Hq": HQ, "Hkv": HKV, "D": D, "live_frac": round(st["live"], 4)}
        for side, mult in (("fwd", 4), ("bwd", 10)):
            t = sorted(st[side][1:])
            med = t[len(t) // 2]
            rec[f"{side}_ms"] = round(med, 4)
            rec[f"{side}_min_ms"] = round(t[0], 4)
            rec[f"{side}_max_ms"] = round(t[-1], 4)
            # FLOPs of the pairs the mask keeps (the causal triangle for plain causal)
            rec[f"{side}_tflops"] = round(mult * B * HQ * (S * (S + 1) / 2) * st["live"] * D / med / 1e9, 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
