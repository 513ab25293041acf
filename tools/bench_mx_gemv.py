"""Decode projection A/B on one MI355X: MXFP4 weights on the VALU kernel (mx_gemv, csrc/gemv_mx.hip;
above its 8 rows mx_dequant + GEMM, the route without an MFMA form) and on MFMA weight tiles
(mx_gemm, csrc/gemv_mx_mfma.hip) against skinny_linear with int8 and with bf16 weights
(csrc/gemv.hip) on Llama-3.2-1B / Llama-3-8B projection shapes at 1..16 activation rows.  The two
MXFP4 kernels are called directly, so the result does not depend on the routing knob NXD_MX_MFMA.

The four variants alternate in one process.  Each is a captured hipGraph of calls that rotate over
enough weight copies to exceed the 256 MiB Infinity Cache, so every call streams its weights from
HBM.  One JSON line per (shape, rows, variant): median time per call, weight bytes per second and
the run-to-run spread (min / max over the rounds)."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from neuronx_distributed_llama3_2_amd.ops import ext, swiglu  # noqa: E402
from neuronx_distributed_llama3_2_amd.ops.gemm import linear  # noqa: E402
from neuronx_distributed_llama3_2_amd.ops.gemv import dequantize_mxfp4, skinny_linear  # noqa: E402

SHAPES = [  # model, op, K, weight rows, glu
    ("llama3.2-1b", "qkv", 2048, 3072, False),
    ("llama3.2-1b", "gate_up", 2048, 2 * 8192, True),
    ("llama3.2-1b", "down", 8192, 2048, False),
    ("llama3.2-1b", "lm_head", 2048, 128256, False),
    ("llama3-8b", "gate_up", 4096, 2 * 14336, True),
    ("llama3-8b", "down", 14336, 4096, False),
    ("llama3-8b", "lm_head", 4096, 128256, False),
]
ROTATE_BYTES = 512 << 20


def weight_bytes(kind, Nw, K):
    return {"mxfp4": Nw * K // 2 + Nw * K // 32, "int8": Nw * K + Nw * 4, "bf16": Nw * K * 2}[kind.split("_")[0]]


def make_weights(kind, Nw, K, copies):
    dev = "cuda"
    ws = []
    for _ in range(copies):
        if kind.startswith("mxfp4"):
            ws.append((torch.randint(0, 256, (Nw, K // 2), device=dev, dtype=torch.uint8),
                       torch.randint(120, 128, (Nw, K // 32), device=dev, dtype=torch.uint8)))
        elif kind == "int8":
            ws.append((torch.randint(-127, 128, (Nw, K), device=dev, dtype=torch.int8),
                       torch.rand(Nw, device=dev) * 1e-3))
        else:
            ws.append((torch.randn(Nw, K, device=dev, dtype=torch.bfloat16) * 0.02, None))
    return ws


MFMA_CFG = 0   # --cfg: force tiles per wave / K split of mx_gemm (16 T + KS), 0 = the launcher's choice


def call(kind, x, w, glu):
    if kind.startswith("mxfp4"):
        M, N = x.shape[0], w[0].shape[0] // (2 if glu else 1)
        if kind == "mxfp4" and M > 8:   # no VALU form: dequantise the whole weight, then the GEMM
            y = linear(x, dequantize_mxfp4(w[0], w[1], x.dtype), None)
            return swiglu(y) if glu else y
        y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
        if kind == "mxfp4":
            ext().mx_gemv(x, w[0], w[1], None, y, glu)
        else:
            ext().mx_gemm(x, w[0], w[1], None, y, glu, MFMA_CFG)
        return y
    return skinny_linear(x, w[0], w[1], glu=glu)


def capture(kind, x, ws, glu, inner):
    for w in ws:   # warm every buffer the graph uses
        call(kind, x, w, glu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(inner):
            call(kind, x, ws[i % len(ws)], glu)
    g.replay()
    torch.cuda.synchronize()
    return g


def time_graph(g, replays):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / replays   # us per replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", default="1,4,8")
    ap.add_argument("--only", default=None, help="model name filter")
    ap.add_argument("--kinds", default="mxfp4,mxfp4_mfma,int8,bf16")
    ap.add_argument("--cfg", type=int, default=0, help="force mx_gemm's tiles per wave T and K split KS: 16 T + KS")
    a = ap.parse_args()
    global MFMA_CFG
    MFMA_CFG = a.cfg
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_gemv needs a GPU")
    sink = open(a.out, "a") if a.out else None
    kinds = tuple(a.kinds.split(","))
    if any(not 1 <= int(m) <= 16 for m in a.rows.split(",")):
        raise SystemExit("--rows: 1..16")
    for model, op, K, Nw, glu in SHAPES:
        if a.only and a.only != model:
            continue
        weights = {}
        for kind in kinds:
            copies = max(2, -(-ROTATE_BYTES // weight_bytes(kind, Nw, K)))
            weights[kind] = make_weights(kind, Nw, K, copies)
        for M in (int(m) for m in a.rows.split(",")):
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            inner = {k: 4 * len(weights[k]) for k in kinds}
            graphs = {k: capture(k, x, weights[k], glu, inner[k]) for k in kinds}
            # replays sized for a window of about 30 ms per sample
            reps = {k: max(3, int(30000.0 / max(time_graph(graphs[k], 3), 1.0))) for k in kinds}
            samples = {k: [] for k in kinds}
            for _ in range(a.rounds):
                for k in kinds:   # alternate the variants
                    samples[k].append(time_graph(graphs[k], reps[k]) / inner[k])
            for k in kinds:
                us = statistics.median(samples[k])
                nbytes = weight_bytes(k, Nw, K)
                rec = {"model": model, "op": op, "K": K, "Nw": Nw, "glu": glu, "M": M, "weights": k,
                       "us": round(us, 2), "us_min": round(min(samples[k]), 2), "us_max": round(max(samples[k]), 2),
                       "weight_bytes": nbytes, "weight_TBps": round(nbytes / us / 1e6, 3), "rounds": a.rounds,
                       "copies": len(weights[k])}
                if k == "mxfp4_mfma" and a.cfg:
                    rec["cfg"] = a.cfg
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
            del graphs
        del weights
        torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
