"""Fused decode launches over MXFP4 weights (dgemv_mx: csrc/decode_fused_mx.hip at 1-3 rows, csrc/decode_fused_mx_mfma.hip
at 4-16) on one MI355X against what each replaces and against the bf16 fused launch of the same shape, on the
Llama-3.2-1B / Llama-3-8B decode projections at 1-16 activation rows (--rows, default 1,2,3):

  fused     one dgemv_mx launch: o_proj / down with the residual add, gate_up with RMSNorm + SwiGLU, norm + lm_head,
            qkv with RMSNorm, RoPE and the KV-cache write
  unfused   the launches it replaces: rms_norm + mx_gemv (gate_up, lm_head), mx_gemv + add (o_proj, down); from 4 rows
            mx_gemm (csrc/gemv_mx_mfma.hip) in place of mx_gemv, as ops.mx_linear routes them; qkv: rms_norm + mx_gemv /
            mx_gemm + rope_inplace_ + kv_cache_write
  bf16      dgemv (csrc/decode_fused.hip) with bf16 weights, same epilogue and prologue; it ends at 8 rows and at
            M * K <= 32768 with a norm, beyond that the variant is left out

The kernels are called directly, so the result does not depend on NXD_DECODE_FUSED_MX or NXD_DECODE_FUSED_MX_ROWS.  The variants alternate in
one process; each is a captured hipGraph of calls that rotate over more than 512 MiB of weight copies (the Infinity
Cache holds 256 MiB), so every call streams its weights from HBM.  One JSON line per (shape, rows, variant): median
time per call over the rounds, its min / max (the run-to-run spread), the bytes the call must move (weights,
scales, activations in and out) and the rate that gives."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from neuronx_distributed_llama3_2_amd.ops import ext, kv_cache_write, rms_norm, rope_inplace_  # noqa: E402

PLAIN, RESID, GLU, QKV = 0, 1, 2, 3
MODELS = {"llama3.2-1b": (2048, 8192, 128256), "llama3-8b": (4096, 14336, 128256)}   # hidden, intermediate, vocabulary
HEADS = {2048: (32, 8, 64), 4096: (32, 8, 128)}   # by hidden size: q heads, kv heads, head dim
LMAX = 64   # positions of the qkv shape's KV caches; every row writes position 7 of its own sequence
_ROPE = {}
ROTATE_BYTES = 512 << 20
EPS = 1e-5
CFG = 0   # --cfg: force dgemv_mx's rows per wave R and k-slices KS (16 R + KS); 0 = the launcher's choice


def shapes(model):
    H, I, V = MODELS[model]   # op, epilogue, K, weight rows
    nq, nkv, D = HEADS[H]
    return [("o_proj", RESID, H, H), ("gate_up", GLU, H, 2 * I), ("down", RESID, I, H), ("lm_head", PLAIN, H, V),
            ("qkv", QKV, H, (nq + 2 * nkv) * D)]


def rope_operands(M, K):
    """cos / sin tables, positions and the bf16 KV caches of the qkv shape at M rows (one token per sequence)."""
    if (M, K) not in _ROPE:
        nq, nkv, D = HEADS[K]
        ang = torch.rand(LMAX, D // 2, device="cuda") * 6.28
        _ROPE[(M, K)] = dict(nq=nq, nkv=nkv, D=D, cos_t=ang.cos(), sin_t=ang.sin(), T=1,
                             pos=torch.full((M,), 7, dtype=torch.int64, device="cuda"),
                             kc=torch.zeros(M, nkv, LMAX, D, device="cuda", dtype=torch.bfloat16),
                             vc=torch.zeros(M, nkv, LMAX, D, device="cuda", dtype=torch.bfloat16))
    return _ROPE[(M, K)]


def weight_bytes(kind, Nw, K):
    return Nw * K * 2 if kind == "bf16" else Nw * K // 2 + Nw * K // 32


def make_weights(kind, Nw, K, copies):
    if kind == "bf16":
        return [(torch.randn(Nw, K, device="cuda", dtype=torch.bfloat16) * 0.02,) for _ in range(copies)]
    return [(torch.randint(0, 256, (Nw, K // 2), device="cuda", dtype=torch.uint8),
             torch.randint(120, 128, (Nw, K // 32), device="cuda", dtype=torch.uint8)) for _ in range(copies)]


def call(kind, epi, x, nw, w, res):
    """One projection; res is the [M, N] residual stream of the RESID forms (updated in place)."""
    C = ext()
    M, N = x.shape[0], w[0].shape[0] // (2 if epi == GLU else 1)
    y = res if epi == RESID else torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    norm = None if epi == RESID else nw
    if epi == QKV:
        r = rope_operands(M, x.shape[1])
        if kind == "fused":
            C.dgemv_mx(epi, x, nw, EPS, w[0], w[1], y, CFG, **r)
        elif kind == "bf16":
            C.dgemv(epi, x, nw, EPS, w[0], y, r["nq"], r["nkv"], r["D"], r["cos_t"], r["sin_t"], r["pos"], 1, r["kc"], r["vc"], None)
        else:
            (C.mx_gemv if M <= 3 else C.mx_gemm)(rms_norm(x, nw, EPS)[0], w[0], w[1], None, y, False)
            rope_inplace_(y, 0, r["nq"] + r["nkv"], r["D"], r["cos_t"], r["sin_t"], r["pos"])
            h = y.view(M, 1, r["nq"] + 2 * r["nkv"], r["D"])
            kv_cache_write(h[:, :, r["nq"]:r["nq"] + r["nkv"]], h[:, :, r["nq"] + r["nkv"]:], r["kc"], r["vc"], r["pos"].to(torch.int32))
    elif kind == "fused":
        C.dgemv_mx(epi, x, norm, EPS, w[0], w[1], y, CFG)
    elif kind == "bf16":
        C.dgemv(epi, x, norm, EPS, w[0], y, 0, 0, 0, None, None, None, 1, None, None, None)
    else:
        mx = C.mx_gemv if M <= 3 else C.mx_gemm
        if epi == RESID:
            t = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
            mx(x, w[0], w[1], None, t, False)
            res.add_(t)
        else:
            mx(rms_norm(x, nw, EPS)[0], w[0], w[1], None, y, epi == GLU)
    return y


def runs(kind, epi, M, K):
    """Whether the variant exists at this shape (only the bf16 launch has limits inside 16 rows)."""
    return kind != "bf16" or (M <= 8 and (epi == RESID or M * K <= 32768))


def capture(kind, epi, x, nw, ws, res, inner):
    for w in ws:   # warm every buffer the graph uses
        call(kind, epi, x, nw, w, res)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(inner):
            call(kind, epi, x, nw, ws[i % len(ws)], res)
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
    ap.add_argument("--rows", default="1,2,3")
    ap.add_argument("--only", default=None, help="model name filter")
    ap.add_argument("--ops", default=None, help="comma-separated projection filter (o_proj,gate_up,down,lm_head,qkv)")
    ap.add_argument("--kinds", default="fused,unfused,bf16")
    ap.add_argument("--cfg", type=int, default=0, help="force dgemv_mx's rows per wave R and k-slices KS: 16 R + KS")
    a = ap.parse_args()
    global CFG
    CFG = a.cfg
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_decode needs a GPU")
    rows = [int(m) for m in a.rows.split(",")]
    if any(not 1 <= m <= 16 for m in rows):
        raise SystemExit("--rows: 1..16")
    all_kinds = tuple(a.kinds.split(","))
    sink = open(a.out, "a") if a.out else None
    for model in MODELS:
        if a.only and a.only != model:
            continue
        for op, epi, K, Nw in shapes(model):
            if a.ops and op not in a.ops.split(","):
                continue
            N = Nw // 2 if epi == GLU else Nw
            weights = {k: make_weights(k, Nw, K, max(2, -(-ROTATE_BYTES // weight_bytes(k, Nw, K)))) for k in all_kinds}
            nw = torch.ones(K, device="cuda", dtype=torch.bfloat16)
            for M in rows:
                kinds = tuple(k for k in all_kinds if runs(k, epi, M, K))
                x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
                res = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
                inner = {k: 4 * len(weights[k]) for k in kinds}
                graphs = {k: capture(k, epi, x, nw, weights[k], res, inner[k]) for k in kinds}
                # replays sized for a window of about 30 ms per sample
                reps = {k: max(3, int(30000.0 / max(time_graph(graphs[k], 3), 1.0))) for k in kinds}
                samples = {k: [] for k in kinds}
                for _ in range(a.rounds):
                    for k in kinds:   # alternate the variants
                        samples[k].append(time_graph(graphs[k], reps[k]) / inner[k])
                for k in kinds:
                    us = statistics.median(samples[k])
                    # what the call must move: weights (+ scales), x, the norm weight, y (RESID: read and written)
                    nbytes = weight_bytes(k, Nw, K) + 2 * (M * K + (0 if epi == RESID else K) + M * N * (2 if epi == RESID else 1))
                    rec = {"model": model, "op": op, "K": K, "Nw": Nw, "M": M, "variant": k, "us": round(us, 2),
                           "us_min": round(min(samples[k]), 2), "us_max": round(max(samples[k]), 2), "bytes": nbytes,
                           "TBps": round(nbytes / us / 1e6, 3), "rounds": a.rounds, "copies": len(weights[k])}
                    if k == "fused" and a.cfg:
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
