"""Decode attention A/B on one MI355X: ops.decode_attention over an MXFP8 KV cache (KV8 form of
csrc/decode_attn.hip) against the bf16 cache, Llama-3-8B-like (32/8 heads, D 128) and Llama-3.2-1B
(32/8, D 64) shapes at batch 1 and 8, caches filled to 2,048 and 32,000 keys, window 0 and 4,096.

The two cache kinds alternate in one process.  Each is a captured hipGraph of calls (attention + merge
launches) that cycle over enough layer caches to exceed the 256 MiB Infinity Cache, so every call
streams its keys from HBM.  One JSON line per (shape, batch, fill, window, kind): median device time per
call, the K/V (+ scale) bytes a call has to read, bytes per second and the run-to-run spread.

`--kinds bf16` runs the bf16 cache alone: it needs nothing of the MXFP8 interface, so the same file
measures an older checkout (run it with that checkout as the working directory)."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
import neuronx_distributed_llama3_2_amd.ops as ops  # noqa: E402

SHAPES = [("32/8 D128", 32, 8, 128), ("llama3.2-1b 32/8 D64", 32, 8, 64)]
FILLS = [(2048, 2304), (32000, 32768)]     # keys filled, cache length
ROTATE_BYTES = 512 << 20


def layer_bytes(kind, B, Hkv, Lmax, D):
    per = 2 if kind == "bf16" else 1
    return 2 * B * Hkv * Lmax * (D * per + (D // 32 if kind == "mxfp8" else 0))


def make_layers(kind, B, Hkv, Lmax, D, copies):
    out = []
    for _ in range(copies):
        if kind == "bf16":
            out.append((torch.randn(B, Hkv, Lmax, D, device="cuda", dtype=torch.bfloat16),
                        torch.randn(B, Hkv, Lmax, D, device="cuda", dtype=torch.bfloat16), {}))
        else:
            def codes():
                c = torch.randint(0, 256, (B, Hkv, Lmax, D), device="cuda", dtype=torch.uint8)
                return c & 0x77   # positive codes below 2: no NaN code
            sc = lambda: torch.randint(116, 120, (B, Hkv, Lmax, D // 32), device="cuda", dtype=torch.uint8)
            out.append((codes(), codes(), {"k_scale": sc(), "v_scale": sc()}))
    return out


def capture(q, layers, seq, window, o, inner):
    for kc, vc, kw in layers:
        ops.decode_attention(q, kc, vc, seq, out=o, window=window, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(inner):
            kc, vc, kw = layers[i % len(layers)]
            ops.decode_attention(q, kc, vc, seq, out=o, window=window, **kw)
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
    ap.add_argument("--kinds", default="bf16,mxfp8")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--fills", default="2048,32000")
    ap.add_argument("--windows", default="0,4096")
    ap.add_argument("--tag", default="branch", help="recorded as 'code' in every line")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_cache needs a GPU")
    sink = open(a.out, "a") if a.out else None
    kinds = tuple(a.kinds.split(","))
    fills = [f for f in FILLS if str(f[0]) in a.fills.split(",")]
    for name, Hq, Hkv, D in SHAPES:
        for B in (int(b) for b in a.batches.split(",")):
            for filled, Lmax in fills:
                layers = {k: make_layers(k, B, Hkv, Lmax, D, max(2, -(-ROTATE_BYTES // layer_bytes(k, B, Hkv, Lmax, D))))
                          for k in kinds}
                torch.manual_seed(0)
                q = torch.randn(B, 1, Hq, D, device="cuda", dtype=torch.bfloat16)
                o = torch.empty_like(q)
                seq = torch.full((B,), filled, device="cuda", dtype=torch.int32)
                for window in (int(w) for w in a.windows.split(",")):
                    if window >= filled:
                        continue
                    inner = {k: 8 * len(layers[k]) for k in kinds}
                    graphs = {k: capture(q, layers[k], seq, window or None, o, inner[k]) for k in kinds}
                    reps = {k: max(3, int(30000.0 / max(time_graph(graphs[k], 3), 1.0))) for k in kinds}
                    samples = {k: [] for k in kinds}
                    for _ in range(a.rounds):
                        for k in kinds:   # alternate the kinds
                            samples[k].append(time_graph(graphs[k], reps[k]) / inner[k])
                    for k in kinds:
                        us = statistics.median(samples[k])
                        visible = min(filled, window) if window else filled
                        nbytes = layer_bytes(k, B, Hkv, visible, D)
                        rec = {"what": f"decode_attention {name} B={B} Hq={Hq} Hkv={Hkv} D={D} cache={Lmax} filled={filled} T=1",
                               "code": a.tag, "kv_cache": k, "window": window or None, "us_per_call_median": round(us, 3),
                               "us_per_call_min": round(min(samples[k]), 3), "us_per_call_max": round(max(samples[k]), 3),
                               "kv_bytes_visible": nbytes, "TBps": round(nbytes / us / 1e6, 3), "rounds": a.rounds,
                               "layer_caches": len(layers[k])}
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if sink:
                            sink.write(line + "\n")
                            sink.flush()
                    del graphs
                del layers
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
