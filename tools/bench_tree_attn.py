"""Tree-verification attention A/B on one MI355X: ops.tree_attention on csrc/tree_attn.hip against the same
call with NXD_TREE_ATTN=0 (the plain-PyTorch arithmetic forward_tree ran before the kernel), Llama-3.2-1B
(32/8 heads, D 64) and Llama-3-8B (32/8, D 128) shapes, the default Medusa tree (11 nodes) and a 64-node
tree, prefixes of 128, 2,048 and 32,000 cached keys.

The two routes alternate in one process, eager (the NXD_TREE_ATTN=0 route slices by the Python prefix_len, so
it cannot be captured), cycling over enough layer caches to exceed the 256 MiB Infinity Cache where one
layer's prefix is large.  The kernel route gets prefix_len as a device tensor and the packed mask, the other
route a Python int and the bool mask (no host read: the arithmetic as forward_tree ran it before the kernel).

The figure is time per call between two device events around an eager Python loop of calls: it includes the
host's launch work (Python dispatch, the partials' allocation, hipFuncSetAttribute), so where the kernel is
short (small prefixes) it is the rate at which the host can issue the call, not kernel time.  One JSON line
per (shape, nodes, prefix, route): its median over the rounds, min / max, and the largest difference between
the two routes' outputs."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
import neuronx_distributed_llama3_2_amd.ops as ops  # noqa: E402

SHAPES = [("llama3.2-1b 32/8 D64", 32, 8, 64), ("llama3-8b 32/8 D128", 32, 8, 128)]
PREFIXES = [(128, 2304), (2048, 2304), (32000, 32768)]   # cached keys, cache length
ROTATE_BYTES = 512 << 20


def time_calls(fn, layers, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(reps):
        fn(layers[i % len(layers)])
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / reps   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--nodes", default="11,64")
    ap.add_argument("--prefixes", default="128,2048,32000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tree_attn needs a GPU")
    sink = open(a.out, "a") if a.out else None
    for name, Hq, Hkv, D in SHAPES:
        for prefix, Lmax in (p for p in PREFIXES if str(p[0]) in a.prefixes.split(",")):
            copies = max(2, min(32, -(-ROTATE_BYTES // (2 * Hkv * prefix * D * 2))))
            layers = [torch.randn(2, 1, Hkv, Lmax, D, device="cuda", dtype=torch.bfloat16) for _ in range(copies)]
            plen = torch.tensor([prefix], dtype=torch.int32, device="cuda")
            for N in (int(n) for n in a.nodes.split(",")):
                torch.manual_seed(N)
                qkv = torch.randn(1, N, Hq + 2 * Hkv, D, device="cuda", dtype=torch.bfloat16)
                q, k, v = qkv[:, :, :Hq], qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:]
                mask = torch.eye(N, dtype=torch.bool)
                for j in range(1, N):   # a random tree: self + ancestors
                    mask[j] |= mask[int(torch.randint(0, j, (1,)))]
                routes = {"kernel": ("1", ops.pack_tree_mask(mask.cuda()), plen), "torch": ("0", mask.cuda(), prefix)}
                out = torch.empty_like(q)

                def run(route, layer):
                    os.environ["NXD_TREE_ATTN"] = routes[route][0]
                    return ops.tree_attention(q, k, v, routes[route][1], layer[0], layer[1], routes[route][2], out=out)

                outs = {r: run(r, layers[0]).float().clone() for r in routes}
                diff = (outs["kernel"] - outs["torch"]).abs().max().item()
                reps = {}
                for r in routes:   # warm-up on every layer cache, then size the timed window to ~30 ms
                    time_calls(lambda layer: run(r, layer), layers, len(layers))
                    reps[r] = max(3, min(400, int(30000.0 / max(time_calls(lambda layer: run(r, layer), layers, 3), 1.0))))
                samples = {r: [] for r in routes}
                for _ in range(a.rounds):
                    for r in routes:   # alternate the routes
                        samples[r].append(time_calls(lambda layer: run(r, layer), layers, reps[r]))
                # the kernel route alone, captured (8 calls per layer cache in one hipGraph): device time per call
                # with no host work between the launches
                os.environ["NXD_TREE_ATTN"] = "1"
                graph, inner = torch.cuda.CUDAGraph(), 8 * len(layers)
                with torch.cuda.graph(graph):
                    for i in range(inner):
                        run("kernel", layers[i % len(layers)])
                graph_us = []
                for _ in range(a.rounds):
                    graph_us.append(time_calls(lambda _l: graph.replay(), layers, 3) / inner)
                for r in routes:
                    extra = {"us_per_call_in_graph_median": round(statistics.median(graph_us), 2)} if r == "kernel" else {}
                    rec = {**extra, "what": f"tree_attention {name} B=1 Hq={Hq} Hkv={Hkv} D={D} N={N} cache={Lmax} prefix={prefix}",
                           "route": r, "NXD_TREE_ATTN": routes[r][0],
                           "timed": "device events around an eager loop (host launch work included)",
                           "us_per_call_median": round(statistics.median(samples[r]), 2),
                           "us_per_call_min": round(min(samples[r]), 2), "us_per_call_max": round(max(samples[r]), 2),
                           "calls_per_sample": reps[r], "rounds": a.rounds, "layer_caches": len(layers),
                           "max_abs_diff_between_routes": diff}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if sink:
                        sink.write(line + "\n")
                        sink.flush()
            del layers
            torch.cuda.empty_cache()
    os.environ.pop("NXD_TREE_ATTN", None)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
