"""MoE decode projection A/B on one MI355X: the MXFP4 expert kernels (mx_expert_linear /
mx_experts_linear, csrc/gemv_mx.hip; the all-experts form at 8 and 16 rows also on the MFMA weight
tiles of csrc/gemv_mx_mfma.hip) against the bf16 forms (expert_linear, csrc/gemv.hip; the
all-experts matmuls of inference/modeling_moe.py) at the Mixtral-8x7B TP=1 expert shapes, and
with --e2e the decode time per token of a Mixtral-shaped 4-layer random model, bf16 against MXFP4.

Method of tools/bench_mx_gemv.py: the variants alternate in one process; each is a captured hipGraph
of calls that rotate over expert stacks (and, for the selective form, over which experts of a stack
are chosen) holding more than 512 MB, twice the Infinity Cache, so every call streams its weights
from HBM; the median of >= 7 rounds is reported with the min / max over the rounds.  One JSON line
per (op, form, variant), then one line per (op, form) comparing the two."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from neuronx_distributed_llama3_2_amd.ops import ext, swiglu  # noqa: E402
from neuronx_distributed_llama3_2_amd.ops.gemv import dequantize_mxfp4_into, expert_linear, mx_expert_linear  # noqa: E402

E, H, I = 8, 4096, 14336   # Mixtral-8x7B
OPS = [("gate_up", H, 2 * I, True), ("down", I, H, False)]   # op, K, weight rows, glu
ROTATE_BYTES = 512 << 20


def expert_bytes(kind, Nw, K):
    return Nw * K // 2 + Nw * K // 32 if kind.startswith("mxfp4") else Nw * K * 2


def make_stacks(kind, Nw, K):
    copies = max(2, -(-ROTATE_BYTES // (E * expert_bytes(kind, Nw, K))) + 1)
    out = []
    for _ in range(copies):
        if kind == "mxfp4":
            out.append((torch.randint(0, 256, (E, Nw, K // 2), device="cuda", dtype=torch.uint8),
                        torch.randint(120, 128, (E, Nw, K // 32), device="cuda", dtype=torch.uint8)))
        else:
            out.append((torch.randn(E, Nw, K, device="cuda", dtype=torch.bfloat16) * 0.02, None))
    return out


_SCRATCH = {}


def call(kind, form, x, w, eidx, glu):
    if form == "all":
        if kind.startswith("mxfp4"):
            # both bodies called directly, whatever NXD_MX_MFMA routes to: the VALU kernel (at most 8
            # rows; above, the route without an MFMA form: dequantise the stack into a scratch, then
            # the bf16 matmul) and the MFMA weight tiles
            M, N = x.shape[-2], w[0].shape[1] // (2 if glu else 1)
            if kind == "mxfp4" and M > 8:
                key = tuple(w[0].shape)
                if key not in _SCRATCH:
                    _SCRATCH[key] = torch.empty(w[0].shape[:2] + (w[0].shape[2] * 2,), dtype=torch.bfloat16, device="cuda")
                s = _SCRATCH[key]
                dequantize_mxfp4_into(w[0], w[1], s)
                y = torch.matmul(x.unsqueeze(0) if x.dim() == 2 else x, s.transpose(1, 2))
                return swiglu(y) if glu else y
            y = torch.empty((E, M, N), dtype=torch.bfloat16, device="cuda")
            (ext().mx_experts_gemv if kind == "mxfp4" else ext().mx_experts_gemm)(x, w[0], w[1], y, glu)
            return y
        # the bf16 all-experts step of MoEInferenceModel._all_experts on output-major weights
        y = torch.matmul(x.unsqueeze(0) if x.dim() == 2 else x, w[0].transpose(1, 2))
        return swiglu(y) if glu else y
    xdiv = 2 if glu else 1   # gate_up: the two slots of a token share its row; down: one row per pair
    if kind == "mxfp4":
        return mx_expert_linear(x, w[0], w[1], eidx, xdiv=xdiv, glu=glu)
    return expert_linear(x, w[0], eidx, xdiv=xdiv, glu=glu)


def capture(kind, form, x, stacks, eidxs, glu, inner):
    for i in range(len(stacks) * len(eidxs)):   # warm every buffer the graph uses
        call(kind, form, x, stacks[i % len(stacks)], eidxs[i % len(eidxs)], glu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(inner):
            call(kind, form, x, stacks[i % len(stacks)], eidxs[(i // len(stacks)) % len(eidxs)], glu)
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


def emit(rec, sink):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def bench_kernels(a, sink):
    for op, K, Nw, glu in OPS:
        stacks = {k: make_stacks(k, Nw, K) for k in ("mxfp4", "bf16")}
        stacks["mxfp4_mfma"] = stacks["mxfp4"]
        # form, pairs / rows, expert choices to rotate over (2 pairs: four disjoint choices of two
        # experts; 8 pairs: every expert once, the most bytes 8 pairs can read); the all-experts form
        # at 8 and 16 rows with both MXFP4 bodies (see call)
        forms = [("selective", 2, [[0, 1], [2, 3], [4, 5], [6, 7]]), ("selective", 8, [list(range(8))]), ("all", 8, [None]),
                 ("all", 16, [None])]
        for form, P, choices in forms:
            if a.forms and form not in a.forms.split(","):
                continue
            kinds = ("mxfp4", "mxfp4_mfma", "bf16") if form == "all" else ("mxfp4", "bf16")
            eidxs = [None if c is None else torch.tensor(c, dtype=torch.int32, device="cuda") for c in choices]
            if form == "all":
                x = torch.randn(P, K, device="cuda", dtype=torch.bfloat16) if glu else \
                    torch.randn(E, P, K, device="cuda", dtype=torch.bfloat16)
                read = E
            else:
                x = torch.randn(P // 2 if glu else P, K, device="cuda", dtype=torch.bfloat16)
                read = len(set(choices[0]))
            inner = {k: 2 * len(stacks[k]) * len(eidxs) for k in kinds}
            graphs = {k: capture(k, form, x, stacks[k], eidxs, glu, inner[k]) for k in kinds}
            reps = {k: max(3, int(30000.0 / max(time_graph(graphs[k], 3), 1.0))) for k in kinds}   # ~30 ms per sample
            samples = {k: [] for k in kinds}
            for _ in range(a.rounds):
                for k in kinds:   # alternate the variants
                    samples[k].append(time_graph(graphs[k], reps[k]) / inner[k])
            med = {}
            for k in kinds:
                us = med[k] = statistics.median(samples[k])
                nbytes = read * expert_bytes(k, Nw, K)
                emit({"bench": "mx_expert_gemv", "op": op, "form": form, "pairs_or_rows": P, "K": K, "Nw": Nw, "glu": glu,
                      "weights": k, "us": round(us, 2), "us_min": round(min(samples[k]), 2),
                      "us_max": round(max(samples[k]), 2), "weight_bytes": nbytes,
                      "weight_TBps": round(nbytes / us / 1e6, 3), "rounds": a.rounds, "stacks": len(stacks[k])}, sink)
            pairs = [("mxfp4", "bf16")] + ([("mxfp4_mfma", "bf16"), ("mxfp4_mfma", "mxfp4")] if form == "all" else [])
            for n, d in pairs:
                spread = max((max(samples[k]) - min(samples[k])) / med[k] for k in (n, d))
                emit({"bench": "mx_expert_gemv", "op": op, "form": form, "pairs_or_rows": P, "compare": f"{n} / {d}",
                      "time_ratio": round(med[n] / med[d], 3),
                      "byte_ratio": round(expert_bytes(n, Nw, K) / expert_bytes(d, Nw, K), 3),
                      "worst_relative_spread": round(spread, 3),
                      "faster_by_more_than_spread": bool(max(samples[n]) < min(samples[d]))}, sink)
            del graphs
        del stacks
        _SCRATCH.clear()
        torch.cuda.empty_cache()


def random_app(quantized, layers):
    """A Mixtral-8x7B-shaped model of `layers` layers with random weights, filled on the GPU."""
    from transformers import MixtralConfig

    from neuronx_distributed_llama3_2_amd.inference import InferenceConfig, MixtralForCausalLMInference

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=layers, num_attention_heads=32,
                        num_key_value_heads=8, vocab_size=32000, max_position_embeddings=4096, num_local_experts=E,
                        num_experts_per_tok=2)
    kw = dict(quantized=True, quantization_type="mxfp4") if quantized else {}
    icfg = InferenceConfig(batch_size=1, seq_len=512, max_context_length=128, use_hip_graphs=True, decode_graph_steps=8, **kw)
    app = MixtralForCausalLMInference(cfg, icfg, dtype=torch.bfloat16, device=torch.device("cuda"), init_weights=False)
    app.model.to_empty(device=app.device)
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for n, p in app.model.named_parameters():
            if p.dtype == torch.uint8:
                lo, hi = (116, 120) if n.endswith("scale") else (0, 256)   # |w| <= 6 * 2^-8
                p.copy_(torch.randint(lo, hi, p.shape, device="cuda", dtype=torch.uint8, generator=g))
            elif "norm" in n:
                p.fill_(1.0)
            else:
                p.normal_(0.0, 0.02, generator=g)
            p.requires_grad_(False)
    app.model.post_load()
    app.model.setup_kv_cache(app.max_batch, app.cache_len, app.device)
    return app


def bench_e2e(a, sink):
    apps = {"bf16": random_app(False, a.layers), "mxfp4": random_app(True, a.layers)}
    ids = torch.randint(3, 32000, (1, 64))
    short, long_ = 8, 8 + a.tokens

    def ms_per_token(app):
        t = []
        for n in (short, long_):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            app.generate(ids, max_new_tokens=n, eos_token_id=-1)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return (t[1] - t[0]) * 1000.0 / (long_ - short)   # prefill and fixed costs cancel

    for app in apps.values():   # warm-up: graph capture, GEMM tuning
        ms_per_token(app)
    samples = {k: [] for k in apps}
    for _ in range(a.rounds):
        for k, app in apps.items():
            samples[k].append(ms_per_token(app))
    for k in apps:
        emit({"bench": "mixtral_shaped_decode", "layers": a.layers, "batch": 1, "weights": k,
              "ms_per_token": round(statistics.median(samples[k]), 3), "ms_min": round(min(samples[k]), 3),
              "ms_max": round(max(samples[k]), 3), "rounds": a.rounds, "tokens": a.tokens}, sink)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--e2e", action="store_true", help="also time the Mixtral-shaped random model")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--forms", default=None, help="kernel forms to time: selective,all (default both)")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_expert_gemv needs a GPU")
    if a.rounds < 7:
        raise SystemExit("at least 7 rounds")
    sink = open(a.out, "a") if a.out else None
    if not a.skip_kernels:
        bench_kernels(a, sink)
    if a.e2e:
        bench_e2e(a, sink)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
