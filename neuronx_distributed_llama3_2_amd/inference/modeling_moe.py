"""Sparse-MoE causal LM inference (Mixtral, DBRX) on the shared decoder inference forward
(reference: examples/inference/mixtral/neuron_modeling_mixtral.py, examples/inference/dbrx/
neuron_modeling_dbrx.py — both built on the MoE module with RouterTopK + ExpertMLPs).

The module IS the training `MixtralForCausalLM` (attention identical to Llama, MoE block from
modules/moe), so training checkpoints and converted HF weights load directly.  The MoE block picks
its dispatch per call, all with experts TP-sharded on the intermediate dim (one all-reduce after
the down projection, like a dense MLP):

* few (token, expert) pairs (T * top_k <= E: token generation) — *selective loading*: the
  expert-mode skinny GEMM (csrc/gemv.hip) reads only the chosen experts' weights, SwiGLU fused in
  its epilogue; static shapes, no host sync, captured in the decode hipGraph;
* small T under graph capture (batched decode / speculation) — every token through every expert
  as two batched GEMMs (each expert's weights read once, static shapes);
* prefill — tokens sorted by expert on the device, each expert multiplies only its own rows (the
  training path's grouped GEMM kernels, top_k / E of the dense work, no host sync).

To feed the skinny-GEMM kernel, the expert weights are stored output-major ([E, out, in] in
memory) while keeping their logical [E, in, out] parameter shapes (`post_load`).

With MXFP4 experts (quantization_type="mxfp4": packed codes [E, out, in/2] + block scales, output-major
as stored) the first two regimes read the 4-bit codes directly -- the selective and the all-experts
(at most 8 tokens) kernels of csrc/gemv_mx.hip -- and anything larger dequantises the layer's
experts into one bf16 scratch pair shared by all layers (E * 3 * H * I/tp * 2 bytes, allocated with
the KV cache, before any graph capture) and runs the float code on it.
DBRX differences handled here: LayerNorm without bias instead of RMSNorm (`norm_type`), QKV
clamped to +-clip_qkv, optional top-k renormalisation (models/mixtral/convert.py translates its
config and weights).
"""

from __future__ import annotations

import copy

import torch
import torch.nn.functional as F

from ..models.mixtral.modeling_mixtral import MixtralForCausalLM
from ..ops._ext import ext, use_native
from ..ops.gemv import dequantize_mxfp4_into, expert_linear, mx_expert_linear, mx_experts_linear
from ..ops.grouped_gemm import moe_dispatch, moe_permutation, moe_unpermute_combine
from ..ops import swiglu
from .model_base import DecoderInferenceMixin

# below this many tokens a capture-safe dense all-experts dispatch is used outside selective loading
_DENSE_MAX_TOKENS = 64
# MXFP4 experts: the all-experts kernel carries at most this many rows per weight load (csrc/gemv_mx.hip)
_MX_ALL_EXPERTS_MAX_TOKENS = 8


class MoEInferenceModel(DecoderInferenceMixin, MixtralForCausalLM):
    def __init__(self, config, dtype=torch.bfloat16, device=None):
        cfg = copy.copy(config)
        cfg.sequence_parallel_enabled = False
        cfg.capacity_factor = None
        MixtralForCausalLM.__init__(self, cfg, dtype=dtype, device=device)
        self._init_inference(config)
        self.norm_type = getattr(config, "norm_type", "rmsnorm")
        self.clip_qkv = getattr(config, "clip_qkv", None)
        self.top_k = int(config.num_experts_per_tok)
        self.num_experts = int(config.num_local_experts)
        self.normalize_top_k = bool(getattr(config, "normalize_top_k_affinities", self.top_k > 1))
        if next(self.parameters()).device.type != "meta":
            self.post_load()

    # ------------------------------------------------------------------ weights
    def _expert_weights(self, layer):
        """Float experts: the logical weights [E, H, 2I/tp], [E, I/tp, H].  MXFP4 experts
        (quantization_layers.MXFP4ExpertFused*): the (packed, scale) pairs of gate_up and down,
        stored output-major ([E, 2I/tp, H/2] and [E, H, I/tp/2] codes)."""
        mo = layer.block_sparse_moe.expert_mlps.mlp_op
        if mo.gate_up_proj.weight.dtype == torch.uint8:
            return (mo.gate_up_proj.weight, mo.gate_up_proj.scale), (mo.down_proj.weight, mo.down_proj.scale)
        return mo.gate_up_proj.weight, mo.down_proj.weight

    def _experts_packed(self) -> bool:
        return self.model.layers[0].block_sparse_moe.expert_mlps.mlp_op.gate_up_proj.weight.dtype == torch.uint8

    @torch.no_grad()
    def post_load(self) -> None:
        """Re-lay the float expert weights output-major in memory (logical shapes unchanged); MXFP4
        experts are stored that way already."""
        if self._experts_packed():
            return
        for layer in self.model.layers:
            for w in self._expert_weights(layer):
                if w.stride(-1) == 1 and w.shape[-1] > 1:
                    w.data = w.data.transpose(1, 2).contiguous().transpose(1, 2)

    def setup_kv_cache(self, max_batch: int, max_len: int, device=None) -> torch.Tensor:
        """With MXFP4 experts this is also where the prefill scratch is allocated: one output-major
        pair ([E, 2I/tp, H], [E, H, I/tp], activation dtype: E * 3 * H * I/tp elements) shared by
        all layers, which `_ffn` dequantises a layer's experts into.  It exists before any graph
        is captured, so a captured prefill or large-batch step allocates nothing."""
        kv = DecoderInferenceMixin.setup_kv_cache(self, max_batch, max_len, device)
        if self._experts_packed():
            (p_gu, _), (p_d, _) = self._expert_weights(self.model.layers[0])
            shapes = [tuple(p.shape[:2]) + (p.shape[2] * 2,) for p in (p_gu, p_d)]
            old = getattr(self, "_expert_scratch", None)
            if old is None or old[0].device != kv.device or [tuple(t.shape) for t in old] != shapes:
                dtype = self.model.embed_tokens.weight.dtype
                self._expert_scratch = tuple(torch.empty(s, dtype=dtype, device=kv.device) for s in shapes)
        return kv

    # ------------------------------------------------------------------ block pieces
    def _qkv_hook(self, qkv: torch.Tensor) -> torch.Tensor:
        if self.clip_qkv is not None:
            qkv.clamp_(-float(self.clip_qkv), float(self.clip_qkv))
        return qkv

    def _norm(self, x, w, residual):
        if self.norm_type == "rmsnorm":
            return DecoderInferenceMixin._norm(self, x, w, residual)
        r = x if residual is None else x + residual
        y = F.layer_norm(r.float(), (r.shape[-1],), w.float(), None, self.eps).to(r.dtype)
        return y, r

    def _route(self, layer, x: torch.Tensor):
        router = layer.block_sparse_moe.router.linear_router
        logits = F.linear(x, router.weight.to(x.dtype))
        probs = torch.softmax(logits.float(), dim=-1)
        top_w, top_i = torch.topk(probs, self.top_k, dim=-1)
        if self.normalize_top_k:
            top_w = top_w / top_w.sum(-1, keepdim=True)
        return top_w, top_i

    def _ffn(self, layer, h: torch.Tensor) -> torch.Tensor:
        shape = h.shape
        x = h.reshape(-1, shape[-1])
        top_w, top_i = self._route(layer, x)
        out = self._experts(x, top_w, top_i, *self._expert_weights(layer))
        return self._all_reduce(out).view(shape)

    def _experts(self, x, top_w, top_i, w_gu, w_d):
        """The dispatch of the module docstring on routed tokens x [n, H]; TP-partial result [n, H]."""
        n, k, E = x.shape[0], self.top_k, self.num_experts
        if isinstance(w_gu, tuple):   # MXFP4 experts: (packed, scale) pairs
            if n * k <= E:
                return self._selective_mx(x, top_w, top_i, w_gu, w_d)
            if n <= _MX_ALL_EXPERTS_MAX_TOKENS:
                return self._all_experts_mx(x, top_w, top_i, w_gu, w_d)
            w_gu, w_d = self._dequantized_experts(w_gu, w_d)
        if n * k <= E:
            return self._selective(x, top_w, top_i, w_gu, w_d)
        if n <= _DENSE_MAX_TOKENS or (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            return self._all_experts(x, top_w, top_i, w_gu, w_d)
        return self._grouped(x, top_w, top_i, w_gu, w_d)

    def _selective(self, x, top_w, top_i, w_gu, w_d):
        n, k = top_i.shape
        eidx = top_i.reshape(-1).to(torch.int32)
        a = expert_linear(x, w_gu.transpose(1, 2), eidx, xdiv=k, glu=True)   # [n*k, I/tp]
        y = expert_linear(a, w_d.transpose(1, 2), eidx, xdiv=1)             # [n*k, H] partial over TP
        return (y.view(n, k, -1).float() * top_w.unsqueeze(-1)).sum(1).to(x.dtype)

    def _selective_mx(self, x, top_w, top_i, gu, d):
        """`_selective` on the 4-bit codes: only the chosen experts' codes and scales are read."""
        n, k = top_i.shape
        eidx = top_i.reshape(-1).to(torch.int32)
        a = mx_expert_linear(x, gu[0], gu[1], eidx, xdiv=k, glu=True)       # [n*k, I/tp]
        y = mx_expert_linear(a, d[0], d[1], eidx, xdiv=1)                   # [n*k, H] partial over TP
        return (y.view(n, k, -1).float() * top_w.unsqueeze(-1)).sum(1).to(x.dtype)

    def _all_experts(self, x, top_w, top_i, w_gu, w_d):
        E = self.num_experts
        gu = torch.matmul(x.unsqueeze(0), w_gu)                              # [E, n, 2I/tp]
        y = torch.matmul(swiglu(gu), w_d)                                    # [E, n, H]
        dense_w = torch.zeros(x.shape[0], E, dtype=torch.float32, device=x.device).scatter_(1, top_i, top_w)
        return torch.einsum("enh,ne->nh", y.float(), dense_w).to(x.dtype)

    def _all_experts_mx(self, x, top_w, top_i, gu, d):
        """`_all_experts` for at most 8 tokens on the 4-bit codes, each expert's bytes read once."""
        E = self.num_experts
        a = mx_experts_linear(x, gu[0], gu[1], glu=True)                     # [E, n, I/tp]
        y = mx_experts_linear(a, d[0], d[1])                                 # [E, n, H]
        dense_w = torch.zeros(x.shape[0], E, dtype=torch.float32, device=x.device).scatter_(1, top_i, top_w)
        return torch.einsum("enh,ne->nh", y.float(), dense_w).to(x.dtype)

    def _dequantized_experts(self, gu, d):
        """Prefill-sized inputs: this layer's experts dequantised into the scratch pair shared by all
        layers (`setup_kv_cache`), returned in the logical [E, in, out] shapes over output-major
        storage -- what `post_load` gives float experts, so `_all_experts` / `_grouped` run unchanged."""
        s_gu, s_d = self._expert_scratch
        dequantize_mxfp4_into(gu[0], gu[1], s_gu)
        dequantize_mxfp4_into(d[0], d[1], s_d)
        return s_gu.transpose(1, 2), s_d.transpose(1, 2)

    def _grouped(self, x, top_w, top_i, w_gu, w_d):
        """Prefill: (token, choice) slots sorted by expert on the device, each expert multiplying only
        its own rows.  GPU bf16: the training path's sync-free kernels -- device-side permutation,
        dispatch gather, the grouped GEMMs (csrc/grouped_rowgemm.hip / grouped_gemm.hip) with the
        expert weights read output-major in place, SwiGLU, and the fused un-permute + affinity
        combine (csrc/moe_combine.hip); no host read of the group sizes, so a prefill graph can
        capture it.  Otherwise (CPU, fp32): per-expert matmuls over host-read group sizes.
        Reference: src/neuronx_distributed/modules/moe/expert_mlps.py:169-265."""
        if x.is_cuda and x.dtype == torch.bfloat16 and use_native(x) and x.shape[1] % 8 == 0 \
                and w_gu.shape[2] % 8 == 0 and top_i.shape[1] <= 8:
            return self._grouped_device(x, top_w, top_i, w_gu, w_d)
        n, k = top_i.shape
        flat = top_i.reshape(-1)
        order = torch.argsort(flat, stable=True)
        tok = order // k
        counts = torch.bincount(flat, minlength=self.num_experts).tolist()   # one host sync (prefill)
        xs = x.index_select(0, tok)
        ys = torch.empty((n * k, x.shape[1]), dtype=x.dtype, device=x.device)
        start = 0
        for e, c in enumerate(counts):
            if c:
                seg = xs[start:start + c]
                ys[start:start + c] = torch.matmul(swiglu(torch.matmul(seg, w_gu[e])), w_d[e])
                start += c
        ys = ys.float() * top_w.reshape(-1)[order].unsqueeze(1)
        out = torch.zeros((n, x.shape[1]), dtype=torch.float32, device=x.device)
        out.index_add_(0, tok, ys)
        return out.to(x.dtype)

    def _grouped_device(self, x, top_w, top_i, w_gu, w_d):
        n, k = top_i.shape
        order, inverse, offs = moe_permutation(top_i, self.num_experts)
        xs = moe_dispatch(x, order, inverse, k)                       # [n*k, H], expert-sorted rows
        gu = _grouped_mm(xs, w_gu, offs)                              # [n*k, 2I/tp]
        ys = _grouped_mm(swiglu(gu), w_d, offs)                       # [n*k, H] partial over TP
        return moe_unpermute_combine(ys, inverse, top_w.float())      # [n, H]


def _grouped_mm(x: torch.Tensor, w: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """y[rows of e] = x[rows of e] @ w[e] for logical w [E, K, N], read in its stored layout: the
    grouped kernel's forward mode for [E, K, N]-contiguous weights, its input-gradient mode (x @ W^T)
    for the output-major [E, N, K] storage `post_load` gives the expert weights."""
    y = torch.empty(x.shape[0], w.shape[2], dtype=x.dtype, device=x.device)
    if w.is_contiguous():
        ext().grouped_gemm(0, x.contiguous(), w, offs, y, False)
    else:
        ext().grouped_gemm(1, x.contiguous(), w.transpose(1, 2).contiguous(), offs, y, False)
    return y
