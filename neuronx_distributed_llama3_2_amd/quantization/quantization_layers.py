"""int8 weight-only quantized tensor-parallel linears
(reference: src/neuronx_distributed/quantization/quantization_layers.py:60-890).

Weights are stored as int8 shards with fp32 symmetric scales (per tensor [1], or per output
channel [out, 1] — sharded with the weight when the channel axis is the partition dim).  The matmul:
* token generation (<= 8 rows): the int8 skinny-GEMM kernel (csrc/gemv.hip) reads the int8 weight
  directly and applies the scale in the epilogue — half the HBM bytes of bf16 decode;
* prefill / training-size inputs: one int8 -> bf16 dequantisation kernel, then the tuned GEMM.
Same collectives as the float layers (TP all-reduce / SP reduce-scatter / gather_output).

MXFP4ColumnParallel / MXFP4RowParallel are the same pair with MXFP4 storage (packed 4-bit e2m1 codes and
one E8M0 scale per 32 in-features, both uint8; format in ops/gemv.py, kernels in csrc/gemv_mx.hip).
MXFP4ExpertFusedColumnParallel / MXFP4ExpertFusedRowParallel hold an MoE expert stack the same way,
output-major ([E, out, in/2] codes), for the expert kernels of the same file.
"""

from __future__ import annotations

from typing import Any, Optional

import torch
from torch import nn
from torch.nn.parameter import Parameter

from ..modules.moe.moe_parallel_layers import ExpertFusedColumnParallelLinear, ExpertFusedRowParallelLinear
from ..ops.gemv import MX_BLOCK, dequantize_weight, mx_experts_linear, mx_linear, quantize_mxfp4, skinny_linear
from ..parallel_layers import mappings
from ..parallel_layers import parallel_state as ps
from ..parallel_layers import sp
from ..parallel_layers.layers import ColumnParallelLinear, RowParallelLinear
from ..parallel_layers.utils import divide, set_tensor_model_parallel_attributes
from .quantization_config import (
    BASE_QCONFIG_DICT_TYPE,
    QuantizationType,
    QuantizedDtype,
    get_default_custom_qconfig_dict,
)


def quantize_symmetric(w: torch.Tensor, per_channel_axis: Optional[int] = None):
    """float -> (int8, fp32 scale): scale = absmax / 127 over the tensor or per channel."""
    wf = w.detach().float()
    if per_channel_axis is None:
        scale = (wf.abs().max() / 127.0).clamp(min=1e-12).reshape(1)
        q = torch.round(wf / scale).clamp(-127, 127).to(torch.int8)
        return q, scale
    red = [d for d in range(wf.dim()) if d != per_channel_axis]
    amax = wf.abs().amax(dim=red, keepdim=True)
    scale = (amax / 127.0).clamp(min=1e-12)
    q = torch.round(wf / scale).clamp(-127, 127).to(torch.int8)
    return q, scale


class QuantizedParallelLinearLayerStateDictAdaptor:
    """Accepts float or int8 weights in a state dict; float ones are quantized on load."""

    @staticmethod
    def get_weight_from_state_dict(prefix: str, state_dict: dict) -> torch.Tensor:
        for k in (prefix + "weight", prefix + "_packed_params.weight"):
            if k in state_dict:
                return state_dict[k]
        raise RuntimeError(f"Cannot find weight in state dict for prefix {prefix}")

    @staticmethod
    def get_scale_from_state_dict(prefix: str, state_dict: dict) -> Optional[torch.Tensor]:
        return state_dict.get(prefix + "scale")


class BaseQuantizeParallelLinear(nn.Module):
    def _setup_q(self, q_config: Optional[BASE_QCONFIG_DICT_TYPE], weight_shape, partition_dim: int, stride: int,
                 device, is_expert: bool = False):
        q_config = q_config or get_default_custom_qconfig_dict()
        qt = q_config["quantization_type"]
        self.quantization_type = QuantizationType(qt) if not isinstance(qt, QuantizationType) else qt
        qd = q_config.get("quantized_dtype", QuantizedDtype.INT8)
        self.quantized_dtype = qd.value if isinstance(qd, QuantizedDtype) else qd
        assert self.quantized_dtype == torch.int8, "only int8 weight-only quantization is supported"
        self.per_channel_axis = q_config.get("quantization_per_channel_axis", 0) \
            if self.quantization_type == QuantizationType.PER_CHANNEL_SYMMETRIC else None
        self.weight = Parameter(torch.zeros(weight_shape, dtype=torch.int8, device=device), requires_grad=False)
        set_tensor_model_parallel_attributes(self.weight, True, partition_dim, stride)
        if self.per_channel_axis is None:
            self.scale = Parameter(torch.ones(1, dtype=torch.float32, device=device), requires_grad=False)
        else:
            shape = [1] * len(weight_shape)
            shape[self.per_channel_axis] = weight_shape[self.per_channel_axis]
            self.scale = Parameter(torch.ones(shape, dtype=torch.float32, device=device), requires_grad=False)
            if self.per_channel_axis == partition_dim:
                set_tensor_model_parallel_attributes(self.scale, True, partition_dim, stride)

    def quantize_from(self, w_float: torch.Tensor) -> None:
        """Quantise a float weight of this layer's (local) shape into the int8 weight + scale."""
        q, s = quantize_symmetric(w_float, self.per_channel_axis)
        with torch.no_grad():
            self.weight.copy_(q.to(self.weight.device))
            self.scale.copy_(s.reshape(self.scale.shape).to(self.scale.device))

    def _row_scale(self) -> torch.Tensor:
        """Scale as one fp32 value per output row of the [out, in] weight."""
        if self.per_channel_axis is None:
            return self.scale.reshape(1)
        assert self.per_channel_axis == 0, "per-channel scales must be along the output dim"
        return self.scale.reshape(-1)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        wk = prefix + "weight"
        if wk in state_dict and state_dict[wk].is_floating_point():
            q, s = quantize_symmetric(state_dict[wk], self.per_channel_axis)
            state_dict[wk] = q
            state_dict[prefix + "scale"] = s.reshape(self.scale.shape)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return skinny_linear(x, self.weight, self._row_scale())


class QuantizedColumnParallel(BaseQuantizeParallelLinear):
    def __init__(self, input_size: int, output_size: int, bias: bool = True, gather_output: bool = True,
                 dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None, stride: int = 1,
                 sequence_parallel_enabled: bool = False, keep_master_weight: bool = False,
                 quantization_type: Any = None, quantized_dtype: Any = QuantizedDtype.INT8,
                 quantization_per_channel_axis: Optional[int] = None, q_config: Optional[dict] = None, **kw):
        super().__init__()
        tp = ps.get_tensor_model_parallel_size()
        self.input_size, self.output_size = input_size, output_size
        self.output_size_per_partition = divide(output_size, tp)
        self.gather_output, self.stride, self.dtype = gather_output, stride, dtype
        self.sequence_parallel_enabled = sequence_parallel_enabled and tp > 1
        q_config = q_config or _qc(quantization_type, quantized_dtype, quantization_per_channel_axis)
        self._setup_q(q_config, (self.output_size_per_partition, input_size), 0, stride, device)
        if bias:
            self.bias = Parameter(torch.zeros(self.output_size if gather_output else self.output_size_per_partition,
                                              dtype=dtype, device=device), requires_grad=False)
            if not gather_output:
                set_tensor_model_parallel_attributes(self.bias, True, 0, stride)
        else:
            self.register_parameter("bias", None)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        x = sp.sp_gather(input) if self.sequence_parallel_enabled else input
        out = self._matmul(x.to(self.dtype) if x.dtype != self.dtype else x)
        if self.gather_output and ps.get_tensor_model_parallel_size() > 1:
            out = mappings.gather_from_tensor_model_parallel_region(out)
        return out + self.bias if self.bias is not None else out

    @classmethod
    def from_float(cls, mod: ColumnParallelLinear, q_config: BASE_QCONFIG_DICT_TYPE = None):
        new = cls(mod.input_size, mod.output_size, bias=mod.bias is not None, gather_output=mod.gather_output,
                  dtype=mod.weight.dtype if mod.weight.is_floating_point() else torch.bfloat16,
                  device=mod.weight.device, stride=mod.stride,
                  sequence_parallel_enabled=mod.sequence_parallel_enabled, q_config=q_config)
        if mod.weight.device.type != "meta":
            new.quantize_from(mod.weight)
            if mod.bias is not None:
                with torch.no_grad():
                    new.bias.copy_(mod.bias)
        return new


class QuantizedRowParallel(BaseQuantizeParallelLinear):
    def __init__(self, input_size: int, output_size: int, bias: bool = True, input_is_parallel: bool = False,
                 dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None, stride: int = 1,
                 sequence_parallel_enabled: bool = False, keep_master_weight: bool = False,
                 quantization_type: Any = None, quantized_dtype: Any = QuantizedDtype.INT8,
                 quantization_per_channel_axis: Optional[int] = None, q_config: Optional[dict] = None, **kw):
        super().__init__()
        tp = ps.get_tensor_model_parallel_size()
        self.input_size, self.output_size = input_size, output_size
        self.input_size_per_partition = divide(input_size, tp)
        self.input_is_parallel, self.stride, self.dtype = input_is_parallel, stride, dtype
        self.sequence_parallel_enabled = sequence_parallel_enabled and tp > 1
        q_config = q_config or _qc(quantization_type, quantized_dtype, quantization_per_channel_axis)
        self._setup_q(q_config, (output_size, self.input_size_per_partition), 1, stride, device)
        if bias:
            self.bias = Parameter(torch.zeros(output_size, dtype=dtype, device=device), requires_grad=False)
        else:
            self.register_parameter("bias", None)

    def forward(self, input_: torch.Tensor) -> torch.Tensor:
        x = input_ if self.input_is_parallel else mappings.scatter_to_tensor_model_parallel_region(input_)
        out = self._matmul(x.to(self.dtype) if x.dtype != self.dtype else x)
        if self.sequence_parallel_enabled:
            out = sp.sp_reduce_scatter(out)
        elif ps.get_tensor_model_parallel_size() > 1:
            out = mappings.reduce_from_tensor_model_parallel_region(out)
        return out + self.bias if self.bias is not None else out

    @classmethod
    def from_float(cls, mod: RowParallelLinear, q_config: BASE_QCONFIG_DICT_TYPE = None):
        new = cls(mod.input_size, mod.output_size, bias=mod.bias is not None, input_is_parallel=mod.input_is_parallel,
                  dtype=mod.weight.dtype if mod.weight.is_floating_point() else torch.bfloat16,
                  device=mod.weight.device, stride=mod.stride,
                  sequence_parallel_enabled=mod.sequence_parallel_enabled, q_config=q_config)
        if mod.weight.device.type != "meta":
            new.quantize_from(mod.weight)
            if mod.bias is not None:
                with torch.no_grad():
                    new.bias.copy_(mod.bias)
        return new


class _QuantizedExpertFused(nn.Module):
    """int8 3-D expert weights [E, in, out] (+ scale per expert [E, 1, 1] or per out channel [E, 1, out])."""

    def _init_q(self, mod, q_config):
        q_config = q_config or get_default_custom_qconfig_dict()
        qt = q_config["quantization_type"]
        self.quantization_type = QuantizationType(qt) if not isinstance(qt, QuantizationType) else qt
        w = mod.weight
        self.num_experts = mod.num_experts
        self.weight = Parameter(torch.zeros(w.shape, dtype=torch.int8, device=w.device if w.device.type != "meta" else None),
                                requires_grad=False)
        for a in ("tensor_model_parallel", "partition_dim", "partition_stride", "expert_model_parallel"):
            if hasattr(w, a):
                setattr(self.weight, a, getattr(w, a))
        per_ch = self.quantization_type == QuantizationType.PER_CHANNEL_SYMMETRIC
        sshape = (w.shape[0], 1, w.shape[2]) if per_ch else (w.shape[0], 1, 1)
        self.scale = Parameter(torch.ones(sshape, dtype=torch.float32, device=self.weight.device), requires_grad=False)
        if w.device.type != "meta":
            wf = w.detach().float()
            amax = wf.abs().amax(dim=1, keepdim=True) if per_ch else wf.abs().amax(dim=(1, 2), keepdim=True)
            s = (amax / 127.0).clamp(min=1e-12)
            with torch.no_grad():
                self.weight.copy_(torch.round(wf / s).clamp(-127, 127).to(torch.int8))
                self.scale.copy_(s)
        self.dtype = w.dtype if w.is_floating_point() else torch.bfloat16

    def _w(self, expert_indices=None):
        w, s = (self.weight, self.scale) if expert_indices is None else (self.weight[expert_indices], self.scale[expert_indices])
        return (w.float() * s).to(self.dtype)


class QuantizedExpertFusedColumnParallel(_QuantizedExpertFused):
    def __init__(self, mod: ExpertFusedColumnParallelLinear, q_config=None):
        super().__init__()
        self._init_q(mod, q_config)
        self.async_tensor_model_parallel_allreduce = False

    def forward(self, input_, expert_indices=None):
        w = self._w(expert_indices)
        E = w.shape[0]
        x = input_.expand((E,) + tuple(input_.shape[1:])) if input_.shape[0] == 1 and E > 1 else input_
        return torch.bmm(x.reshape(E, -1, x.shape[-1]), w).view(tuple(x.shape[:-1]) + (w.shape[-1],))

    @classmethod
    def from_float(cls, mod, q_config=None):
        return cls(mod, q_config)


class QuantizedExpertFusedRowParallel(QuantizedExpertFusedColumnParallel):
    def __init__(self, mod: ExpertFusedRowParallelLinear, q_config=None):
        super().__init__(mod, q_config)
        self.reduce_output = getattr(mod, "reduce_output", True)

    def forward(self, input_, expert_indices=None):
        out = super().forward(input_, expert_indices)
        if self.reduce_output and ps.get_tensor_model_parallel_size() > 1:
            out = mappings.reduce_from_tensor_model_parallel_region(out)
        return out


class _MXFP4ParallelLinear(nn.Module):
    """MXFP4 weight-only storage of a tensor-parallel linear (format: ops/gemv.py): `weight` is the
    packed uint8 [out, in/2] parameter, `scale` the E8M0 uint8 [out, in/32] one; both are sharded
    along the layer's partition dim (blocks run along `in`, so a row-parallel shard needs its local
    `in` to be a multiple of 32).  Decode-sized inputs read the 4-bit weights directly (mx_gemv);
    larger ones dequantise to bf16 and take the tuned GEMM."""

    def _setup_mx(self, out_features: int, in_features: int, partition_dim: int, stride: int, device) -> None:
        if in_features % MX_BLOCK != 0:
            raise ValueError(f"MXFP4 needs the local in-features ({in_features}) to be a multiple of {MX_BLOCK}")
        self.quantization_type = QuantizationType.MX_BLOCK
        self.quantized_dtype = QuantizedDtype.MXFP4.value
        self.weight = Parameter(torch.zeros((out_features, in_features // 2), dtype=torch.uint8, device=device),
                                requires_grad=False)
        # e = 127 (scale 1) with zero codes: an unloaded layer dequantises to zeros
        self.scale = Parameter(torch.full((out_features, in_features // MX_BLOCK), 127, dtype=torch.uint8, device=device),
                               requires_grad=False)
        set_tensor_model_parallel_attributes(self.weight, True, partition_dim, stride)
        set_tensor_model_parallel_attributes(self.scale, True, partition_dim, stride)

    def quantize_from(self, w_float: torch.Tensor) -> None:
        """Quantise a float weight of this layer's (local) [out, in] shape into weight + scale."""
        q, s = quantize_mxfp4(w_float)
        with torch.no_grad():
            self.weight.copy_(q.to(self.weight.device))
            self.scale.copy_(s.to(self.scale.device))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        wk = prefix + "weight"
        if wk in state_dict and state_dict[wk].is_floating_point():
            state_dict[wk], state_dict[prefix + "scale"] = quantize_mxfp4(state_dict[wk])
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return mx_linear(x, self.weight, self.scale)

    def _copy_bias(self, mod) -> None:
        if mod.bias is not None:
            with torch.no_grad():
                self.bias.copy_(mod.bias)


class MXFP4ColumnParallel(_MXFP4ParallelLinear):
    def __init__(self, input_size: int, output_size: int, bias: bool = True, gather_output: bool = True,
                 dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None, stride: int = 1,
                 sequence_parallel_enabled: bool = False, keep_master_weight: bool = False,
                 quantization_type: Any = None, quantized_dtype: Any = QuantizedDtype.MXFP4,
                 quantization_per_channel_axis: Optional[int] = None, q_config: Optional[dict] = None, **kw):
        super().__init__()
        tp = ps.get_tensor_model_parallel_size()
        self.input_size, self.output_size = input_size, output_size
        self.output_size_per_partition = divide(output_size, tp)
        self.gather_output, self.stride, self.dtype = gather_output, stride, dtype
        self.sequence_parallel_enabled = sequence_parallel_enabled and tp > 1
        self._setup_mx(self.output_size_per_partition, input_size, 0, stride, device)
        if bias:
            self.bias = Parameter(torch.zeros(self.output_size if gather_output else self.output_size_per_partition,
                                              dtype=dtype, device=device), requires_grad=False)
            if not gather_output:
                set_tensor_model_parallel_attributes(self.bias, True, 0, stride)
        else:
            self.register_parameter("bias", None)

    forward = QuantizedColumnParallel.forward

    @classmethod
    def from_float(cls, mod: ColumnParallelLinear, q_config: BASE_QCONFIG_DICT_TYPE = None):
        new = cls(mod.input_size, mod.output_size, bias=mod.bias is not None, gather_output=mod.gather_output,
                  dtype=mod.weight.dtype if mod.weight.is_floating_point() else torch.bfloat16,
                  device=mod.weight.device, stride=mod.stride,
                  sequence_parallel_enabled=mod.sequence_parallel_enabled, q_config=q_config)
        if mod.weight.device.type != "meta":
            new.quantize_from(mod.weight)
            new._copy_bias(mod)
        return new


class MXFP4RowParallel(_MXFP4ParallelLinear):
    def __init__(self, input_size: int, output_size: int, bias: bool = True, input_is_parallel: bool = False,
                 dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None, stride: int = 1,
                 sequence_parallel_enabled: bool = False, keep_master_weight: bool = False,
                 quantization_type: Any = None, quantized_dtype: Any = QuantizedDtype.MXFP4,
                 quantization_per_channel_axis: Optional[int] = None, q_config: Optional[dict] = None, **kw):
        super().__init__()
        tp = ps.get_tensor_model_parallel_size()
        self.input_size, self.output_size = input_size, output_size
        self.input_size_per_partition = divide(input_size, tp)
        self.input_is_parallel, self.stride, self.dtype = input_is_parallel, stride, dtype
        self.sequence_parallel_enabled = sequence_parallel_enabled and tp > 1
        self._setup_mx(output_size, self.input_size_per_partition, 1, stride, device)
        if bias:
            self.bias = Parameter(torch.zeros(output_size, dtype=dtype, device=device), requires_grad=False)
        else:
            self.register_parameter("bias", None)

    forward = QuantizedRowParallel.forward

    @classmethod
    def from_float(cls, mod: RowParallelLinear, q_config: BASE_QCONFIG_DICT_TYPE = None):
        new = cls(mod.input_size, mod.output_size, bias=mod.bias is not None, input_is_parallel=mod.input_is_parallel,
                  dtype=mod.weight.dtype if mod.weight.is_floating_point() else torch.bfloat16,
                  device=mod.weight.device, stride=mod.stride,
                  sequence_parallel_enabled=mod.sequence_parallel_enabled, q_config=q_config)
        if mod.weight.device.type != "meta":
            new.quantize_from(mod.weight)
            new._copy_bias(mod)
        return new


class _MXFP4ExpertFused(nn.Module):
    """MXFP4 storage of an expert-fused linear (logical weight [E, in, out]): `weight` is the packed
    uint8 [E, out_local, in_local/2] parameter, `scale` the E8M0 uint8 [E, out_local, in_local/32] one
    -- output-major, which is what the expert kernels of csrc/gemv_mx.hip read.  Both keep the float
    layer's TP sharding (column: out with the layer's stride, i.e. 2 for [gate; up]; row: in) on
    the transposed axes, so a full float weight has to be output-major when it is sliced by these
    parameters' partition dims (inference/moe.py `_load_full`)."""

    def _setup_mx(self, num_experts: int, in_local: int, out_local: int, partition_dim: int, stride: int, dtype,
                  device) -> None:
        if in_local % MX_BLOCK != 0:
            raise ValueError(f"MXFP4 needs the local in-features ({in_local}) to be a multiple of {MX_BLOCK}")
        ep = ps.get_expert_model_parallel_size() if ps.model_parallel_is_initialized() else 1
        self.num_experts = num_experts
        self._n_local_experts = divide(num_experts, ep)
        self.quantization_type = QuantizationType.MX_BLOCK
        self.quantized_dtype = QuantizedDtype.MXFP4.value
        self.dtype = dtype
        E = self._n_local_experts
        self.weight = Parameter(torch.zeros((E, out_local, in_local // 2), dtype=torch.uint8, device=device),
                                requires_grad=False)
        # e = 127 (scale 1) with zero codes: an unloaded layer dequantises to zeros
        self.scale = Parameter(torch.full((E, out_local, in_local // MX_BLOCK), 127, dtype=torch.uint8, device=device),
                               requires_grad=False)
        for t in (self.weight, self.scale):
            set_tensor_model_parallel_attributes(t, True, partition_dim, stride)
            setattr(t, "expert_model_parallel", True)

    def quantize_from(self, w_float: torch.Tensor) -> None:
        """Quantise a float weight of this layer's logical (local) [E, in, out] shape."""
        q, s = quantize_mxfp4(w_float.detach().transpose(1, 2).contiguous())
        with torch.no_grad():
            self.weight.copy_(q.to(self.weight.device))
            self.scale.copy_(s.to(self.scale.device))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        wk = prefix + "weight"
        if wk in state_dict and state_dict[wk].is_floating_point():
            w = state_dict[wk]
            E, o, i2 = self.weight.shape
            if tuple(w.shape) != (E, i2 * 2, o):
                error_msgs.append(f"{wk}: a float expert weight must be [E, in, out] = {(E, i2 * 2, o)}, got {tuple(w.shape)}")
                return
            state_dict[wk], state_dict[prefix + "scale"] = quantize_mxfp4(w.transpose(1, 2).contiguous())
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def _matmul(self, input_: torch.Tensor, expert_indices=None) -> torch.Tensor:
        w, s = (self.weight, self.scale) if expert_indices is None else (self.weight[expert_indices], self.scale[expert_indices])
        E = w.shape[0]
        x = input_.to(self.dtype) if input_.dtype != self.dtype else input_
        if x.shape[0] not in (1, E):
            raise RuntimeError(f"input/weight expert count mismatch: {tuple(x.shape)} vs {E} experts")
        x3 = x.reshape(x.shape[0], -1, x.shape[-1])
        out = mx_experts_linear(x3[0] if x3.shape[0] == 1 and E > 1 else x3, w, s)
        return out.view((E,) + tuple(x.shape[1:-1]) + (w.shape[1],))


class MXFP4ExpertFusedColumnParallel(_MXFP4ExpertFused):
    """[E, ..., H] -> [E, ..., out/tp] on MXFP4 expert weights."""

    def __init__(self, num_experts: int, input_size: int, output_size: int, dtype: torch.dtype = torch.bfloat16,
                 device: Optional[torch.device] = None, stride: int = 1, **kw):
        super().__init__()
        self.input_size, self.output_size, self.stride = input_size, output_size, stride
        self._setup_mx(num_experts, input_size, divide(output_size, ps.get_tensor_model_parallel_size()), 1, stride, dtype,
                       device)

    def forward(self, input_: torch.Tensor, expert_indices: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._matmul(input_, expert_indices)

    @classmethod
    def from_float(cls, mod: ExpertFusedColumnParallelLinear, q_config: BASE_QCONFIG_DICT_TYPE = None):
        new = cls(mod.num_experts, mod.input_size, mod.output_size,
                  dtype=mod.weight.dtype if mod.weight.is_floating_point() else torch.bfloat16,
                  device=mod.weight.device, stride=mod.stride)
        if mod.weight.device.type != "meta":
            new.quantize_from(mod.weight)
        return new


class MXFP4ExpertFusedRowParallel(_MXFP4ExpertFused):
    """[E, ..., in/tp] -> [E, ..., H] partial sums on MXFP4 expert weights (reduced over TP here when
    `reduce_output` is set, as the float layer does)."""

    def __init__(self, num_experts: int, input_size: int, output_size: int, reduce_output: bool = True,
                 dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None, stride: int = 1, **kw):
        super().__init__()
        self.input_size, self.output_size, self.stride = input_size, output_size, stride
        self.reduce_output = reduce_output
        self._setup_mx(num_experts, divide(input_size, ps.get_tensor_model_parallel_size()), output_size, 2, stride, dtype,
                       device)

    def forward(self, input_: torch.Tensor, expert_indices: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = self._matmul(input_, expert_indices)
        if self.reduce_output and ps.get_tensor_model_parallel_size() > 1:
            out = mappings.reduce_from_tensor_model_parallel_region(out)
        return out

    @classmethod
    def from_float(cls, mod: ExpertFusedRowParallelLinear, q_config: BASE_QCONFIG_DICT_TYPE = None):
        new = cls(mod.num_experts, mod.input_size, mod.output_size, reduce_output=getattr(mod, "reduce_output", True),
                  dtype=mod.weight.dtype if mod.weight.is_floating_point() else torch.bfloat16,
                  device=mod.weight.device, stride=mod.stride)
        if mod.weight.device.type != "meta":
            new.quantize_from(mod.weight)
        return new


class MXFP4ExpertFusedUnsupported:
    """Stub of the default MXFP4 mapping: convert() on a model with MoE experts refuses unless the
    caller passes the mapping with the expert layers (get_mxfp4_moe_quant_module_mappings)."""

    @classmethod
    def from_float(cls, mod, q_config=None):
        raise NotImplementedError("MXFP4 weight-only quantization covers the dense linears only, not MoE experts")


def _qc(quantization_type, quantized_dtype, axis):
    if quantization_type is None:
        return get_default_custom_qconfig_dict()
    d = {"quantization_type": QuantizationType(quantization_type) if not isinstance(quantization_type, QuantizationType)
         else quantization_type, "quantized_dtype": quantized_dtype}
    if d["quantization_type"] == QuantizationType.PER_CHANNEL_SYMMETRIC:
        d["quantization_per_channel_axis"] = 0 if axis is None else axis
    return d
