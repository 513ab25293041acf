"""Float -> quantized module mapping (reference: src/neuronx_distributed/quantization/quantization_mappings.py:11-16)."""

from typing import Any, Callable, Dict

from ..modules.moe import moe_parallel_layers
from ..parallel_layers import layers as parallel_layers
from . import quantization_layers as q_layers

DEFAULT_QUANT_MODULE_MAPPINGS: Dict[Callable, Any] = {
    parallel_layers.ColumnParallelLinear: q_layers.QuantizedColumnParallel,
    parallel_layers.RowParallelLinear: q_layers.QuantizedRowParallel,
    moe_parallel_layers.ExpertFusedColumnParallelLinear: q_layers.QuantizedExpertFusedColumnParallel,
    moe_parallel_layers.ExpertFusedRowParallelLinear: q_layers.QuantizedExpertFusedRowParallel,
}


MXFP4_QUANT_MODULE_MAPPINGS: Dict[Callable, Any] = {
    parallel_layers.ColumnParallelLinear: q_layers.MXFP4ColumnParallel,
    parallel_layers.RowParallelLinear: q_layers.MXFP4RowParallel,
    moe_parallel_layers.ExpertFusedColumnParallelLinear: q_layers.MXFP4ExpertFusedUnsupported,
    moe_parallel_layers.ExpertFusedRowParallelLinear: q_layers.MXFP4ExpertFusedUnsupported,
}


# The MoE inference applications pass this one to convert(..., mapping=): the default MXFP4 mapping
# above keeps refusing expert-fused layers.
MXFP4_MOE_QUANT_MODULE_MAPPINGS: Dict[Callable, Any] = {
    parallel_layers.ColumnParallelLinear: q_layers.MXFP4ColumnParallel,
    parallel_layers.RowParallelLinear: q_layers.MXFP4RowParallel,
    moe_parallel_layers.ExpertFusedColumnParallelLinear: q_layers.MXFP4ExpertFusedColumnParallel,
    moe_parallel_layers.ExpertFusedRowParallelLinear: q_layers.MXFP4ExpertFusedRowParallel,
}


def get_mxfp4_moe_quant_module_mappings() -> Dict[Callable, Any]:
    return MXFP4_MOE_QUANT_MODULE_MAPPINGS


def get_default_quant_module_mappings() -> Dict[Callable, Any]:
    return DEFAULT_QUANT_MODULE_MAPPINGS


def get_mxfp4_quant_module_mappings() -> Dict[Callable, Any]:
    return MXFP4_QUANT_MODULE_MAPPINGS
