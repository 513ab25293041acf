"""int8 and MXFP4 weight-only quantization (reference: src/neuronx_distributed/quantization/)."""

from ..ops.gemv import dequantize_mxfp4, mx_expert_linear, mx_experts_linear, mx_linear, quantize_mxfp4  # noqa: F401
from .dequantize import direct_cast_dequantize, scale_dequantize  # noqa: F401
from .observer import PerChannelAbsMaxObserver  # noqa: F401
from .quantization_config import (  # noqa: F401
    QuantizationType,
    QuantizedDtype,
    get_default_custom_qconfig_dict,
    get_default_mxfp4_qconfig_dict,
    get_default_per_channel_custom_qconfig_dict,
)
from .quantization_layers import (  # noqa: F401
    BaseQuantizeParallelLinear,
    MXFP4ColumnParallel,
    MXFP4ExpertFusedColumnParallel,
    MXFP4ExpertFusedRowParallel,
    MXFP4RowParallel,
    QuantizedColumnParallel,
    QuantizedExpertFusedColumnParallel,
    QuantizedExpertFusedRowParallel,
    QuantizedParallelLinearLayerStateDictAdaptor,
    QuantizedRowParallel,
    quantize_symmetric,
)
from .quantization_utils import (  # noqa: F401
    convert_qint8_to_int8_state_dict,
    quantize_pytorch_model_per_channel_symmetric,
    quantize_pytorch_model_per_tensor_symmetric,
)
from .quantization_mappings import get_mxfp4_moe_quant_module_mappings  # noqa: F401
from .quantize import convert  # noqa: F401
