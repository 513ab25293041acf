"""Hot ops of the framework: each runs a hand-written CDNA4 HIP kernel on the GPU and a plain
PyTorch fp32 reference on the CPU (see _ext.use_native)."""

from ._ext import ext, ext_available, use_native  # noqa: F401
from .activations import swiglu, swiglu_reference  # noqa: F401
from .cross_entropy import parallel_cross_entropy_reference, vocab_parallel_cross_entropy  # noqa: F401
from .decode import (argmax_rows, decode_attention, decode_window, dequantize_mxfp8, greedy_advance_,  # noqa: F401
                     kv_cache_write, quantize_mxfp8, topk_sample)
from .embedding import vocab_parallel_embedding  # noqa: F401
from .grouped_gemm import (grouped_linear, grouped_linear_reference, moe_dispatch, moe_permutation,  # noqa: F401
                           moe_unpermute_combine)
from .attention_ranges import (KeyRanges, intersect_ranges, positions_from_ranges, ranges_from_cu_seqlens,  # noqa: F401
                               ranges_from_document_starts, ranges_from_eos, ranges_from_lengths,
                               ranges_sliding_window, validate)
from .flash_attn import attention_reference, flash_attn_func, flash_attn_fwd_lse, rope_attention  # noqa: F401
from .norm import rms_norm, rms_norm_reference  # noqa: F401
from .optim import (adamw_flat_, clip_coefficient, flat_absmax, flat_sumsq, scale_flat_, sr_seed_for_step,  # noqa: F401
                    stochastic_round_bf16)
from .rope import apply_rotary_reference, inv_freq_from_config, llama3_inv_freq, rope_inplace_, rope_tables  # noqa: F401
