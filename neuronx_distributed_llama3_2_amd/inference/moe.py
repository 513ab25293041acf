"""Mixtral / DBRX inference applications and runners (reference: examples/inference/mixtral/
{neuron_modeling_mixtral.py:128-340, mixtral_runner.py}, examples/inference/dbrx/{neuron_modeling_dbrx.py,
dbrx_runner.py}, run_mixtral.py, run_dbrx.py).

Same lifecycle as the Llama application (from_pretrained -> compile -> load -> generate, hipGraph
token generation, on-device sampling, speculation), with the MoE device module
(inference/modeling_moe.py).  `capacity_factor` / `glu_mlp` are accepted for parity with the
reference's NeuronMixtralConfig / NeuronDbrxConfig: inference is always dropless (the reference's
capacity_factor=None default) and the experts are GLU.
"""

from __future__ import annotations

import json
import os

import torch

from ..models.mixtral.convert import dbrx_hf_to_nxd, dbrx_to_mixtral_config, mixtral_hf_to_nxd
from ..parallel_layers import parallel_state as ps
from ..parallel_layers.sharding import shard_state_dict
from .config import InferenceConfig
from .generation import LlamaForCausalLMInference
from .modeling_moe import MoEInferenceModel
from .runner import InferenceRunner


def moe_config_from_dir(path: str):
    """config.json of a Mixtral or DBRX directory (or of a compiled MoE model) -> MixtralConfig."""
    from transformers import MixtralConfig

    with open(os.path.join(path, "config.json")) as f:
        d = json.load(f)
    d = {k: v for k, v in d.items() if k not in ("architectures", "transformers_version")}
    if d.get("model_type") == "dbrx":
        return dbrx_to_mixtral_config(d)
    d.pop("model_type", None)
    return MixtralConfig(**d)


class _MoEInferenceBase(LlamaForCausalLMInference):
    _model_cls = MoEInferenceModel

    @staticmethod
    def _config_from_dir(path: str):
        return moe_config_from_dir(path)

    def _quantize(self) -> None:
        """quantization_type="mxfp4": o_proj, the lm_head and the expert linears become MXFP4 weight-only
        layers (quantization_layers.MXFP4*); the router and the fused QKV stay in the activation dtype."""
        from ..quantization import convert, get_default_mxfp4_qconfig_dict, get_mxfp4_moe_quant_module_mappings

        qt = str(self.config.quantization_type)
        if qt != "mxfp4":
            raise NotImplementedError(f"quantization_type={qt!r}: the MoE applications implement MXFP4 weight-only "
                                      "quantization only; int8 MoE experts are not implemented for inference")
        convert(self.model, get_default_mxfp4_qconfig_dict(), inplace=True, mapping=get_mxfp4_moe_quant_module_mappings())

    def _load_full(self, full_sd) -> None:
        """The packed expert parameters are output-major ([E, out, in/2]) while a full float expert
        weight is [E, in, out], and shard_state_dict slices the full tensor by the parameter's
        partition dim: give it the float expert weights output-major, and hand the layers the shard
        back in its logical [E, in_local, out_local] shape (they quantize it on load)."""
        keys = [n for n, p in self.model.named_parameters()
                if p.dtype == torch.uint8 and p.dim() == 3 and n.endswith(".weight")
                and n in full_sd and full_sd[n].is_floating_point()]
        if not keys:
            return super()._load_full(full_sd)
        full_sd = dict(full_sd)
        if self._mha_from is not None:
            from ..modules.gqa import convert_state_dict_to_mha

            full_sd = convert_state_dict_to_mha(full_sd, *self._mha_from)
        for n in keys:
            full_sd[n] = full_sd[n].transpose(1, 2)
        tp, rank = ps.get_tensor_model_parallel_size(), ps.get_tensor_model_parallel_rank()
        local = shard_state_dict(self.model, full_sd, tp, rank, strict=False)
        for n in keys:
            local[n] = local[n].transpose(1, 2)
        self._load_local(local)


class MixtralForCausalLMInference(_MoEInferenceBase):
    @staticmethod
    def _hf_to_nxd(hf_sd, model_config):
        return mixtral_hf_to_nxd(hf_sd, model_config)


class DbrxForCausalLMInference(_MoEInferenceBase):
    @staticmethod
    def _hf_to_nxd(hf_sd, model_config):
        return dbrx_hf_to_nxd(hf_sd, model_config)


NeuronMixtralForCausalLM = MixtralForCausalLMInference
NeuronDbrxForCausalLM = DbrxForCausalLMInference


def _moe_inference_config(capacity_factor=None, glu_mlp=True, **kwargs) -> InferenceConfig:
    if not glu_mlp:
        raise NotImplementedError("Only GLU experts are supported (reference: neuron_modeling_mixtral.py:65)")
    cfg = InferenceConfig(**kwargs)
    cfg.capacity_factor = float(capacity_factor) if capacity_factor is not None else None
    cfg.glu_mlp = glu_mlp
    return cfg


class MixtralRunner(InferenceRunner):
    """reference: examples/inference/mixtral/mixtral_runner.py"""

    app_cls = MixtralForCausalLMInference

    def load_hf_model(self):
        from transformers import MixtralForCausalLM

        return MixtralForCausalLM.from_pretrained(self.model_path)

    def get_config_for_nxd(self, batch_size: int, tp_degree: int, max_prompt_length: int, sequence_length: int,
                           enable_bucketing: bool = False, **kwargs) -> InferenceConfig:
        return _moe_inference_config(tp_degree=tp_degree, batch_size=batch_size, seq_len=sequence_length,
                                     max_context_length=max_prompt_length, enable_bucketing=enable_bucketing, **kwargs)

    def get_model_config(self):
        return moe_config_from_dir(self.model_path)


class DbrxRunner(MixtralRunner):
    """reference: examples/inference/dbrx/dbrx_runner.py"""

    app_cls = DbrxForCausalLMInference

    def load_hf_model(self):
        from transformers import DbrxForCausalLM

        return DbrxForCausalLM.from_pretrained(self.model_path)
