"""Routing of the MXFP4 decode products (ops.gemv.mx_route, knob NXD_MX_MFMA) and the CPU behaviour
of mx_linear / mx_experts_linear at the row counts that the MFMA form takes on the GPU."""

import pytest
import torch

from neuronx_distributed_llama3_2_amd.ops import gemv


def _routes():
    return [gemv.mx_route(M) for M in range(1, 18)]


def test_mx_route_default(monkeypatch):
    """The shipped default: a single row stays on the VALU kernel, rows from the default on (at most
    9) up to 16 take the MFMA form, 17 dequantises."""
    first = gemv._MX_MFMA_DEFAULT
    assert 2 <= first <= 9
    monkeypatch.setattr(gemv, "_MX_MFMA", first)
    assert _routes() == ["gemv"] * (first - 1) + ["gemm"] * (17 - first) + ["dequant"]
    assert gemv.mx_route(0) == "dequant"


@pytest.mark.parametrize("knob,want", [
    (0, ["gemv"] * 8 + ["dequant"] * 9),
    (2, ["gemv"] + ["gemm"] * 15 + ["dequant"]),
    (9, ["gemv"] * 8 + ["gemm"] * 8 + ["dequant"]),
    (12, ["gemv"] * 8 + ["gemm"] * 8 + ["dequant"]),   # rows 9..16 take the MFMA form whenever it is on
])
def test_mx_route_knob(monkeypatch, knob, want):
    monkeypatch.setattr(gemv, "_MX_MFMA", knob)
    assert _routes() == want


def test_mx_linear_12_rows_cpu():
    torch.manual_seed(0)
    w = torch.randn(24, 96)
    packed, scale = gemv.quantize_mxfp4(w)
    wd = gemv.dequantize_mxfp4(packed, scale, torch.float32)
    x = torch.randn(12, 96)
    b = torch.randn(24)
    assert gemv.mx_route(12) != "gemv"
    torch.testing.assert_close(gemv.mx_linear(x, packed, scale, b), x @ wd.t() + b)
    full = x @ wd.t()
    torch.testing.assert_close(gemv.mx_linear(x, packed, scale, glu=True),
                               torch.nn.functional.silu(full[:, :12]) * full[:, 12:])


def test_mx_experts_linear_16_rows_cpu():
    """The all-experts op is not routed to the MFMA form; at 16 rows it stays the dequantize reference."""
    torch.manual_seed(1)
    E = 3
    w = torch.randn(E, 10, 64)
    packed, scale = gemv.quantize_mxfp4(w)
    wd = gemv.dequantize_mxfp4(packed, scale, torch.float32)
    xs = torch.randn(16, 64)
    xp = torch.randn(E, 16, 64)
    torch.testing.assert_close(gemv.mx_experts_linear(xs, packed, scale), torch.einsum("mk,enk->emn", xs, wd))
    torch.testing.assert_close(gemv.mx_experts_linear(xp, packed, scale), torch.einsum("emk,enk->emn", xp, wd))
