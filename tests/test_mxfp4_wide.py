"""Routing of MXFP4 products above 16 rows (ops.gemv.mx_wide_ok, knob NXD_MX_WIDE) and the CPU
behaviour of mx_linear at a row count that mx_gemm_wide takes on the GPU."""

import pytest
import torch

from neuronx_distributed_llama3_2_amd.ops import gemv


@pytest.mark.parametrize("knob", [0, 32, 512, 4096])
def test_mx_wide_ok_and_route(monkeypatch, knob):
    monkeypatch.setattr(gemv, "_MX_WIDE", knob)
    top = min(knob, 512)
    assert [gemv.mx_wide_ok(M) for M in range(514)] == [16 < M <= top for M in range(514)]
    # mx_route does not see the knob
    first = gemv._MX_MFMA
    want = ["gemv"] * 8 + ["dequant"] * 9 if first <= 0 else \
        ["gemv"] * (min(first, 9) - 1) + ["gemm"] * (17 - min(first, 9)) + ["dequant"]
    assert [gemv.mx_route(M) for M in range(1, 18)] == want


def test_mx_linear_24_rows_cpu(monkeypatch):
    monkeypatch.setattr(gemv, "_MX_WIDE", 512)
    assert gemv.mx_wide_ok(24)
    torch.manual_seed(0)
    w = torch.randn(24, 96)
    packed, scale = gemv.quantize_mxfp4(w)
    wd = gemv.dequantize_mxfp4(packed, scale, torch.float32)
    x = torch.randn(24, 96)
    b = torch.randn(24)
    torch.testing.assert_close(gemv.mx_linear(x, packed, scale, b), x @ wd.t() + b)
    full = x @ wd.t()
    torch.testing.assert_close(gemv.mx_linear(x, packed, scale, glu=True),
                               torch.nn.functional.silu(full[:, :12]) * full[:, 12:])
