"""ops.linear_fp8w(..., tiled=...) off the GPU: the op is linear_fp8w_ref
whatever the argument or LPP_FP8W_TILED says."""

import torch


def test_tiled_is_the_reference_on_cpu(monkeypatch):
    from lpp_amd import ops
    from lpp_amd.ops.linear import linear_fp8w_ref

    g = torch.Generator().manual_seed(0)
    wq, scale = ops.quantize_weight_fp8(torch.randn(48, 256, generator=g).bfloat16())
    x = torch.randn(70, 256, generator=g).bfloat16()
    ref = linear_fp8w_ref(x, wq, scale)
    assert torch.equal(ops.linear_fp8w(x, wq, scale, tiled=True), ref)
    monkeypatch.setenv("LPP_FP8W_TILED", "1")
    assert torch.equal(ops.linear_fp8w(x, wq, scale), ref)
    assert torch.equal(ops.linear_fp8w(x, wq, scale, tiled=False), ref)
