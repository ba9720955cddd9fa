"""Fused SwiGLU: y = silu(gate) * up  (fwd+bwd).

Kernel manifest row: SURVEY.md §2.7 "MLP gate/up + SiLU(.)" — the reference
runs HF LlamaMLP's unfused silu-then-mul.  Fusing the elementwise pair halves
HBM traffic on the [B*S, I] intermediate (I=22016 for 65B), the largest
activation tensor in the layer.
"""

from __future__ import annotations

import torch

from . import use_hip, extension
from .linear import bwd_handoff_enabled, register_handoff


def swiglu_ref(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    gf = gate.float()
    return (gf * torch.sigmoid(gf) * up.float()).to(gate.dtype)


class _SwiGLUHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        ext = extension()
        y = ext.swiglu_fwd(gate, up)
        ctx.save_for_backward(gate, up)
        return y

    @staticmethod
    def backward(ctx, dy):
        gate, up = ctx.saved_tensors
        ext = extension()
        if not bwd_handoff_enabled():
            dgate, dup = ext.swiglu_bwd(dy.contiguous(), gate, up)
            return dgate, dup
        # aligned shapes also get dgate^T / dup^T, which the gate_proj /
        # up_proj wgrads take instead of transposing
        out = ext.swiglu_bwd_t(dy.contiguous(), gate, up)
        if len(out) == 4:
            register_handoff(out[0], out[2])
            register_handoff(out[1], out[3])
        return out[0], out[1]


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    if use_hip(gate):
        return _SwiGLUHIP.apply(gate.contiguous(), up.contiguous())
    return swiglu_ref(gate, up)
