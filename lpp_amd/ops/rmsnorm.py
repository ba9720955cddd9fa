"""RMSNorm (fwd+bwd).

Kernel manifest row: SURVEY.md §2.7 "RMSNorm x2 + final" — the reference runs
HF ``LlamaRMSNorm`` (imported at models/llama_ds_mp_wrap.py:12, final-norm
LayerSpec at :218).  Memory-bound: target is the HBM roofline (~6.3 TB/s on
MI355X), reached with vectorised bf16x8 loads (guide G13).
"""

from __future__ import annotations

import torch

from . import use_hip, extension
from .linear import bwd_handoff_enabled, register_handoff


def rmsnorm_ref(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """Eager reference: full fp32 math, ONE rounding to the input dtype at
    the end (matches the HIP kernel; HF's LlamaRMSNorm double-rounds by
    casting before the weight multiply)."""
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * weight.float()).to(x.dtype)


class _RMSNormHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        ext = extension()
        y, invrms = ext.rmsnorm_fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, invrms)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, invrms = ctx.saved_tensors
        ext = extension()
        dx, dw = ext.rmsnorm_bwd(dy.contiguous(), x, weight, invrms)
        return dx, dw, None


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    if use_hip(x):
        return _RMSNormHIP.apply(x.contiguous(), weight, eps)
    return rmsnorm_ref(x, weight, eps)


class _RMSNormForkHIP(torch.autograd.Function):
    """Pre-norm residual block entry: ``(residual, y_1 .. y_n)`` from ``x``.

    ``residual`` is ``x`` and every ``y_i`` is the same normed activation,
    one alias per consumer (q/k/v or gate/up).  Because each consumer reads
    its own alias, autograd hands the partial input gradients to this
    backward unsummed, together with the residual-stream gradient, and one
    ``rmsnorm_bwd_fused`` launch does what would otherwise be n-1 elementwise
    adds, the norm backward and one more add — rounding to bf16 at the same
    points, so the result is bit-identical.

    With ``want_t`` the transposed total gradient is registered for the
    wgrad that consumes it (o_proj of this layer or down_proj of the one
    before)."""

    @staticmethod
    def forward(ctx, x, weight, eps, n, want_t):
        ext = extension()
        y, invrms = ext.rmsnorm_fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, invrms)
        ctx.want_t = want_t
        ctx.set_materialize_grads(False)
        return (x.view_as(x),) + tuple(y.view_as(y) for _ in range(n))

    @staticmethod
    def backward(ctx, dres, *dys):
        x, weight, invrms = ctx.saved_tensors
        ext = extension()
        # Autograd sums sibling gradients in the order their backward nodes
        # run, which is the reverse of the forward call order: for q, k, v
        # it computes (dv + dk) + dq.  Same order here, same bits (pinned by
        # tests/test_gpu_bwd_handoff.py::test_layer_matches_unfused).
        parts = [d.contiguous() for d in reversed(dys) if d is not None]
        if not parts:
            return dres, None, None, None, None
        dx, dw, dxT = ext.rmsnorm_bwd_fused(
            parts, x, weight, invrms,
            dres.contiguous() if dres is not None else None, ctx.want_t)
        if dxT.numel():
            register_handoff(dx, dxT)
        return dx, dw, None, None, None


def rmsnorm_fork(x: torch.Tensor, weight: torch.Tensor, eps: float, n: int,
                 want_t: bool = True):
    """``(x, y, y, ...)`` with ``n`` aliases of ``y = rmsnorm(x)`` whose
    backward fuses the sibling-gradient and residual adds (GPU training
    path only; see ``rmsnorm_fork_applies``)."""
    return _RMSNormForkHIP.apply(x.contiguous(), weight, eps, n, want_t)


def rmsnorm_fork_applies(x: torch.Tensor) -> bool:
    return (use_hip(x) and torch.is_grad_enabled() and x.dtype is torch.bfloat16
            and bwd_handoff_enabled())
