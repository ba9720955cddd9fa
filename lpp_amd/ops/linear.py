"""Linear layer whose weight gradient accumulates straight into the
optimizer's flat fp32 buffer (``weight.main_grad``) through a single
hipBLASLt GEMM with beta=1 — no bf16 dW tensor, no separate fp32
accumulation pass (see csrc/wgrad.cpp; SURVEY.md §2.5 grad-accum).

Falls back to stock ``F.linear`` autograd whenever the fused path does not
apply (CPU, eager-forced, no attached optimizer buffer) so all CPU tests
and optimizer-less forward paths are unchanged.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import extension, force_eager, use_hip


class _XTCache:
    """One-entry memo for the backward-side activation transpose.

    q/k/v (and gate/up) share the same input activation and their backwards
    run consecutively, so the xT produced for the first projection is
    reused for its siblings.  Keyed by tensor identity with a STRONG
    reference held, so the storage cannot be recycled under the key."""

    __slots__ = ("x", "xT")

    def __init__(self):
        self.x = None
        self.xT = None

    def get(self, ext, x2: torch.Tensor) -> torch.Tensor:
        # The held strong reference keeps the storage alive, so a matching
        # (data_ptr, shape, dtype) can only be the same activation.
        if (self.x is not None and self.x.data_ptr() == x2.data_ptr()
                and self.x.shape == x2.shape and self.x.dtype == x2.dtype):
            return self.xT
        xT = ext.transpose2d(x2)
        self.x = x2
        self.xT = xT
        return xT

    def clear(self):
        self.x = None
        self.xT = None


_xt_cache = _XTCache()


class _HandoffCache:
    """Transposed wgrad operands handed over by the kernel that produced dy.

    The memory-bound backward kernels (swiglu, rope, the fused norm backward)
    write their gradient and its transposed image together; the producer
    registers ``(natural, image)`` here and the wgrad that consumes that very
    gradient takes the image instead of running ``transpose2d``.  Looked up
    by (data_ptr, shape, dtype) with a STRONG reference held, the same rule
    as ``_XTCache`` and for the same reason.  A hit removes the entry (one
    consumer per gradient); at most ``CAPACITY`` entries, oldest dropped
    first, so an image nobody takes does not outlive the next few
    producers."""

    CAPACITY = 4
    __slots__ = ("entries", "hits", "misses")

    def __init__(self):
        self.entries = []  # [(natural, image)], oldest first
        self.hits = 0
        self.misses = 0

    def put(self, natural: torch.Tensor, image: torch.Tensor) -> None:
        self.entries.append((natural, image))
        if len(self.entries) > self.CAPACITY:
            del self.entries[0]

    def take(self, dy2: torch.Tensor):
        """The image registered for ``dy2`` (removed), or None."""
        for i, (nat, img) in enumerate(self.entries):
            if (nat.data_ptr() == dy2.data_ptr() and nat.shape == dy2.shape
                    and nat.dtype == dy2.dtype):
                del self.entries[i]
                self.hits += 1
                return img
        self.misses += 1
        return None

    def clear(self):
        self.entries.clear()

    def __len__(self):
        return len(self.entries)


_handoff = _HandoffCache()


def bwd_handoff_enabled() -> bool:
    """Producers write the transposed wgrad operand and the norm backward
    fuses the gradient adds (default).  LPP_BWD_HANDOFF=0 restores separate
    transposes, the plain rmsnorm_bwd and autograd's elementwise adds."""
    return os.environ.get("LPP_BWD_HANDOFF", "1") == "1"


def register_handoff(natural: torch.Tensor, image: torch.Tensor) -> None:
    """Called by a producer: ``image`` is ``natural`` viewed [T, C], transposed."""
    _handoff.put(natural.view(image.shape[1], image.shape[0]), image)


def clear_backward_caches() -> None:
    _xt_cache.clear()
    _handoff.clear()


def _wgrad_pre_enabled() -> bool:
    return os.environ.get("LPP_WGRAD_PRE", "1") == "1"


def _wgrad_bf16d_enabled() -> bool:
    """bf16-D wgrad GEMM + separate fp32 accumulate (default): hipBLASLt's
    bf16-D solution pool is 15-20% faster than fp32-D at the 65B shapes and
    the accumulate pass is ~5% of the GEMM.  Numerics match the reference
    stack's own flow (bf16 dW per microbatch, fp32 accumulation across
    microbatches — SURVEY.md §2.5).  Set LPP_WGRAD_BF16D=0 for the exact
    fp32-D GEMM epilogue."""
    return os.environ.get("LPP_WGRAD_BF16D", "1") == "1"


def _dgrad_wt_enabled() -> bool:
    return os.environ.get("LPP_DGRAD_WT", "1") == "1"


def _weight_t(ext, weight: torch.nn.Parameter) -> torch.Tensor:
    """Cached transposed weight for the dgrad GEMM.

    dx = dy @ W is the k-strided hipBLASLt class (the contraction dim runs
    down W's rows) and measures 8-21% below the k-contiguous class at the
    65B shapes (profiles/r02_gemm_probe2.txt).  W only changes at the
    optimizer step, so one transposed copy per step turns every dgrad into
    the fast class:  dx = dy @ (W^T)^T with W^T materialised [in, out].
    The engine invalidates the cache after each optimizer step
    (engine._optimizer_step -> invalidate_weight_transposes)."""
    wt = getattr(weight, "_wt", None)
    if wt is None:
        wt = ext.transpose2d(weight.data)
        weight._wt = wt
    return wt


def invalidate_weight_transposes(module: torch.nn.Module) -> None:
    """Drop cached W^T copies (call after any in-place weight update)."""
    for p in module.parameters():
        if hasattr(p, "_wt"):
            p._wt = None


class _LinearWgradF32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.nn.Parameter):
        ctx.save_for_backward(x, weight)
        # saved_tensors unwraps the Parameter, so keep the fp32 buffer
        # reference directly (it is optimizer state, not part of the graph)
        ctx.main_grad = weight.main_grad
        return F.linear(x, weight)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        ext = extension()
        if _dgrad_wt_enabled():
            dx = dy @ _weight_t(ext, weight).t()
        else:
            dx = dy @ weight
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        dy2 = dy.reshape(-1, dy.shape[-1])
        if _wgrad_pre_enabled():
            # Pre-transposed formulation: both GEMM operands k-contiguous
            # (the fast hipBLASLt class, +25-40% over the natural TN
            # layout) at the cost of two HBM-speed LDS-tiled transposes;
            # the x transpose is shared across sibling projections.
            xT = _xt_cache.get(ext, x2)
            dyT = _handoff.take(dy2) if bwd_handoff_enabled() else None
            if dyT is None:
                dyT = ext.transpose2d(dy2)
            if _wgrad_bf16d_enabled():
                ext.accum_bf16_f32(ctx.main_grad.view(-1),
                                   torch.matmul(dyT, xT.t()).view(-1))
            else:
                ext.wgrad_f32_accum_pre(xT, dyT, ctx.main_grad)
        else:
            ext.wgrad_f32_accum(x2, dy2, ctx.main_grad)
        # This path bypasses autograd's grad accumulation, so the engine's
        # DP-bucket overlap (post-accumulate hooks) must be notified here.
        cb = getattr(weight, "_on_accumulate", None)
        if cb is not None:
            cb(weight)
        return dx, None


def lp_linear(x: torch.Tensor, weight: torch.nn.Parameter) -> torch.Tensor:
    """F.linear with fused-fp32-wgrad backward when the optimizer has
    attached ``main_grad`` (training on GPU); plain autograd otherwise."""
    if (
        x.is_cuda
        and x.dtype is torch.bfloat16
        and torch.is_grad_enabled()
        and weight.requires_grad
        and hasattr(weight, "main_grad")
        and not force_eager()
    ):
        return _LinearWgradF32.apply(x, weight)
    return F.linear(x, weight)


# ---------------------------------------------------------------------------
# FP8 weight-only linear (serving).  A weight [out, in] is held as e4m3 bytes
# and one power-of-two fp32 scale per (output row, block of 128 inputs): the
# KV-cache rule (ops.quantize_kv_rows_fp8) applied to each block, so byte *
# scale is exact in bf16 and the product is a bf16 GEMM over the dequantised
# weight.  Activations stay bf16 (W8A16); csrc/linear_fp8w.hip.
# ---------------------------------------------------------------------------
FP8W_BLOCK = 128     # inputs per scale
FP8W_MAX_M = 64      # rows of x the kernel serves


def quantize_weight_fp8(w: torch.Tensor):
    """``w [out, in]`` -> ``(wq float8_e4m3fn [out, in], scale fp32 [out,
    in/128])``; needs ``in % 128 == 0`` and ``out % 16 == 0``."""
    from .attention import quantize_kv_rows_fp8

    if w.dim() != 2:
        raise ValueError(f"quantize_weight_fp8: weight must be [out, in], got {tuple(w.shape)}")
    out, inn = w.shape
    if inn % FP8W_BLOCK or out % 16:
        raise ValueError(f"quantize_weight_fp8: needs in % {FP8W_BLOCK} == 0 and out % 16 == 0, "
                         f"got [out, in] = [{out}, {inn}]")
    wq, scale = quantize_kv_rows_fp8(w.reshape(out, inn // FP8W_BLOCK, FP8W_BLOCK))
    return wq.reshape(out, inn), scale


def _dequant_weight_ref(wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The bf16 weight of (wq, scale), exactly, in stock torch ops."""
    out, inn = wq.shape
    w = wq.float().view(out, inn // FP8W_BLOCK, FP8W_BLOCK) * scale[..., None]
    return w.view(out, inn).to(torch.bfloat16)


def linear_fp8w_ref(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``F.linear`` over the dequantised bf16 weight: the CPU path and the
    kernel's oracle, bit for bit a model that holds the dequantised weights."""
    return F.linear(x, _dequant_weight_ref(wq, scale).to(x.dtype))


def _fp8w_tiled_enabled() -> bool:
    """Above 64 rows take the tiled fp8 kernel instead of dequantise +
    hipBLASLt.  Off by default; LPP_FP8W_TILED=1 turns it on."""
    return os.environ.get("LPP_FP8W_TILED", "0") == "1"


def linear_fp8w(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor,
                tiled: bool | None = None) -> torch.Tensor:
    """``x [..., in] @ dequant(wq, scale)^T -> [..., out]``, inference only.

    On the GPU with bf16 x and at most 64 rows (decode ticks) the skinny
    gfx950 kernel streams the e4m3 weight once; its result does not depend on
    how many rows ride together, and it always serves this range.  Above 64
    rows (prefill ticks, whole-prompt admission) there are two paths:

    * default: the weight is dequantised into a bf16 scratch tensor by
      ``linear_fp8w_dequant`` and ``F.linear`` (hipBLASLt) runs over it;
    * ``tiled=True``, or ``tiled=None`` with ``LPP_FP8W_TILED=1``: the tiled
      gfx950 kernel (``linear_fp8w_tiled``) reads the e4m3 bytes once per
      128-token tile and dequantises them on the way into LDS, with no bf16
      copy of the weight.  It splits K by a rule of (in, out, number of
      token tiles), so the same call returns the same bits every time, but
      the bits of a row may depend on how many rows ride along, as they may
      on the hipBLASLt path.

    ``tiled=False`` forces the default path.  On the CPU or under
    ``LPP_FORCE_EAGER`` the op is ``linear_fp8w_ref`` whatever ``tiled`` says."""
    if not use_hip(x):
        return linear_fp8w_ref(x, wq, scale)
    if x.dtype is not torch.bfloat16:
        raise ValueError(f"linear_fp8w: the gfx950 kernel takes bf16 x, got {x.dtype}")
    ext = extension()
    if x.dim() < 1 or x.shape[-1] != wq.shape[1]:
        raise ValueError(f"linear_fp8w: x [..., {x.shape[-1] if x.dim() else '?'}] against a "
                         f"weight [out, in] = {tuple(wq.shape)}")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[0] == 0:
        return x.new_empty(*lead, wq.shape[0])
    if x2.shape[0] <= FP8W_MAX_M:
        y = ext.linear_fp8w(x2, wq, scale)   # raises on a non-contiguous x
    elif _fp8w_tiled_enabled() if tiled is None else tiled:
        y = ext.linear_fp8w_tiled(x2, wq, scale, 0)
    else:
        y = F.linear(x2, ext.linear_fp8w_dequant(wq, scale))
    return y.view(*lead, wq.shape[0])


def quantize_module_fp8_(mod: torch.nn.Module) -> None:
    """Replace ``mod.weight`` by the buffers ``weight_fp8`` / ``weight_scale``."""
    if getattr(mod, "weight", None) is None:
        return  # already quantised
    wq, scale = quantize_weight_fp8(mod.weight.data)
    mod.register_parameter("weight", None)   # the bf16 storage goes with its last reference
    mod.register_buffer("weight_fp8", wq)
    mod.register_buffer("weight_scale", scale)


def forward_fp8(mod: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
    if torch.is_grad_enabled():
        raise RuntimeError(f"{type(mod).__name__}: fp8 weights are inference-only; call under "
                           "torch.no_grad()")
    return linear_fp8w(x, mod.weight_fp8, mod.weight_scale)


# ---------------------------------------------------------------------------
# MXFP4 weight-only linear (serving).  A weight [out, in] is held in the OCP
# microscaling format: e2m1 nibbles, two per byte (element 2i in the low
# nibble of byte i), and one e8m0 scale byte per (output row, block of 32
# inputs).  code * 2^(b-127) is exact in bf16, so the product is a bf16 GEMM
# over the dequantised weight.  Activations stay bf16 (W4A16);
# csrc/linear_fp4w.hip.
# ---------------------------------------------------------------------------
FP4W_BLOCK = 32      # inputs per scale byte
FP4W_MAX_M = 64      # rows of x the kernel serves
FP4W_MIN_EXP = -100  # the contract on a scale byte b: |b - 127| <= 100
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 from an integer tensor, -126 <= e <= 127, on the float's bits."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quantize_weight_fp4(w: torch.Tensor):
    """``w [out, in]`` -> ``(wq uint8 [out, in/2], scale uint8 [out, in/32])``
    in the MXFP4 format; needs ``in % 128 == 0`` and ``out % 16 == 0``.

    Per block of 32 inputs, with amax = m 2^E, 0.5 <= m < 1: the scale is 2^e,
    e = E - 3 if m <= 0.75 else E - 2, e >= -100, e = 0 for a block of zeros,
    stored as the e8m0 byte e + 127.  Then 3 < amax / 2^e <= 6, nothing
    saturates, and values round to the nearest e2m1 code, ties to the even
    code, so |w - deq| <= amax / 4 per block.  A weight above 2^102 in
    magnitude would need a byte above 227, outside the kernel's contract."""
    if w.dim() != 2:
        raise ValueError(f"quantize_weight_fp4: weight must be [out, in], got {tuple(w.shape)}")
    out, inn = w.shape
    if inn % 128 or out % 16:
        raise ValueError(f"quantize_weight_fp4: needs in % 128 == 0 and out % 16 == 0, "
                         f"got [out, in] = [{out}, {inn}]")
    wf = w.detach().float().view(out, inn // FP4W_BLOCK, FP4W_BLOCK)
    bits = wf.abs().amax(-1, keepdim=True).view(torch.int32)
    # amax = 1.f 2^(b-127) = (1.f / 2) 2^(b-126), and m <= 0.75 iff 1.f <= 1.5
    E = (bits >> 23) - 126
    e = torch.where((bits & 0x7FFFFF) <= 0x400000, E - 3, E - 2).clamp_(min=FP4W_MIN_EXP)
    e = torch.where(bits == 0, torch.zeros_like(e), e)
    v = wf.abs() * _pow2(-e)
    # the code is the number of midpoints passed; a tie stays on the even code
    code = ((v > 0.25).to(torch.uint8) + (v >= 0.75) + (v > 1.25) + (v >= 1.75)
            + (v > 2.5) + (v >= 3.5) + (v > 5.0))
    nib = (code | ((wf < 0).to(torch.uint8) << 3)).view(out, inn // 2, 2)
    wq = nib[..., 0] | (nib[..., 1] << 4)
    return wq.contiguous(), (e + 127).to(torch.uint8).view(out, inn // FP4W_BLOCK)


def _dequant_weight_fp4_ref(wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The bf16 weight of (wq, scale), exactly, in stock torch ops."""
    out, half = wq.shape
    lut = torch.tensor(_E2M1 + tuple(-c for c in _E2M1), device=wq.device)
    val = lut[torch.stack((wq & 15, wq >> 4), -1).long()]          # [out, in/2, 2]
    w = val.view(out, -1, FP4W_BLOCK) * _pow2(scale.to(torch.int32) - 127)[..., None]
    return w.view(out, 2 * half).to(torch.bfloat16)


def linear_fp4w_ref(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``F.linear`` over the dequantised bf16 weight: the CPU path and the
    kernel's oracle, bit for bit a model that holds the dequantised weights."""
    return F.linear(x, _dequant_weight_fp4_ref(wq, scale).to(x.dtype))


def linear_fp4w(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``x [..., in] @ dequant(wq, scale)^T -> [..., out]``, inference only.

    ``wq`` is ``uint8 [out, in/2]``, two e2m1 values per byte, element 2i of a
    row in the low nibble of byte i (the ``float4_e2m1fn_x2`` order); ``scale``
    is ``uint8 [out, in/32]``, e8m0: byte b stands for 2^(b-127).  The contract
    is 27 <= b <= 227, which keeps every dequantised value a normal bf16;
    bytes outside it are not checked and their result is undefined.

    On the GPU with bf16 x and at most 64 rows (decode ticks) the skinny
    gfx950 kernel streams the packed weight once; its result does not depend
    on how many rows ride together.  Above 64 rows the weight is dequantised
    into a bf16 scratch tensor by ``linear_fp4w_dequant`` and ``F.linear``
    (hipBLASLt) runs over it.  On the CPU or under ``LPP_FORCE_EAGER`` the op
    is ``linear_fp4w_ref``."""
    if not use_hip(x):
        return linear_fp4w_ref(x, wq, scale)
    if x.dtype is not torch.bfloat16:
        raise ValueError(f"linear_fp4w: the gfx950 kernel takes bf16 x, got {x.dtype}")
    ext = extension()
    if x.dim() < 1 or wq.dim() != 2 or x.shape[-1] != 2 * wq.shape[1]:
        raise ValueError(f"linear_fp4w: x [..., {x.shape[-1] if x.dim() else '?'}] against a "
                         f"packed weight [out, in/2] = {tuple(wq.shape)}")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[0] == 0:
        return x.new_empty(*lead, wq.shape[0])
    if x2.shape[0] <= FP4W_MAX_M:
        y = ext.linear_fp4w(x2, wq, scale)   # raises on a non-contiguous x
    else:
        y = F.linear(x2, ext.linear_fp4w_dequant(wq, scale))
    return y.view(*lead, wq.shape[0])


def quantize_module_fp4_(mod: torch.nn.Module) -> None:
    """Replace ``mod.weight`` by the buffers ``weight_fp4`` / ``weight_scale``."""
    if getattr(mod, "weight", None) is None:
        return  # already quantised
    wq, scale = quantize_weight_fp4(mod.weight.data)
    mod.register_parameter("weight", None)   # the bf16 storage goes with its last reference
    mod.register_buffer("weight_fp4", wq)
    mod.register_buffer("weight_scale", scale)


def forward_quantized(mod: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
    """The forward of a module whose weight is held quantised, by the buffer it holds."""
    if getattr(mod, "weight_fp4", None) is None:
        return forward_fp8(mod, x)
    if torch.is_grad_enabled():
        raise RuntimeError(f"{type(mod).__name__}: fp4 weights are inference-only; call under "
                           "torch.no_grad()")
    return linear_fp4w(x, mod.weight_fp4, mod.weight_scale)


class LPLinear(torch.nn.Linear):
    """Drop-in nn.Linear (bias-free) using the fused-wgrad path."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False):
        assert not bias, "LLaMA projections are bias-free"
        super().__init__(in_features, out_features, bias=False)

    def quantize_fp8_(self) -> "LPLinear":
        """Hold the weight as e4m3 + block scales from now on (inference only)."""
        quantize_module_fp8_(self)
        return self

    def quantize_fp4_(self) -> "LPLinear":
        """Hold the weight as MXFP4 (e2m1 + e8m0 per 32) from now on (inference only)."""
        quantize_module_fp4_(self)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.weight is None:
            return forward_quantized(self, x)
        return lp_linear(x, self.weight)
