"""Causal self-attention core.

The reference runs *materialised-mask eager attention* — the [B,1,S,S] fp16
additive mask is built host-side in the collator (data/flan.py:194-243) and
shipped through every pipeline stage; flash attention was documented broken
under DeepSpeed-PP (README.md:141-143).  This module fixes that design:
the mask is implicit (causal) — nothing S^2-shaped is ever materialised,
shipped over xGMI, or saved for backward.

Dispatch:
- HIP flash-style kernel (gfx950 MFMA, online softmax) when available.
- Otherwise torch SDPA with ``is_causal=True`` (CPU tests / A-B baseline).

Layout contract: q [B, S, H, D], k/v [B, S, Hkv, D]; returns [B, S, H, D].
"""

from __future__ import annotations

import torch

from . import use_hip, extension, force_eager


def causal_attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    qt = q.transpose(1, 2)  # [B,H,S,D]
    kt = k.transpose(1, 2)
    vt = v.transpose(1, 2)
    if Hkv != H:
        rep = H // Hkv
        kt = kt.repeat_interleave(rep, dim=1)
        vt = vt.repeat_interleave(rep, dim=1)
    out = torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, is_causal=True)
    return out.transpose(1, 2).contiguous()


def _hip_supported(q: torch.Tensor) -> bool:
    """HIP flash kernels cover the production shape: bf16, head_dim 128."""
    if force_eager():
        return False
    if q.dtype is not torch.bfloat16 or q.shape[-1] != 128:
        return False
    ext = extension()  # raises loudly if the native path is missing on GPU
    return hasattr(ext, "attention_fwd") and hasattr(ext, "attention_bwd")


class _FlashAttnHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v):
        ext = extension()
        o, lse = ext.attention_fwd(q, k, v)
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        ext = extension()
        dq, dk, dv = ext.attention_bwd(do.contiguous(), q, k, v, o, lse)
        return dq, dk, dv


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    if use_hip(q) and _hip_supported(q):
        return _FlashAttnHIP.apply(q.contiguous(), k.contiguous(), v.contiguous())
    return causal_attention_ref(q, k, v)


# ---------------------------------------------------------------------------
# Single-token decode over a KV cache with per-row positions.
#
# Contract (both implementations): q [N,1,H,D], k_new/v_new [N,1,Hkv,D],
# k_cache/v_cache [slots,Tmax,Hkv,D], cos/sin [Smax,D/2] fp32.  Batch row n
# sits at position positions[n] of cache row rows[n] (rows=None: row n).
# In place: rotated k_new and v_new land at [row, position], lengths[row]
# becomes position + 1.  Returns o [N,1,H,D]: rotated q attending keys
# 0..position of its row, the new token included.
# ---------------------------------------------------------------------------

_DECODE_REPS = (1, 2, 4, 8)


def decode_attention_hip_supported(q: torch.Tensor, num_kv_heads: int) -> bool:
    """True when ``decode_attention`` runs the fused gfx950 kernel for a
    query of this device/dtype/geometry (else it runs the reference)."""
    if not use_hip(q):
        return False
    if q.dtype is not torch.bfloat16 or q.shape[-1] != 128:
        return False
    H = q.shape[-2]
    if num_kv_heads <= 0 or H % num_kv_heads or H // num_kv_heads not in _DECODE_REPS:
        return False
    return hasattr(extension(), "attention_decode")


def _positions_tensor(positions, N: int, device) -> torch.Tensor:
    if isinstance(positions, int):
        return torch.full((N,), positions, dtype=torch.long, device=device)
    return positions


@torch.no_grad()
def decode_attention_ref(q, k_new, v_new, k_cache, v_cache, cos, sin, positions, *,
                         rows=None, lengths=None, max_len=None) -> torch.Tensor:
    """Plain per-row fp32 composition: rotate (the apply_rope_positions
    formula), round to the cache dtype, write, softmax over keys 0..p.
    The CPU path and the oracle of the kernel; ``max_len`` is unused."""
    from .rope import apply_rope_positions

    N, _, H, D = q.shape
    Hkv = k_new.shape[2]
    rep = H // Hkv
    pos = _positions_tensor(positions, N, q.device)
    row_t = rows if rows is not None else torch.arange(N, device=q.device)
    qr = apply_rope_positions(q, cos, sin, pos)
    kr = apply_rope_positions(k_new, cos, sin, pos).to(k_cache.dtype)
    k_cache[row_t, pos] = kr[:, 0]
    v_cache[row_t, pos] = v_new[:, 0].to(v_cache.dtype)
    if lengths is not None:
        lengths[row_t] = pos + 1
    scale = 1.0 / (D ** 0.5)
    o = torch.empty_like(q)
    for n, (r, p) in enumerate(zip(row_t.tolist(), pos.tolist())):
        kk = k_cache[r, : p + 1].float().repeat_interleave(rep, dim=1)  # [T,H,D]
        vv = v_cache[r, : p + 1].float().repeat_interleave(rep, dim=1)
        s = torch.einsum("hd,thd->ht", qr[n, 0].float(), kk) * scale
        o[n, 0] = torch.einsum("ht,thd->hd", torch.softmax(s, dim=-1), vv).to(q.dtype)
    return o


def _shares_storage(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (a.device == b.device
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr())


@torch.no_grad()
def decode_attention(q, k_new, v_new, k_cache, v_cache, cos, sin, positions, *,
                     rows=None, lengths=None, max_len=None) -> torch.Tensor:
    """Fused RoPE + cache write + GQA decode attention (one kernel launch plus
    a small combine) for bf16 / head_dim 128 / H/Hkv in {1,2,4,8} on the GPU;
    ``decode_attention_ref`` otherwise.  ``positions`` is a long tensor [N] or
    an int (every row at that position).  ``max_len`` is a host bound on
    every position + 1 (default: the cache length); a tighter bound launches
    fewer workgroups."""
    if not decode_attention_hip_supported(q, k_new.shape[2]):
        return decode_attention_ref(q, k_new, v_new, k_cache, v_cache, cos, sin,
                                    positions, rows=rows, lengths=lengths, max_len=max_len)
    ext = extension()
    pos_t, upos = (None, positions) if isinstance(positions, int) else (positions, 0)
    if pos_t is not None and lengths is not None and _shares_storage(pos_t, lengths):
        # the kernel stores lengths[row] while other workgroups still read positions
        pos_t = pos_t.clone()
    if pos_t is not None:
        pos_t = pos_t.contiguous()
    if rows is not None:
        rows = rows.contiguous()
    if max_len is None:
        max_len = min(k_cache.shape[1], cos.shape[0])
    return ext.attention_decode(q.contiguous(), k_new.contiguous(), v_new.contiguous(),
                                k_cache, v_cache, cos, sin, pos_t, rows, lengths,
                                upos, int(max_len))
