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

Packed rows (several documents in one [S] row) are described by a
``DocLayout``: attention stays causal and is confined to each document.  The
kernels take two int32 [B,S] tensors instead of a mask and skip the key tiles
no query of a wave can see.

Layout contract: q [B, S, H, D], k/v [B, S, Hkv, D]; returns [B, S, H, D].
"""

from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import use_hip, extension, force_eager


class DocLayout:
    """Document layout of one packed microbatch, shared by every layer of a
    stage (build it once per microbatch, not per layer).

    ``doc_start`` int32 [B,S]: ``doc_start[b,i]`` is the index in row ``b`` of
    the first token of the document that holds token ``i``; non-decreasing
    along ``i``, ``doc_start[b,i] <= i``, ``doc_start[b,0] == 0``, and constant
    over each document (``doc_start[b, doc_start[b,i]] == doc_start[b,i]``).
    Query ``i`` sees key ``j`` iff ``doc_start[b,i] <= j <= i``.  A padding
    token is its own one-token document.

    ``doc_end`` int32 [B,S], derived here on ``doc_start``'s device:
    one past the last token of token ``j``'s document.
    """

    def __init__(self, doc_start: torch.Tensor, validate: bool = True):
        if doc_start.dim() != 2:
            raise ValueError(f"doc_start must be [B,S], got {tuple(doc_start.shape)}")
        if doc_start.dtype is not torch.int32:
            raise ValueError(f"doc_start must be int32, got {doc_start.dtype}")
        if doc_start.shape[1] < 1:
            raise ValueError("doc_start needs at least one token per row")
        doc_start = doc_start.contiguous()
        B, S = doc_start.shape
        idx = torch.arange(S, dtype=torch.int32, device=doc_start.device)
        if validate:
            if bool((doc_start[:, 0] != 0).any()):
                raise ValueError("doc_start[b, 0] must be 0")
            if bool((doc_start < 0).any()) or bool((doc_start > idx).any()):
                raise ValueError("doc_start[b, i] must lie in 0..i")
            if bool((doc_start[:, 1:] < doc_start[:, :-1]).any()):
                raise ValueError("doc_start must be non-decreasing along the row")
            if bool((torch.gather(doc_start, 1, doc_start.long()) != doc_start).any()):
                raise ValueError("doc_start must be constant over each document")
        # doc_end[j] = the next document's start after j, or S: a reversed
        # running minimum over the starts of the boundaries to the right.
        is_first = doc_start == idx
        nxt = torch.where(is_first, idx.expand(B, S), torch.full_like(doc_start, S))
        nxt = torch.cat([nxt[:, 1:], torch.full_like(nxt[:, :1], S)], dim=1)
        self.doc_start = doc_start
        self.doc_end = torch.flip(torch.cummin(torch.flip(nxt, [1]), dim=1).values,
                                  [1]).contiguous()

    @classmethod
    def from_lengths(cls, lengths_per_row: Sequence[Sequence[int]], S: int,
                     device=None) -> "DocLayout":
        """Rows given as document lengths, in order; what is left of a row
        after its documents is padding (one-token documents)."""
        rows = []
        for lengths in lengths_per_row:
            if any(int(n) < 1 for n in lengths) or sum(int(n) for n in lengths) > S:
                raise ValueError(f"document lengths {list(lengths)} do not fit a row of {S}")
            row, at = [], 0
            for n in lengths:
                row += [at] * int(n)
                at += int(n)
            row += list(range(at, S))
            rows.append(row)
        return cls(torch.tensor(rows, dtype=torch.int32, device=device))

    def lengths(self):
        """Document lengths per row, padding tokens as documents of one."""
        out = []
        for ds in self.doc_start.cpu().tolist():
            firsts = [i for i, s in enumerate(ds) if s == i] + [len(ds)]
            out.append([b - a for a, b in zip(firsts[:-1], firsts[1:])])
        return out

    def mask(self) -> torch.Tensor:
        """The block-diagonal causal boolean mask [B,1,S,S] (True = attend):
        the oracle's form, never built on the kernel path."""
        S = self.doc_start.shape[1]
        j = torch.arange(S, device=self.doc_start.device)
        return ((j[None, None, :] >= self.doc_start[:, :, None])
                & (j[None, None, :] <= j[None, :, None]))[:, None]


def causal_attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                         docs: Optional[DocLayout] = None) -> torch.Tensor:
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    qt = q.transpose(1, 2)  # [B,H,S,D]
    kt = k.transpose(1, 2)
    vt = v.transpose(1, 2)
    if Hkv != H:
        rep = H // Hkv
        kt = kt.repeat_interleave(rep, dim=1)
        vt = vt.repeat_interleave(rep, dim=1)
    if docs is None:
        out = torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, is_causal=True)
    else:
        _check_docs(q, docs)
        out = torch.nn.functional.scaled_dot_product_attention(
            qt, kt, vt, attn_mask=docs.mask())
    return out.transpose(1, 2).contiguous()


def _check_docs(q: torch.Tensor, docs: DocLayout) -> None:
    if tuple(docs.doc_start.shape) != (q.shape[0], q.shape[1]):
        raise ValueError(f"DocLayout is {tuple(docs.doc_start.shape)}, "
                         f"q has [B,S] = {tuple(q.shape[:2])}")
    if docs.doc_start.device != q.device:
        raise ValueError(f"DocLayout on {docs.doc_start.device}, q on {q.device}")


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


class _FlashAttnDocsHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, doc_start, doc_end):
        ext = extension()
        o, lse = ext.attention_fwd_docs(q, k, v, doc_start)
        ctx.save_for_backward(q, k, v, o, lse, doc_start, doc_end)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, doc_start, doc_end = ctx.saved_tensors
        ext = extension()
        dq, dk, dv = ext.attention_bwd_docs(do.contiguous(), q, k, v, o, lse,
                                            doc_start, doc_end)
        return dq, dk, dv, None, None


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     docs: Optional[DocLayout] = None) -> torch.Tensor:
    """Causal attention; with ``docs``, confined to each document of a packed
    row (query i sees keys ``doc_start[b,i] .. i``).

    q and k carry RoPE of their absolute row positions, with or without
    ``docs``: a RoPE score depends only on ``i - j``, so under the document
    mask absolute positions give the attention that positions reset per
    document would, up to the rounding of the rotated q/k.  Nothing
    position-shaped accompanies a packed row."""
    if docs is None:
        if use_hip(q) and _hip_supported(q):
            return _FlashAttnHIP.apply(q.contiguous(), k.contiguous(), v.contiguous())
        return causal_attention_ref(q, k, v)
    if use_hip(q) and _hip_supported(q):
        _check_docs(q, docs)
        return _FlashAttnDocsHIP.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                                       docs.doc_start, docs.doc_end)
    return causal_attention_ref(q, k, v, docs)


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
