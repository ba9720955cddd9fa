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
# decode alone also serves groups of 16 (attention_decode_mfma.hip); extend
# stays at _DECODE_REPS and runs its reference there
_DECODE_KERNEL_REPS = _DECODE_REPS + (16,)
_DECODE_IMPLS = {None: 0, "valu": 1, "mfma": 2}

# ---------------------------------------------------------------------------
# FP8 KV cache (opt-in).  k_cache / v_cache are float8_e4m3fn
# [slots,Tmax,Hkv,128]; k_scale / v_scale are fp32 [slots,Hkv,Tmax], one
# power-of-two scale per (slot, kv head, token).  A stored row is the
# round-to-nearest-even e4m3 of x / scale, and byte * scale is exact in bf16.
# ---------------------------------------------------------------------------
FP8_KV_DTYPE = torch.float8_e4m3fn
_FP8_MIN_EXP = -100


def quantize_kv_rows_fp8(x: torch.Tensor):
    """Quantise rows [..., D] to (e4m3 [..., D], fp32 scale [...]).  With
    ``amax = m * 2**E``, ``0.5 <= m < 1``: ``scale = 2**(E - 9)`` if
    ``m <= 0.875`` else ``2**(E - 8)``, never below ``2**-100``, and 1 for a
    row of zeros - so ``|x| / scale <= 448`` and nothing saturates."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    m, E = torch.frexp(amax)
    e = torch.where(m <= 0.875, E - 9, E - 8).clamp(min=_FP8_MIN_EXP)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    scale = torch.ldexp(torch.ones_like(amax), e)
    return (xf / scale[..., None]).to(FP8_KV_DTYPE), scale


def _check_fp8_args(who: str, k_cache, v_cache, k_scale, v_scale) -> bool:
    """True for an fp8 cache (both scales required), False for any other."""
    fp8 = k_cache.dtype is FP8_KV_DTYPE
    if fp8 != (v_cache.dtype is FP8_KV_DTYPE):
        raise ValueError(f"{who}: k_cache and v_cache must share a dtype")
    if fp8 and (k_scale is None or v_scale is None):
        raise ValueError(f"{who}: an fp8 cache needs k_scale and v_scale")
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError(f"{who}: k_scale / v_scale go with a float8_e4m3fn cache only")
    return fp8


def _cache_store(cache, scale, r, t, x):
    """cache[r, t] = x ([.., Hkv, D]; r, t index tensors or an int and a
    slice), quantised when the cache has a scale."""
    if scale is None:
        cache[r, t] = x.to(cache.dtype)
        return
    qb, sc = quantize_kv_rows_fp8(x)
    cache.view(torch.uint8)[r, t] = qb.view(torch.uint8)   # bytes: fp8 has no index_put
    if isinstance(t, slice):
        scale[r, :, t] = sc.T          # [ln,Hkv] -> [Hkv,ln]
    else:
        scale[r, :, t] = sc            # advanced indices first: [N,Hkv]


def _cache_prefix(cache, scale, r: int, T: int) -> torch.Tensor:
    """fp32 [T,Hkv,D] of cache row r, dequantised when the cache has a scale."""
    x = cache[r, :T].float()
    return x if scale is None else x * scale[r, :, :T].T[..., None]


# ---------------------------------------------------------------------------
# Paged KV cache (opt-in).  With ``block_table`` (int32 [table_rows,
# max_pages]) k_cache / v_cache are a pool [num_pages, page, Hkv, D] (scales
# [num_pages, Hkv, page]) and token t of table row r lives at
# cache[block_table[r, t // page], t % page]; ``rows`` selects table rows and
# ``lengths`` is [table_rows].  The kernels serve page == 64.
# ---------------------------------------------------------------------------
PAGE_TOKENS = 64


def _check_block_table(who: str, block_table, k_cache) -> None:
    if block_table.dim() != 2 or block_table.dtype is not torch.int32:
        raise ValueError(f"{who}: block_table must be int32 [table_rows, max_pages], got "
                         f"{block_table.dtype} {tuple(block_table.shape)}")
    if block_table.device != k_cache.device:
        raise ValueError(f"{who}: block_table on {block_table.device}, the cache on "
                         f"{k_cache.device}")


def _gather_pages(cache, scale, block_table):
    """The slot-layout copy of a pool: cache [table_rows, max_pages * page, Hkv,
    D] and scale [table_rows, Hkv, max_pages * page] (or None).  Ids outside
    the pool (entries no token uses) are clamped."""
    bt = block_table.long().clamp(0, cache.shape[0] - 1)
    R, M = bt.shape
    P, Hkv = cache.shape[1], cache.shape[2]
    slot = cache.view(torch.uint8)[bt].reshape(R, M * P, Hkv, -1).view(cache.dtype)
    if scale is None:
        return slot, None
    return slot, scale[bt].permute(0, 2, 1, 3).reshape(R, Hkv, M * P)


def _cache_tokens(k_cache, block_table) -> int:
    """Tokens a row can hold: Tmax, or max_pages * page with a table."""
    if block_table is None:
        return k_cache.shape[1]
    return block_table.shape[1] * k_cache.shape[1]


def _scatter_pages(cache, scale, slot, slot_scale, block_table, r: int, t0: int, t1: int):
    """Tokens t0 .. t1-1 of table row r, from the slot-layout copy back into
    the pool (bytes, and scales when there are any)."""
    t = torch.arange(t0, t1, device=cache.device)
    P = cache.shape[1]
    pg, off = block_table[r, t // P].long(), t % P
    cache.view(torch.uint8)[pg, off] = slot.view(torch.uint8)[r, t0:t1]
    if scale is not None:
        scale[pg, :, off] = slot_scale[r, :, t0:t1].T


def decode_attention_hip_supported(q: torch.Tensor, num_kv_heads: int,
                                   cache_dtype: Optional[torch.dtype] = None,
                                   page_size: Optional[int] = None) -> bool:
    """True when ``decode_attention`` runs the fused gfx950 kernel for a
    query of this device/dtype/geometry (else it runs the reference).
    ``cache_dtype``: None or bf16 for the bf16 cache, ``float8_e4m3fn`` for
    the fp8 one.  ``page_size``: the page of a paged cache (one called with a
    ``block_table``), None for the slot cache."""
    if not use_hip(q):
        return False
    if page_size not in (None, PAGE_TOKENS):
        return False
    if cache_dtype not in (None, torch.bfloat16, FP8_KV_DTYPE):
        return False
    if q.dtype is not torch.bfloat16 or q.shape[-1] != 128:
        return False
    H = q.shape[-2]
    if num_kv_heads <= 0 or H % num_kv_heads or H // num_kv_heads not in _DECODE_KERNEL_REPS:
        return False
    name = "attention_decode_fp8" if cache_dtype is FP8_KV_DTYPE else "attention_decode"
    return hasattr(extension(), name)


def _positions_tensor(positions, N: int, device) -> torch.Tensor:
    if isinstance(positions, int):
        return torch.full((N,), positions, dtype=torch.long, device=device)
    return positions


@torch.no_grad()
def decode_attention_ref(q, k_new, v_new, k_cache, v_cache, cos, sin, positions, *,
                         rows=None, lengths=None, max_len=None,
                         k_scale=None, v_scale=None, block_table=None) -> torch.Tensor:
    """Plain per-row fp32 composition: rotate (the apply_rope_positions
    formula), round to the cache dtype, write, softmax over keys 0..p.
    The CPU path and the oracle of the kernel; ``max_len`` is unused.
    With fp8 caches the rotated bf16 K row and the V row are quantised
    (``quantize_kv_rows_fp8``), byte and scale are written, and the new token
    is attended as its dequantised self, like every cached one.
    With ``block_table`` the caches are a paged pool of any page size: the
    table rows are gathered into a slot-layout copy, the composition runs on
    it, and each row's new token is scattered back to its page."""
    from .rope import apply_rope_positions

    _check_fp8_args("decode_attention_ref", k_cache, v_cache, k_scale, v_scale)

    N, _, H, D = q.shape
    if block_table is not None:
        _check_block_table("decode_attention_ref", block_table, k_cache)
        ks, kss = _gather_pages(k_cache, k_scale, block_table)
        vs, vss = _gather_pages(v_cache, v_scale, block_table)
        o = decode_attention_ref(q, k_new, v_new, ks, vs, cos, sin, positions, rows=rows,
                                 lengths=lengths, k_scale=kss, v_scale=vss)
        row_l = rows.tolist() if rows is not None else range(N)
        for r, p in zip(row_l, _positions_tensor(positions, N, q.device).tolist()):
            _scatter_pages(k_cache, k_scale, ks, kss, block_table, r, p, p + 1)
            _scatter_pages(v_cache, v_scale, vs, vss, block_table, r, p, p + 1)
        return o
    Hkv = k_new.shape[2]
    rep = H // Hkv
    pos = _positions_tensor(positions, N, q.device)
    row_t = rows if rows is not None else torch.arange(N, device=q.device)
    qr = apply_rope_positions(q, cos, sin, pos)
    kr = apply_rope_positions(k_new, cos, sin, pos)
    _cache_store(k_cache, k_scale, row_t, pos, kr[:, 0])
    _cache_store(v_cache, v_scale, row_t, pos, v_new[:, 0])
    if lengths is not None:
        lengths[row_t] = pos + 1
    scale = 1.0 / (D ** 0.5)
    o = torch.empty_like(q)
    for n, (r, p) in enumerate(zip(row_t.tolist(), pos.tolist())):
        kk = _cache_prefix(k_cache, k_scale, r, p + 1).repeat_interleave(rep, dim=1)  # [T,H,D]
        vv = _cache_prefix(v_cache, v_scale, r, p + 1).repeat_interleave(rep, dim=1)
        s = torch.einsum("hd,thd->ht", qr[n, 0].float(), kk) * scale
        o[n, 0] = torch.einsum("ht,thd->hd", torch.softmax(s, dim=-1), vv).to(q.dtype)
    return o


def _shares_storage(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (a.device == b.device
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr())


@torch.no_grad()
def decode_attention(q, k_new, v_new, k_cache, v_cache, cos, sin, positions, *,
                     rows=None, lengths=None, max_len=None,
                     impl: Optional[str] = None,
                     k_scale=None, v_scale=None, block_table=None) -> torch.Tensor:
    """Fused RoPE + cache write + GQA decode attention (one kernel launch plus
    a small combine) for bf16 / head_dim 128 / H/Hkv in {1,2,4,8,16} on the
    GPU; ``decode_attention_ref`` otherwise.  ``positions`` is a long tensor
    [N] or an int (every row at that position).  ``max_len`` is a host bound
    on every position + 1 (default: the cache length); a tighter bound launches
    fewer workgroups.  ``impl`` names the kernel: ``"valu"`` (H/Hkv <= 8),
    ``"mfma"`` (H/Hkv 8 or 16; an error for any other group size) or None for
    the default of the group size (MFMA at 8 and 16, the vector-ALU kernel
    below; profiles/README.md, Round 12).
    The two differ in the last bits of o, never in what they write to the
    cache.
    The cache dtype picks the path.  ``float8_e4m3fn`` caches (opt-in) need
    ``k_scale`` / ``v_scale``, fp32 [slots,Hkv,Tmax]: one power-of-two scale
    per (slot, kv head, token), each row stored as the e4m3 of x / scale
    (``quantize_kv_rows_fp8``).  They have one MFMA kernel for all five group
    sizes, so ``impl`` must stay None.
    ``block_table`` (int32 [table_rows, max_pages]) makes the caches a paged
    pool [num_pages, page, Hkv, 128] (scales [num_pages, Hkv, page]): token t
    of table row ``rows[n]`` lives at ``cache[block_table[row, t // page],
    t % page]`` and ``lengths`` is [table_rows].  The same kernels serve
    page == 64, in every cache dtype and group size; ``max_len`` then defaults
    to ``max_pages * page``."""
    if impl not in _DECODE_IMPLS:
        raise ValueError(f"decode_attention: impl must be None, 'valu' or 'mfma', got {impl!r}")
    fp8 = _check_fp8_args("decode_attention", k_cache, v_cache, k_scale, v_scale)
    if fp8 and impl is not None:
        raise ValueError("decode_attention: impl names a bf16-cache kernel; an fp8 cache "
                         "takes impl=None")
    if block_table is not None:
        _check_block_table("decode_attention", block_table, k_cache)
    page = k_cache.shape[1] if block_table is not None else None
    if not decode_attention_hip_supported(q, k_new.shape[2], FP8_KV_DTYPE if fp8 else None,
                                          page):
        if impl is not None:
            raise ValueError(f"decode_attention: impl={impl!r} needs the gfx950 kernel, which "
                             "does not serve this device/dtype/geometry")
        return decode_attention_ref(q, k_new, v_new, k_cache, v_cache, cos, sin,
                                    positions, rows=rows, lengths=lengths, max_len=max_len,
                                    k_scale=k_scale, v_scale=v_scale, block_table=block_table)
    ext = extension()
    pos_t, upos = (None, positions) if isinstance(positions, int) else (positions, 0)
    if pos_t is not None and lengths is not None and _shares_storage(pos_t, lengths):
        # the kernel stores lengths[row] while other workgroups still read positions
        pos_t = pos_t.clone()
    if pos_t is not None:
        pos_t = pos_t.contiguous()
    if rows is not None:
        rows = rows.contiguous()
    if block_table is not None:
        block_table = block_table.contiguous()
    if max_len is None:
        max_len = min(_cache_tokens(k_cache, block_table), cos.shape[0])
    if fp8:
        return ext.attention_decode_fp8(q.contiguous(), k_new.contiguous(), v_new.contiguous(),
                                        k_cache, v_cache, k_scale, v_scale, cos, sin, pos_t,
                                        rows, lengths, upos, int(max_len), 0, block_table)
    return ext.attention_decode(q.contiguous(), k_new.contiguous(), v_new.contiguous(),
                                k_cache, v_cache, cos, sin, pos_t, rows, lengths,
                                upos, int(max_len), 0, _DECODE_IMPLS[impl], block_table)


# ---------------------------------------------------------------------------
# Multi-token extend over a KV cache with per-row positions: decode's contract
# with a time axis.
#
# Contract (both implementations): q [N,Sq,H,D], k_new/v_new [N,Sq,Hkv,D],
# caches, cos/sin and rows as for decode.  Batch row n has positions[n] tokens
# cached and q_lens[n] (default Sq) valid new tokens.  In place: token
# i < q_lens[n] is rotated at positions[n] + i and its k/v land at
# [row, positions[n] + i]; lengths[row] becomes positions[n] + q_lens[n].
# Returns o [N,Sq,H,D]: o[n, i] attends keys 0 .. positions[n] + i of its
# row; tokens i >= q_lens[n] write nothing and their output is zero.
# ---------------------------------------------------------------------------

def extend_attention_hip_supported(q: torch.Tensor, num_kv_heads: int,
                                   cache_dtype: Optional[torch.dtype] = None,
                                   page_size: Optional[int] = None) -> bool:
    """True when ``extend_attention`` runs the gfx950 kernels for a query of
    this device/dtype/geometry (else it runs the reference).  ``cache_dtype``
    and ``page_size`` as for ``decode_attention_hip_supported``."""
    if not use_hip(q):
        return False
    if page_size not in (None, PAGE_TOKENS):
        return False
    if cache_dtype not in (None, torch.bfloat16, FP8_KV_DTYPE):
        return False
    if q.dtype is not torch.bfloat16 or q.shape[-1] != 128:
        return False
    H = q.shape[-2]
    if num_kv_heads <= 0 or H % num_kv_heads or H // num_kv_heads not in _DECODE_REPS:
        return False
    name = "attention_extend_fp8" if cache_dtype is FP8_KV_DTYPE else "attention_extend"
    return hasattr(extension(), name)


@torch.no_grad()
def extend_attention_ref(q, k_new, v_new, k_cache, v_cache, cos, sin, positions, *,
                         q_lens=None, rows=None, lengths=None, max_len=None,
                         k_scale=None, v_scale=None, block_table=None) -> torch.Tensor:
    """Plain per-row fp32 composition: rotate token i at p + i (the
    apply_rope_positions formula), round to the cache dtype, write, softmax
    over keys 0 .. p + i.  The CPU path and the oracle of the kernel;
    ``max_len`` is unused.  fp8 caches and ``block_table`` as in
    ``decode_attention_ref``."""
    from .rope import apply_rope_positions

    _check_fp8_args("extend_attention_ref", k_cache, v_cache, k_scale, v_scale)

    N, Sq, H, D = q.shape
    rep = H // k_new.shape[2]
    pos = _positions_tensor(positions, N, q.device).tolist()
    lens = q_lens.tolist() if q_lens is not None else [Sq] * N
    row_l = rows.tolist() if rows is not None else list(range(N))
    if block_table is not None:
        _check_block_table("extend_attention_ref", block_table, k_cache)
        ks, kss = _gather_pages(k_cache, k_scale, block_table)
        vs, vss = _gather_pages(v_cache, v_scale, block_table)
        o = extend_attention_ref(q, k_new, v_new, ks, vs, cos, sin, positions, q_lens=q_lens,
                                 rows=rows, lengths=lengths, k_scale=kss, v_scale=vss)
        for r, p, ln in zip(row_l, pos, lens):
            _scatter_pages(k_cache, k_scale, ks, kss, block_table, r, p, p + ln)
            _scatter_pages(v_cache, v_scale, vs, vss, block_table, r, p, p + ln)
        return o
    scale = 1.0 / (D ** 0.5)
    o = torch.zeros_like(q)
    for n, (r, p, ln) in enumerate(zip(row_l, pos, lens)):
        at = torch.arange(p, p + ln, device=q.device)
        # the ln tokens of the row as a batch of single-token rows
        qr = apply_rope_positions(q[n, :ln].unsqueeze(1), cos, sin, at)[:, 0]
        kr = apply_rope_positions(k_new[n, :ln].unsqueeze(1), cos, sin, at)[:, 0]
        _cache_store(k_cache, k_scale, r, slice(p, p + ln), kr)
        _cache_store(v_cache, v_scale, r, slice(p, p + ln), v_new[n, :ln])
        if lengths is not None:
            lengths[r] = p + ln
        kk = _cache_prefix(k_cache, k_scale, r, p + ln).repeat_interleave(rep, dim=1)  # [T,H,D]
        vv = _cache_prefix(v_cache, v_scale, r, p + ln).repeat_interleave(rep, dim=1)
        s = torch.einsum("ihd,thd->hit", qr.float(), kk) * scale
        hidden = torch.arange(p + ln, device=q.device)[None, :] > at[:, None]  # [ln,T]
        s = s.masked_fill(hidden[None], float("-inf"))
        o[n, :ln] = torch.einsum("hit,thd->ihd", torch.softmax(s, dim=-1), vv).to(q.dtype)
    return o


@torch.no_grad()
def extend_attention(q, k_new, v_new, k_cache, v_cache, cos, sin, positions, *,
                     q_lens=None, rows=None, lengths=None, max_len=None,
                     chunk: int = 0, split: Optional[bool] = None,
                     k_scale=None, v_scale=None, block_table=None) -> torch.Tensor:
    """Fused RoPE + cache write + GQA attention of Sq new tokens per row over
    the slot cache (an append launch, an MFMA attention launch and, on the
    split path, a combine) for bf16 / head_dim 128 / H/Hkv in {1,2,4,8} on the
    GPU; ``extend_attention_ref`` otherwise.  ``positions`` is a long tensor
    [N] or an int (every row has that many tokens cached).  ``max_len`` is a
    host bound on every position + q_len (default: the cache length).
    ``chunk`` and ``split`` reach the kernel only: a key-chunk size from its
    fixed set, and the split (True) or direct (False) path instead of the
    choice by ``Sq * H/Hkv``.  ``float8_e4m3fn`` caches with ``k_scale`` /
    ``v_scale`` as for ``decode_attention``: the append quantises, the
    attention kernel dequantises on its way into LDS.  ``block_table`` as for
    ``decode_attention``: a 64-token page is one key tile of the kernel, and a
    chunk that crosses a page boundary is appended to both pages."""
    fp8 = _check_fp8_args("extend_attention", k_cache, v_cache, k_scale, v_scale)
    if block_table is not None:
        _check_block_table("extend_attention", block_table, k_cache)
    page = k_cache.shape[1] if block_table is not None else None
    if not extend_attention_hip_supported(q, k_new.shape[2], FP8_KV_DTYPE if fp8 else None,
                                          page):
        return extend_attention_ref(q, k_new, v_new, k_cache, v_cache, cos, sin, positions,
                                    q_lens=q_lens, rows=rows, lengths=lengths,
                                    max_len=max_len, k_scale=k_scale, v_scale=v_scale,
                                    block_table=block_table)
    ext = extension()
    pos_t, upos = (None, positions) if isinstance(positions, int) else (positions, 0)
    if lengths is not None:
        # the append stores lengths[row]; the later launches still read the metadata
        pos_t, q_lens, rows = (t.clone() if t is not None and _shares_storage(t, lengths)
                               else t for t in (pos_t, q_lens, rows))
    pos_t, q_lens, rows = (t.contiguous() if t is not None else None
                           for t in (pos_t, q_lens, rows))
    if block_table is not None:
        block_table = block_table.contiguous()
    if max_len is None:
        max_len = min(_cache_tokens(k_cache, block_table), cos.shape[0])
    if fp8:
        return ext.attention_extend_fp8(q.contiguous(), k_new.contiguous(), v_new.contiguous(),
                                        k_cache, v_cache, k_scale, v_scale, cos, sin, pos_t,
                                        q_lens, rows, lengths, upos, int(max_len), int(chunk),
                                        -1 if split is None else int(bool(split)), block_table)
    return ext.attention_extend(q.contiguous(), k_new.contiguous(), v_new.contiguous(),
                                k_cache, v_cache, cos, sin, pos_t, q_lens, rows, lengths,
                                upos, int(max_len), int(chunk),
                                -1 if split is None else int(bool(split)), block_table)
