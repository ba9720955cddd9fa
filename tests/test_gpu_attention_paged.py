"""Decode and extend attention over the paged KV cache (attn_paged.h), every
kernel family: a slot cache is scattered into a pool under a non-monotone block
table (pages of the rows interleaved, spare pages holding a sentinel) and the
paged call runs next to the slot call on the same inputs.

(a) Paging changes addresses only, never the arithmetic or a merge order: o,
    the cache gathered back (appended tokens, fp8 bytes, scales) and lengths
    are bit-identical to the slot path's, and the spare pages are untouched.
(b) o against fp32 attention over the (dequantised) cache as the call left it,
    under the slot-path tests' bound (test_gpu_attention_decode.py,
    test_gpu_attention_extend.py): err <= 2 * err_eager + ulp(max|ref|) and
    err < 3e-2, err_eager being bf16 SDPA over the same cache.
"""

import pytest
import torch

from tests.test_attention_paged_cpu import scatter_into_pages

pytestmark = pytest.mark.gpu

D, SLOTS, PAGE, DEV = 128, 4, 64, "cuda"


def _bf16_ulp(x):
    _, e = torch.frexp(x.float())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 8)


def _run(H, Hkv, fp8, Sq, rows, positions, lens, T, **kw):
    from lpp_amd import ops

    N, rep = len(rows), H // Hkv
    g = torch.Generator(device=DEV).manual_seed(H + Sq + positions[1])
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    q, k_new, v_new = (rn(N, Sq, h, D).bfloat16() for h in (H, Hkv, Hkv))
    cos, sin = ops.build_rope_cache(T, D, 10000.0, torch.device(DEV))
    pos, rows, lens_t = (torch.tensor(x, device=DEV) for x in (positions, rows, lens))
    slot = [rn(SLOTS, T, Hkv, D).bfloat16(), rn(SLOTS, T, Hkv, D).bfloat16()]
    if fp8:
        (k, ks), (v, vs) = (ops.quantize_kv_rows_fp8(x) for x in slot)
        slot = [k, v, ks.transpose(1, 2).contiguous(), vs.transpose(1, 2).contiguous()]
    pools, table, gather = scatter_into_pages(slot, PAGE)
    before = [p.clone() for p in pools]
    fn, extra = ((ops.decode_attention, {}) if Sq == 1 and not kw else
                 (ops.extend_attention, dict(q_lens=lens_t, **kw)))
    outs = []
    for c, tab in ((slot, {}), (pools, dict(block_table=table))):
        ln = torch.arange(11, 11 + SLOTS, device=DEV)
        sc = dict(k_scale=c[2], v_scale=c[3]) if fp8 else {}
        outs.append((fn(q, k_new, v_new, c[0], c[1], cos, sin, pos, rows=rows, lengths=ln,
                        max_len=max(p + l for p, l in zip(positions, lens)),
                        **extra, **sc, **tab), ln))
    (o_slot, ln_slot), (o, ln) = outs
    torch.cuda.synchronize()

    # (a) bit-identical to the slot path; spare pages untouched
    assert torch.equal(o.view(torch.int16), o_slot.view(torch.int16))
    assert torch.equal(ln, ln_slot)
    back = gather(pools)
    for got, want in zip(back, slot):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    owned = torch.zeros(pools[0].shape[0], dtype=torch.bool, device=DEV)
    owned[table.long().flatten()] = True
    for p, b in zip(pools, before):
        assert torch.equal(p.view(torch.uint8)[~owned], b.view(torch.uint8)[~owned])

    # (b) fp32 attention over the cache the paged call left, gathered back
    kd, vd = back[0].float(), back[1].float()
    if fp8:
        kd, vd = kd * back[2].transpose(1, 2)[..., None], vd * back[3].transpose(1, 2)[..., None]
    at = pos[:, None] + torch.arange(Sq, device=DEV)                       # [N,Sq]
    q_rot = ops.apply_rope_positions(q.view(N * Sq, 1, H, D), cos, sin,
                                     at.view(-1).clamp(max=T - 1)).view_as(q)
    kt = kd[rows].transpose(1, 2).repeat_interleave(rep, dim=1)            # [N,H,T,D]
    vt = vd[rows].transpose(1, 2).repeat_interleave(rep, dim=1)
    mask = (torch.arange(T, device=DEV)[None, None, :] <= at[:, :, None])[:, None]
    qt = q_rot.transpose(1, 2)
    s = qt.float() @ kt.transpose(2, 3) / D ** 0.5
    ref = (torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ vt).transpose(1, 2)
    eager = torch.nn.functional.scaled_dot_product_attention(
        qt, kt.bfloat16(), vt.bfloat16(), attn_mask=mask).transpose(1, 2)
    valid = torch.arange(Sq, device=DEV)[None, :] < lens_t[:, None]
    assert not o[~valid].float().any()
    err = float((o.float() - ref)[valid].abs().max())
    err_eager = float((eager.float() - ref)[valid].abs().max())
    ulp = float(_bf16_ulp(ref[valid].abs().max()))
    print(f"\npaged H={H} Hkv={Hkv} fp8={fp8} Sq={Sq} {kw}: kernel err {err:.3e}  "
          f"eager err {err_eager:.3e}  ulp {ulp:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err < 3e-2
    assert err <= 2 * err_eager + ulp


@pytest.mark.parametrize("first", [(0, 64), (63, 65)])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (16, 2), (32, 2)])   # vector ALU (bf16), MFMA 8, 16
def test_decode_paged(H, Hkv, fp8, first):
    """p at a page's first and last key and either side of it, and one row of
    the same batch whose keys span two chunks (and five pages)."""
    from lpp_amd import ops

    C = int(ops.extension().attention_decode_chunk())
    _run(H, Hkv, fp8, 1, [2, 0, 3], [*first, C + 1], [1, 1, 1], C + PAGE)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (16, 2)])
def test_extend_paged(H, Hkv, fp8, split):
    """A chunk from key 0, one that starts mid-page and crosses the boundary
    (40 + 24 ends on it, 100 + 64 crosses 128) and a token exactly on a page."""
    _run(H, Hkv, fp8, 64, [2, 0, 3, 1], [0, 40, 64, 100], [33, 24, 1, 64], 3 * PAGE,
         split=split, **(dict(chunk=64) if split else {}))
