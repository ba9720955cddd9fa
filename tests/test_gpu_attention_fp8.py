"""Decode and extend attention over the FP8 (e4m3) KV cache: attention_decode_fp8.hip
and the fp8 instantiations of attention_extend.hip.

The valid prefix of a row is random bf16 rows quantised by the torch rule; every
position at or past the row's own, and all of every unused slot, holds bytes of
+-448 under scales of 2^10, so a stale read shows.  The reference is float64
attention over the dequantised cache as the call left it, and the criterion the
project's own: err <= 2 * err_eager + ulp(max|ref|) and err < 3e-2, err_eager
being bf16 SDPA over that same dequantised cache (which is exact in bf16).
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

D, SLOTS, DEV = 128, 9, "cuda"
FP8 = torch.float8_e4m3fn


def _bf16_ulp(x):
    _, e = torch.frexp(x.float())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 8)


def _case(H, Hkv, Sq, rows, positions, lens, needles, Tmax, seed, dev=DEV):
    """Inputs and the poisoned fp8 cache.  needles[n] is a key position < p (in
    the cache), p itself (through k_new's first token) or None."""
    from lpp_amd import ops

    N, rep = len(rows), H // Hkv
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    head0 = torch.arange(Hkv, device=dev) * rep
    q = rn(N, Sq, H, D)
    q[:, :, head0] *= D ** 0.5 / q[:, :, head0].norm(dim=-1, keepdim=True)    # |q|^2 = D
    q, k_new, v_new = q.bfloat16(), rn(N, Sq, Hkv, D).bfloat16(), rn(N, Sq, Hkv, D).bfloat16()
    cos, sin = ops.build_rope_cache(Tmax, D, 10000.0, torch.device(dev))
    pos, row_t = torch.tensor(positions, device=dev), torch.tensor(rows, device=dev)
    at = (pos[:, None] + torch.arange(Sq, device=dev)).clamp(max=Tmax - 1)    # [N,Sq]
    q_rot = ops.apply_rope_positions(q.view(N * Sq, 1, H, D), cos, sin, at.view(-1)).view_as(q)
    k, ks = ops.quantize_kv_rows_fp8(rn(SLOTS, Tmax, Hkv, D).bfloat16())
    v, vs = ops.quantize_kv_rows_fp8(rn(SLOTS, Tmax, Hkv, D).bfloat16())
    ks, vs = ks.transpose(1, 2).contiguous(), vs.transpose(1, 2).contiguous()
    poison = torch.where(torch.arange(D, device=dev) % 2 == 0, 448.0, -448.0).to(FP8)
    fill = torch.ones(SLOTS, Tmax, dtype=torch.bool, device=dev)
    for n, (r, p, ns) in enumerate(zip(rows, positions, needles)):
        fill[r, :p] = False
        if ns == p:
            k_new[n, 0] = 2 * q[n, 0, head0]
        elif ns is not None:
            k[r, ns], ks[r, :, ns] = ops.quantize_kv_rows_fp8(2 * q_rot[n, 0, head0])
    k.view(torch.uint8)[fill] = v.view(torch.uint8)[fill] = poison.view(torch.uint8)
    ks.transpose(1, 2)[fill], vs.transpose(1, 2)[fill] = 1024.0, 1024.0
    return dict(q=q, k_new=k_new, v_new=v_new, k=k, v=v, ks=ks, vs=vs, cos=cos, sin=sin,
                pos=pos, rows=row_t, lens=torch.tensor(lens, device=dev), q_rot=q_rot,
                lengths=torch.arange(11, 11 + SLOTS, device=dev), head0=head0, at=at,
                needles=needles)


def _call(c, sel=None, **kw):
    """One call on clones of the case's cache -> (o, k, v, ks, vs, lengths)."""
    from lpp_amd import ops

    sel = slice(None) if sel is None else sel
    k, v, ks, vs, ln = (c[n].clone() for n in ("k", "v", "ks", "vs", "lengths"))
    a = [c[n][sel].contiguous() for n in ("q", "k_new", "v_new")]
    common = dict(rows=c["rows"][sel].contiguous(), lengths=ln, k_scale=ks, v_scale=vs, **kw)
    if c["q"].shape[1] == 1 and "split" not in kw:
        o = ops.decode_attention(*a, k, v, c["cos"], c["sin"], c["pos"][sel].contiguous(), **common)
    else:
        o = ops.extend_attention(*a, k, v, c["cos"], c["sin"], c["pos"][sel].contiguous(),
                                 q_lens=c["lens"][sel].contiguous(), **common)
    return o, k, v, ks, vs, ln


def _dequant(x, s):
    return x.float() * s.transpose(1, 2)[..., None]        # exact in bf16


def _check_output(c, o, k, v, ks, vs, tag):
    """o against float64 attention over the dequantised cache (k, v, ks, vs)."""
    N, Sq, H, _ = o.shape
    rep, T = H // k.shape[2], int((c["pos"] + c["lens"]).max())
    kt = _dequant(k, ks)[c["rows"], :T].transpose(1, 2).repeat_interleave(rep, dim=1)  # [N,H,T,D]
    vt = _dequant(v, vs)[c["rows"], :T].transpose(1, 2).repeat_interleave(rep, dim=1)
    mask = (torch.arange(T, device=o.device)[None, None, :] <= c["at"][:, :, None])[:, None]
    qt = c["q_rot"].transpose(1, 2)
    s = qt.double() @ kt.double().transpose(2, 3) / D ** 0.5
    ref = (torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ vt.double()).transpose(1, 2)
    eager = torch.nn.functional.scaled_dot_product_attention(
        qt, kt.bfloat16(), vt.bfloat16(), attn_mask=mask).transpose(1, 2)
    valid = torch.arange(Sq, device=o.device)[None, :] < c["lens"][:, None]
    assert not o[~valid].float().any()              # tokens past q_len: zero, else ignored
    err = float((o.double() - ref)[valid].abs().max())
    err_eager = float((eager.double() - ref)[valid].abs().max())
    top = ref[valid].abs().max()
    print(f"\n{tag}: kernel err {err:.3e}  eager err {err_eager:.3e}  max|ref| {float(top):.3f}")
    assert torch.isfinite(o.float()).all()
    assert err < 3e-2
    assert err <= 2 * err_eager + float(_bf16_ulp(top))
    return ref


def _check_written(c, k, v, ks, vs, ln):
    """The appended entries obey the format; nothing else moved."""
    from lpp_amd import ops

    written = torch.zeros(SLOTS, k.shape[1], dtype=torch.bool, device=k.device)
    want_len = c["lengths"].clone()
    for n, (r, p, l) in enumerate(zip(c["rows"].tolist(), c["pos"].tolist(), c["lens"].tolist())):
        written[r, p : p + l] = True
        want_len[r] = p + l
        vb, vsc = ops.quantize_kv_rows_fp8(c["v_new"][n, :l])           # V: the torch bits
        assert torch.equal(v[r, p : p + l].view(torch.uint8), vb.view(torch.uint8))
        assert torch.equal(vs[r, :, p : p + l], vsc.T)
        # K: the kernels' rotation is within one bf16 ulp of torch's, so the
        # scale is the rule's for an amax within one ulp, and byte * scale is
        # within that ulp plus half an e4m3 step (16 scales at most)
        k_want = ops.apply_rope_positions(c["k_new"][n, :l].unsqueeze(1), c["cos"], c["sin"],
                                          c["at"][n, :l])[:, 0].float()
        amax = k_want.abs().amax(-1)
        near = torch.stack([amax - _bf16_ulp(amax), amax, amax + _bf16_ulp(amax)], -1)
        ok_scale = ops.quantize_kv_rows_fp8(near[..., None])[1]          # [l,Hkv,3]
        sc = ks[r, :, p : p + l].T                                       # [l,Hkv]
        assert bool((sc[..., None] == ok_scale).any(-1).all())
        got = k[r, p : p + l].float() * sc[..., None]
        assert bool(((got - k_want).abs() <= _bf16_ulp(k_want) + 16 * sc[..., None]).all())
    for new, old in ((k, c["k"]), (v, c["v"])):
        assert torch.equal(new.view(torch.uint8)[~written], old.view(torch.uint8)[~written])
    for new, old in ((ks, c["ks"]), (vs, c["vs"])):
        assert torch.equal(new.transpose(1, 2)[~written], old.transpose(1, 2)[~written])
    assert torch.equal(ln, want_len)


@functools.lru_cache(maxsize=None)
def _decode_case(H, Hkv, name):
    """Positions at the edges of a 16-key tile, a 32-key step, a wave's quarter
    chunk and the chunk; one needle per row, at p itself in some."""
    from lpp_amd import ops

    C = int(ops.extension().attention_decode_chunk())
    if name == "a":
        rows, positions = [4, 1, 7, 0, 3, 8, 5], [0, 15, 17, 32, C // 4 - 1, C - 1, C + 1]
        needles = [0, 0, 16, 31, 32, C - 1, C]
    else:
        rows, positions = [2, 0, 3, 6, 8, 5, 1], [1, 16, 31, 33, C // 4, C, 2 * C + 44]
        needles = [0, 16, 15, 32, C // 4 - 1, 16, 2 * C + 32]
    return _case(H, Hkv, 1, rows, positions, [1] * 7, needles, 2 * C + 64, seed=H + len(name))


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (8, 2), (16, 2), (32, 2)])
def test_decode_reference_needles_side_effects(H, Hkv, name):
    c = _decode_case(H, Hkv, name)
    o, k, v, ks, vs, ln = _call(c, max_len=int(c["pos"].max()) + 1)
    ref = _check_output(c, o, k, v, ks, vs, f"decode fp8 H={H} Hkv={Hkv} rows={name}")
    _check_written(c, k, v, ks, vs, ln)
    vd = _dequant(v, vs)
    for n, (r, ns) in enumerate(zip(c["rows"].tolist(), c["needles"])):
        want = vd[r, ns]                    # the needle's V row as cached, [Hkv,D]
        assert float((ref[n, 0, c["head0"]] - want).abs().max()) < 1e-4
        assert float((o[n, 0, c["head0"]].float() - want).abs().max()) <= 2e-2


def test_decode_row_alone_equals_row_in_batch():
    c = _decode_case(32, 2, "b")
    o = _call(c, max_len=int(c["pos"].max()) + 1)[0]
    for n in range(7):
        o1 = _call(c, sel=slice(n, n + 1), max_len=int(c["pos"][n]) + 1)[0]
        assert torch.equal(o1[0].view(torch.int16), o[n].view(torch.int16)), n
    rev = torch.arange(6, -1, -1, device=DEV)
    assert torch.equal(_call(c, sel=rev)[0].view(torch.int16), o[rev].view(torch.int16))


@functools.lru_cache(maxsize=None)
def _extend_case(H, Hkv, Sq):
    """Positions 0, 63, 64 and one that carries the row across a chunk boundary."""
    from lpp_amd import ops

    C = int(ops.extension().attention_extend_chunk())
    return _case(H, Hkv, Sq, [5, 0, 7, 2], [0, 63, 64, C - 3], [Sq, 1, 7, Sq - 2],
                 [None] * 4, C + 64 + Sq, seed=Sq)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("H,Hkv,Sq", [(2, 2, 33), (16, 2, 36), (2, 2, 288)])
def test_extend_reference_side_effects_then_decode(H, Hkv, Sq, split):
    """Sq * H/Hkv = 33 crosses a wave, 288 (at both group sizes) a 256-row
    block.  The tokens extend appended are then read by decode."""
    c = _extend_case(H, Hkv, Sq)
    o, k, v, ks, vs, ln = _call(c, split=split, max_len=int((c["pos"] + c["lens"]).max()))
    _check_output(c, o, k, v, ks, vs, f"extend fp8 H={H} Hkv={Hkv} Sq={Sq} split={split}")
    _check_written(c, k, v, ks, vs, ln)
    if split:
        return
    pos = c["pos"] + c["lens"]
    d = dict(c, q=c["q"][:, :1].contiguous(), k_new=c["k_new"][:, :1].contiguous(),
             v_new=c["v_new"][:, :1].contiguous(), k=k, v=v, ks=ks, vs=vs, pos=pos,
             lens=torch.ones_like(pos), at=pos[:, None])
    from lpp_amd import ops

    d["q_rot"] = ops.apply_rope_positions(d["q"], c["cos"], c["sin"], pos)
    o, k, v, ks, vs, ln = _call(d)
    _check_output(d, o, k, v, ks, vs, f"decode after extend H={H} Hkv={Hkv} Sq={Sq}")
