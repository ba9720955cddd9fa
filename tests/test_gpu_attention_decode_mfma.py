"""MFMA decode attention (attention_decode_mfma.hip) for GQA groups of 8 and 16.

The cache is poisoned as in test_gpu_attention_decode.py: the valid prefix of a
row is random, every position at or past the row's own - and all of every
unused slot - holds k = 4 * rotated q (a score of about 45) and v = 100, and
every row carries one needle key (k = 2 * rotated q) whose value the group's
first head must return.  Positions cover the 16- and 32-key tile edges, the
wave edge C/4 and the chunk edge C of the kernel.

Measured on MI355X (C = 256), printed by test_reference_needles_side_effects
and recorded in profiles/README.md, Round 12: kernel max error 5.0e-3 to
9.1e-3, equal to the eager bf16 path's in every case (max |ref| 3.3 to 3.9);
needle deviation 0 on every row.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
SLOTS = 9


def _chunk():
    from lpp_amd import ops

    return int(ops.extension().attention_decode_chunk())


def _rows(name):
    """(cache slots, positions, needle positions) of a row set."""
    C = _chunk()
    if name == "a":
        return ([4, 1, 7, 0, 3, 8, 5],
                [0, 15, 17, 32, C // 4 - 1, C - 1, C + 1],
                [0, 0, 16, 31, 32, C - 1, C])
    return ([2, 0, 3, 6, 8, 5, 1],
            [1, 16, 31, 33, C // 4, C, 2 * C + 44],
            [0, 16, 15, 32, C // 4 - 1, 16, 2 * C + 32])


def _bf16_ulp(x):
    _, e = torch.frexp(x.float())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 8)


@functools.lru_cache(maxsize=None)
def _case(H, Hkv, name):
    """Inputs, the poisoned cache, the float64 reference and the eager bf16
    result of one case; built once, never modified (the calls clone)."""
    from lpp_amd import ops

    rows, positions, needles = _rows(name)
    Tmax, rep, N, dev = 2 * _chunk() + 64, H // Hkv, len(rows), "cuda"
    g = torch.Generator(device=dev).manual_seed(H + len(name))
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    head0 = torch.arange(Hkv, device=dev) * rep
    q = rn(N, 1, H, D)
    q[:, :, head0] *= D ** 0.5 / q[:, :, head0].norm(dim=-1, keepdim=True)  # |q|^2 = D
    q = q.bfloat16()
    k_new = rn(N, 1, Hkv, D).bfloat16()
    v_new = rn(N, 1, Hkv, D).clamp(-3.9, 3.9).bfloat16()
    cos, sin = ops.build_rope_cache(Tmax, D, 10000.0, torch.device(dev))
    pos, row_t = torch.tensor(positions, device=dev), torch.tensor(rows, device=dev)
    for n in range(N):
        if needles[n] == positions[n]:                 # needle at p: through k_new
            k_new[n, 0] = 2 * q[n, 0, head0]
    q_rot = ops.apply_rope_positions(q, cos, sin, pos)
    k_cache = rn(SLOTS, Tmax, Hkv, D).bfloat16()
    v_cache = rn(SLOTS, Tmax, Hkv, D).clamp(-3.9, 3.9).bfloat16()
    for r in set(range(SLOTS)) - set(rows):
        k_cache[r], v_cache[r] = 4 * q_rot[0, 0, head0], 100.0
    for n, (r, p, ns) in enumerate(zip(rows, positions, needles)):
        k_cache[r, p:], v_cache[r, p:] = 4 * q_rot[n, 0, head0], 100.0
        if ns < p:
            k_cache[r, ns] = 2 * q_rot[n, 0, head0]
    # the cache after the eager write, float64 attention and eager bf16 SDPA over it
    k, v = k_cache.clone(), v_cache.clone()
    k[row_t, pos] = ops.apply_rope_positions(k_new, cos, sin, pos)[:, 0]
    v[row_t, pos] = v_new[:, 0]
    T = max(positions) + 1
    kt = k[row_t, :T].transpose(1, 2).repeat_interleave(rep, dim=1)    # [N,H,T,D]
    vt = v[row_t, :T].transpose(1, 2).repeat_interleave(rep, dim=1)
    mask = (torch.arange(T, device=dev)[None, :] <= pos[:, None])[:, None, None, :]
    s = q_rot.transpose(1, 2).double() @ kt.double().transpose(2, 3) / D ** 0.5
    ref = (torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ vt.double()).transpose(1, 2)
    eager = torch.nn.functional.scaled_dot_product_attention(
        q_rot.transpose(1, 2), kt, vt, attn_mask=mask).transpose(1, 2)
    return dict(q=q, k_new=k_new, v_new=v_new, k_cache=k_cache, v_cache=v_cache, cos=cos,
                sin=sin, pos=pos, rows=row_t, lengths=torch.arange(11, 11 + SLOTS, device=dev),
                head0=head0, ref=ref, k_after=k, Tmax=Tmax,
                err_eager=float((eager.double() - ref).abs().max()))


def _kernel(c, impl, sel=None, max_len=None):
    """One call on clones of the case's cache -> (o, k, v, lengths)."""
    from lpp_amd import ops

    sel = slice(None) if sel is None else sel
    k, v, ln = c["k_cache"].clone(), c["v_cache"].clone(), c["lengths"].clone()
    o = ops.decode_attention(c["q"][sel].contiguous(), c["k_new"][sel].contiguous(),
                             c["v_new"][sel].contiguous(), k, v, c["cos"], c["sin"],
                             c["pos"][sel].contiguous(), rows=c["rows"][sel].contiguous(),
                             lengths=ln, max_len=max_len, impl=impl)
    return o, k, v, ln


def _check_output(c, o, tag):
    ref = c["ref"]
    err, top = float((o.double() - ref).abs().max()), ref.abs().max()
    ulp = float(_bf16_ulp(top))
    print(f"\n{tag}: kernel err {err:.3e}  eager err {c['err_eager']:.3e}  "
          f"max|ref| {float(top):.3f}  ulp {ulp:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err < 3e-2
    assert err <= 2 * c["err_eager"] + ulp


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("H,Hkv", [(16, 2), (32, 2)])
def test_reference_needles_side_effects(H, Hkv, name):
    c = _case(H, Hkv, name)
    rows, positions, needles = _rows(name)
    o, k, v, ln = _kernel(c, "mfma", max_len=max(positions) + 1)
    _check_output(c, o, f"decode mfma H={H} Hkv={Hkv} rows={name}")
    for n, (r, p, ns) in enumerate(zip(rows, positions, needles)):
        want = (c["v_new"][n, 0] if ns == p else c["v_cache"][r, ns]).float()   # [Hkv, D]
        dev_k = float((o[n, 0, c["head0"]].float() - want).abs().max())
        print(f"  needle row {n} p={p} p*={ns}: |o - v[p*]| {dev_k:.3e}")
        assert float((c["ref"][n, 0, c["head0"]] - want).abs().max()) < 1e-4
        assert dev_k <= 2e-2
    pos, row_t = c["pos"], c["rows"]
    assert torch.equal(v[row_t, pos].view(torch.int16), c["v_new"][:, 0].view(torch.int16))
    k_want = c["k_after"][row_t, pos].float()
    assert bool(((k[row_t, pos].float() - k_want).abs() <= _bf16_ulp(k_want)).all())
    untouched = torch.ones(SLOTS, c["Tmax"], dtype=torch.bool, device="cuda")
    untouched[row_t, pos] = False
    for new, old in ((k, c["k_cache"]), (v, c["v_cache"])):
        assert torch.equal(new[untouched].view(torch.int16), old[untouched].view(torch.int16))
    want_len = c["lengths"].clone()
    want_len[row_t] = pos + 1
    assert torch.equal(ln, want_len)


@pytest.mark.parametrize("name", ["a", "b"])
def test_same_token_same_cache_bits_as_valu(name):
    c = _case(16, 2, name)
    om, km, vm, lm = _kernel(c, "mfma")
    ov, kv, vv, lv = _kernel(c, "valu")
    assert torch.equal(km.view(torch.int16), kv.view(torch.int16))
    assert torch.equal(vm.view(torch.int16), vv.view(torch.int16))
    assert torch.equal(lm, lv)
    _check_output(c, om, f"rep 8 rows={name} mfma")
    _check_output(c, ov, f"rep 8 rows={name} valu")


def test_batch_invariance():
    c = _case(32, 2, "b")
    N = len(_rows("b")[0])
    o, _, _, _ = _kernel(c, None, max_len=max(_rows("b")[1]) + 1)
    rev = torch.arange(N - 1, -1, -1, device="cuda")
    o_rev, _, _, _ = _kernel(c, None, sel=rev)          # reversed, max_len = the cache length
    assert torch.equal(o_rev.view(torch.int16), o[rev].view(torch.int16))
    for n in range(N):
        o1, _, _, _ = _kernel(c, None, sel=slice(n, n + 1), max_len=_rows("b")[1][n] + 1)
        assert torch.equal(o1[0].view(torch.int16), o[n].view(torch.int16)), n


def test_dispatch(monkeypatch):
    from lpp_amd import ops
    from lpp_amd.config import model_config
    from lpp_amd.models.llama import GatherKVCache, LlamaAttention, RaggedKVCache

    q = torch.zeros(3, 1, 32, D, device="cuda", dtype=torch.bfloat16)
    assert ops.decode_attention_hip_supported(q, 2)
    c = _case(16, 2, "a")
    with pytest.raises(RuntimeError, match="MFMA"):
        ops.decode_attention(c["q"], c["k_new"].repeat(1, 1, 2, 1), c["v_new"].repeat(1, 1, 2, 1),
                             c["k_cache"].repeat(1, 1, 2, 1), c["v_cache"].repeat(1, 1, 2, 1),
                             c["cos"], c["sin"], c["pos"], rows=c["rows"], impl="mfma")  # rep 4

    real, calls = ops.extension(), []

    class Counting:
        def __getattr__(self, attr):
            return getattr(real, attr)

        def attention_decode(self, *a, **kw):
            calls.append(1)
            return real.attention_decode(*a, **kw)

    monkeypatch.setattr(ops, "_EXT", Counting())
    cfg = model_config("llama-tiny", hidden_size=32 * D, intermediate_size=1024, num_heads=32,
                       num_kv_heads=2, num_layers=1, max_seq_len=128)
    attn = LlamaAttention(cfg).to("cuda", torch.bfloat16)
    with torch.no_grad():
        for w in attn.parameters():
            w.normal_(0.0, 0.02)
    cache = RaggedKVCache(4, 64, cfg.kv_heads, cfg.head_dim, "cuda", torch.bfloat16)
    slot_t = torch.tensor([3, 1], device="cuda")
    cache.lengths[slot_t] = torch.tensor([17, 40], device="cuda")
    with torch.no_grad():
        y = attn(torch.randn(2, 1, cfg.hidden_size, device="cuda").bfloat16(),
                 cache=GatherKVCache(cache, slot_t, total_hint=41))
    assert calls == [1] and torch.isfinite(y.float()).all()
    assert cache.lengths.tolist() == [0, 41, 0, 18]
