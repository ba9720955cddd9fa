"""Extend attention (attention_extend.hip) on the GPU: Sq new tokens per row
at per-row positions over the slot cache, on the split and on the direct path.

The cache is built as in test_gpu_attention_decode.py: the valid prefix of a
row is random, everything at or past p + len - and all of every unused row -
is poison (k = 4 * a rotated q, v = 100), and so is the padded tail of k_new
and v_new.  A read past a row's bound, or a query that sees a later token of
its own chunk, moves the output by order 1.

Measured on MI355X (printed by test_reference_and_side_effects, recorded in
profiles/README.md, Round 11): kernel max error 6.5e-3 to 8.6e-3, equal to the
eager bf16 sequence's in every case and between the two paths (both at the
rounding of the bf16 output; max |ref| 2.8 to 3.5).
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
SLOTS = 5
GEOMS = [(4, 4), (8, 2), (16, 2)]
SQS = [1, 5, 33, 160]
# rows of one kv head: Sq * rep.  33 crosses a wave (32 rows) at every rep, 160
# a workgroup (256 rows) at rep 4 and 8; 272 gives rep 1 a second row block,
# with one row (q_len 137) that ends inside the first
CASES = [(H, Hkv, Sq) for H, Hkv in GEOMS for Sq in SQS] + [(4, 4, 272)]
ROWS = [4, 1, 2, 0, 3]


def _ops():
    from lpp_amd import ops

    return ops


def _chunk():
    return int(_ops().extension().attention_extend_chunk(64))   # the smallest override


def _bf16_ulp(x):
    _, e = torch.frexp(x.float())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 8)


def _rope_tokens(x, cos, sin, pos, lens):
    """x [N,Sq,h,D] rotated at pos[n] + i for i < lens[n] (bf16), zero beyond."""
    out = torch.zeros_like(x)
    for n, (p, ln) in enumerate(zip(pos, lens)):
        at = torch.arange(p, p + ln, device=x.device)
        out[n, :ln] = _ops().apply_rope_positions(x[n, :ln].unsqueeze(1), cos, sin, at)[:, 0]
    return out


@functools.lru_cache(maxsize=None)
def _case(H, Hkv, Sq, seed=0):
    """Inputs, the poisoned cache, the eager bf16 result and the fp32
    reference of one case; shared by the tests and never modified."""
    ops, C, dev = _ops(), _chunk(), "cuda"
    # every p of {0, 1, 63, 64, C-1, C, 2C+44} (C = 64: five distinct values)
    pos = [C, 0, 2 * C + 44, C - 1, 1]
    lens = [Sq, 1, Sq, Sq // 2 + 1, Sq]
    Tmax = 2 * C + 44 + Sq + 20
    rep, N = H // Hkv, len(ROWS)
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    q = rn(N, Sq, H, D)
    head0 = torch.arange(Hkv, device=dev) * rep
    q[:, :, head0] *= D ** 0.5 / q[:, :, head0].norm(dim=-1, keepdim=True)
    q = q.bfloat16()
    k_new = rn(N, Sq, Hkv, D).bfloat16()
    v_new = rn(N, Sq, Hkv, D).clamp(-3.9, 3.9).bfloat16()
    cos, sin = ops.build_rope_cache(Tmax, D, 10000.0, torch.device(dev))
    q_rot = _rope_tokens(q, cos, sin, pos, lens)
    k_cache = rn(SLOTS, Tmax, Hkv, D).bfloat16()
    v_cache = rn(SLOTS, Tmax, Hkv, D).clamp(-3.9, 3.9).bfloat16()
    for n, (r, p, ln) in enumerate(zip(ROWS, pos, lens)):
        # aimed at the row's last valid token, whose bound is next to the poison
        k_cache[r, p:] = 4 * q_rot[n, ln - 1, head0]
        v_cache[r, p:] = 100.0
        k_new[n, ln:] = 4 * q[n, ln - 1, head0]
        v_new[n, ln:] = 100.0
    c = dict(q=q, k_new=k_new, v_new=v_new, k_cache=k_cache, v_cache=v_cache, cos=cos, sin=sin,
             pos=torch.tensor(pos, device=dev), q_lens=torch.tensor(lens, device=dev),
             rows=torch.tensor(ROWS, device=dev), lengths=torch.arange(11, 11 + SLOTS, device=dev),
             Tmax=Tmax, rep=rep, pos_h=pos, lens_h=lens)

    # the eager bf16 sequence the kernel replaces (LlamaAttention.forward, cache
    # and S != total, row by row) and fp32 attention of the same bf16 operands
    k_e, v_e = k_cache.clone(), v_cache.clone()
    k_rot = _rope_tokens(k_new, cos, sin, pos, lens)
    o_e = torch.zeros_like(q)
    ref = torch.zeros(q.shape, dtype=torch.float32, device=dev)
    for n, (r, p, ln) in enumerate(zip(ROWS, pos, lens)):
        k_e[r, p : p + ln] = k_rot[n, :ln]
        v_e[r, p : p + ln] = v_new[n, :ln]
        kt = k_e[r, : p + ln].transpose(0, 1).repeat_interleave(rep, dim=0)[None]  # [1,H,T,D]
        vt = v_e[r, : p + ln].transpose(0, 1).repeat_interleave(rep, dim=0)[None]
        qt = q_rot[n, :ln].transpose(0, 1)[None]
        mask = (torch.arange(p + ln, device=dev)[None, :]
                <= torch.arange(p, p + ln, device=dev)[:, None])
        o_e[n, :ln] = torch.nn.functional.scaled_dot_product_attention(
            qt, kt, vt, attn_mask=mask)[0].transpose(0, 1)
        s = torch.einsum("hid,htd->hit", qt[0].float(), kt[0].float()) / D ** 0.5
        s = s.masked_fill(~mask[None], float("-inf"))
        ref[n, :ln] = torch.einsum("hit,htd->ihd", torch.softmax(s, dim=-1), vt[0].float())
    c.update(o_eager=o_e, ref=ref, k_rot=k_rot)
    return c


def _kernel(c, split, **over):
    """One kernel call on clones of the case's cache -> (o, k, v, lengths)."""
    a = dict(c)
    a.update(over)
    k, v, ln = a["k_cache"].clone(), a["v_cache"].clone(), a["lengths"].clone()
    o = _ops().extend_attention(a["q"], a["k_new"], a["v_new"], k, v, a["cos"], a["sin"],
                                a["pos"], q_lens=a["q_lens"], rows=a["rows"], lengths=ln,
                                max_len=a.get("max_len"), chunk=_chunk(), split=split)
    return o, k, v, ln


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("split", [True, False], ids=["split", "direct"])
@pytest.mark.parametrize("H,Hkv,Sq", CASES)
def test_reference_and_side_effects(H, Hkv, Sq, split):
    c = _case(H, Hkv, Sq)
    o, k, v, ln = _kernel(c, split, max_len=max(p + n for p, n in zip(c["pos_h"], c["lens_h"])))
    ref = c["ref"]
    err = float((o.float() - ref).abs().max())
    err_eager = float((c["o_eager"].float() - ref).abs().max())
    ulp = float(_bf16_ulp(ref.abs().max()))
    print(f"\nextend H={H} Hkv={Hkv} Sq={Sq} {'split' if split else 'direct'}: kernel err "
          f"{err:.3e}  eager err {err_eager:.3e}  max|ref| {float(ref.abs().max()):.3f}  "
          f"ulp {ulp:.3e}")
    assert torch.isfinite(o.float()).all()
    assert float(ref.abs().max()) < 4
    assert err < 3e-2
    assert err <= 2 * err_eager + ulp

    # --- side effects
    written = torch.zeros(SLOTS, c["Tmax"], dtype=torch.bool, device="cuda")
    want_len = c["lengths"].clone()
    for n, (r, p, n_new) in enumerate(zip(ROWS, c["pos_h"], c["lens_h"])):
        written[r, p : p + n_new] = True
        want_len[r] = p + n_new
        assert _same(v[r, p : p + n_new], c["v_new"][n, :n_new])
        k_want = c["k_rot"][n, :n_new].float()
        assert bool(((k[r, p : p + n_new].float() - k_want).abs() <= _bf16_ulp(k_want)).all())
        assert not o[n, n_new:].any()
    for new, old in ((k, c["k_cache"]), (v, c["v_cache"])):
        assert _same(new[~written], old[~written])
    assert torch.equal(ln, want_len)


@pytest.mark.parametrize("split", [True, False], ids=["split", "direct"])
@pytest.mark.parametrize("H,Hkv", GEOMS)
def test_batch_invariance(H, Hkv, split):
    """A row's bits depend on that row and the call's (Sq, rep) alone: not on
    N, on the other rows, on the row order or on max_len."""
    c = _case(H, Hkv, 33)
    o, k, v, ln = _kernel(c, split)                # max_len = the cache length
    one = lambda t, s: t[s].clone()
    for n in range(len(ROWS)):
        s = slice(n, n + 1)
        o1, k1, v1, ln1 = _kernel(c, split, max_len=c["pos_h"][n] + c["lens_h"][n],
                                  **{key: one(c[key], s)
                                     for key in ("q", "k_new", "v_new", "pos", "q_lens", "rows")})
        assert _same(o1[0], o[n]), n
        # its cache row and length as in the full call, every other row untouched
        mine = torch.arange(SLOTS, device="cuda") == ROWS[n]
        for alone, full, old in ((k1, k, c["k_cache"]), (v1, v, c["v_cache"])):
            assert _same(alone[mine], full[mine]) and _same(alone[~mine], old[~mine]), n
        assert torch.equal(ln1, torch.where(mine, ln, c["lengths"])), n
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    o2, k2, v2, ln2 = _kernel(c, split, **{key: c[key][perm].contiguous()
                                           for key in ("q", "k_new", "v_new", "pos", "q_lens",
                                                       "rows")})
    assert _same(o2, o[perm]) and _same(k2, k) and _same(v2, v) and torch.equal(ln2, ln)


def test_single_token_consistent_with_decode():
    ops = _ops()
    c = _case(8, 2, 1)
    o, k, v, ln = _kernel(c, None)
    kd, vd, lnd = c["k_cache"].clone(), c["v_cache"].clone(), c["lengths"].clone()
    od = ops.decode_attention(c["q"], c["k_new"], c["v_new"], kd, vd, c["cos"], c["sin"],
                              c["pos"], rows=c["rows"], lengths=lnd)
    ref = c["ref"]
    err, err_d = (float((x.float() - ref).abs().max()) for x in (o, od))
    print(f"\nextend Sq=1 err {err:.3e}  decode err {err_d:.3e}")
    assert err <= 2 * err_d + float(_bf16_ulp(ref.abs().max())) and err < 3e-2
    assert _same(k, kd) and _same(v, vd) and torch.equal(ln, lnd)


@pytest.mark.parametrize("split", [True, False], ids=["split", "direct"])
def test_bad_metadata_rows_are_skipped(split):
    """A row whose cache row is >= slots and one with p + len > max_len give
    zero output and write nothing; the other rows are unaffected."""
    c = _case(8, 2, 33)
    C = _chunk()
    good, k_g, v_g, ln_g = _kernel(c, split)
    rows = c["rows"].clone()
    rows[2] = SLOTS + 2                            # row 2 (p = 2C+44): no such cache row
    max_len = C + 33 - 1                           # row 0 (p = C, len 33) ends one past it
    o, k, v, ln = _kernel(c, split, rows=rows, max_len=max_len)
    assert not o[0].any() and not o[2].any()
    for n in (1, 3, 4):
        assert _same(o[n], good[n])
    for r in (ROWS[0], ROWS[2]):                   # nothing written for the skipped rows
        assert _same(k[r], c["k_cache"][r]) and _same(v[r], c["v_cache"][r])
        assert ln[r] == c["lengths"][r]
    for r in (ROWS[1], ROWS[3], ROWS[4]):
        assert _same(k[r], k_g[r]) and _same(v[r], v_g[r]) and ln[r] == ln_g[r]


def test_llama_attention_kvcache_chunks_match_whole_prompt(monkeypatch):
    """A prompt fed to a bf16 / head_dim 128 LlamaAttention in chunks through a
    uniform KVCache (the prefill path for the first chunk, then the extend
    kernels) against the whole prompt in one prefill: outputs within the bound
    above, v cache identical, k cache within one bf16 ulp."""
    from lpp_amd.config import model_config
    from lpp_amd.models.llama import KVCache, LlamaAttention

    ops = _ops()
    cfg = model_config("llama-tiny", hidden_size=512, intermediate_size=1024, num_heads=4,
                       num_kv_heads=2, num_layers=1, max_seq_len=128)
    torch.manual_seed(0)
    attn = LlamaAttention(cfg).to("cuda", torch.bfloat16)
    with torch.no_grad():
        for p in attn.parameters():
            p.normal_(0.0, 0.05)
        attn.o_proj.weight.copy_(torch.eye(cfg.hidden_size))   # y is the attention output
    x = torch.randn(2, 11, cfg.hidden_size, device="cuda").bfloat16()
    real, calls = ops.extension(), []

    class Counting:
        def __getattr__(self, name):
            return getattr(real, name)

        def attention_extend(self, *a):
            calls.append(a[0].shape[1])
            return real.attention_extend(*a)

    monkeypatch.setattr(ops, "_EXT", Counting())
    new = lambda: KVCache(2, 16, cfg.kv_heads, cfg.head_dim, "cuda", torch.bfloat16)
    whole, chunked = new(), new()
    with torch.no_grad():
        y_w = attn(x, cache=whole)
        y_c = torch.cat([attn(x[:, a:b], cache=chunked) for a, b in ((0, 4), (4, 9), (9, 11))], 1)
    assert calls == [5, 2] and chunked.length == whole.length == 11
    err = float((y_c.float() - y_w.float()).abs().max())
    print(f"\nLlamaAttention KVCache, chunks vs whole prompt: max |dy| {err:.3e}  "
          f"max |y| {float(y_w.float().abs().max()):.3f}")
    assert torch.isfinite(y_c.float()).all() and float(y_w.float().abs().max()) < 4
    assert err < 3e-2
    assert _same(chunked.v[:, :11], whole.v[:, :11])
    dk = (chunked.k[:, :11].float() - whole.k[:, :11].float()).abs()
    assert bool((dk <= _bf16_ulp(whole.k[:, :11].float())).all())
