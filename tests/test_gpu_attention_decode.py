"""Fused single-token decode attention (attention_decode.hip) on the GPU.

The cache is built so that every way of reading a wrong key shows: the valid
prefix of a row is random, everything at or past the row's position - and all
of every unused row - is poison (k = 4 * rotated q, a score of about 45;
v = 100), and some rows carry a needle key (k = 2 * rotated q) whose value
the output of the group's first head must reproduce.

Measured on MI355X (C = 256; printed by test_reference_needles_side_effects,
recorded in profiles/README.md, Round 6): kernel max error 4.8e-7 to 7.6e-3,
equal to the eager bf16 path's in every case (both at the rounding of the
bf16 output; max |ref| 3.4 to 3.9); needle deviation 0 on every needle row.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
SLOTS = 5
GEOMS = [(4, 4), (8, 2), (16, 2)]


def _ext():
    from lpp_amd import ops

    return ops.extension()


def _chunk():
    return int(_ext().attention_decode_chunk())


def _cases(C):
    """(rows, positions, needle position or None) - every position of
    {0, 1, C-1, C, C+1, 2C+44}; needles at key 0, at the first and the last
    key of a chunk, at p-1 and at p itself."""
    return {
        "a": ([4, 1, 2, 0, 3],
              [C + 1, 0, 2 * C + 44, C - 1, 1],
              [C, 0, C - 1, 0, None]),
        "b": ([2, 0, 3, 4],
              [C, 2 * C + 44, 1, 2 * C + 44],
              [C - 1, 2 * C + 44, 0, 2 * C]),
    }


def _bf16_ulp(x):
    """One bf16 unit in the last place at the magnitude of x (fp32 tensor)."""
    _, e = torch.frexp(x.float())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 8)


def _rope(x, cos, sin, pos):
    from lpp_amd import ops

    return ops.apply_rope_positions(x, cos, sin, pos)


def _build(H, Hkv, rows, positions, needles, seed=0):
    """Inputs and the poisoned cache of one case, on the GPU in bf16."""
    from lpp_amd import ops

    C = _chunk()
    Tmax = 2 * C + 64
    rep = H // Hkv
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(seed)
    N = len(rows)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    q = rn(N, 1, H, D)
    head0 = torch.arange(Hkv, device=dev) * rep          # first head of each group
    # |q|^2 = D for the heads that needles and poison are aimed at, so that a
    # needle scores 2 sqrt(D) = 22.6 and poison 45 whatever the draw
    q[:, :, head0] *= D ** 0.5 / q[:, :, head0].norm(dim=-1, keepdim=True)
    q = q.bfloat16()
    k_new = rn(N, 1, Hkv, D).bfloat16()
    v_new = rn(N, 1, Hkv, D).clamp(-3.9, 3.9).bfloat16()
    cos, sin = ops.build_rope_cache(Tmax, D, 10000.0, torch.device(dev))
    pos = torch.tensor(positions, device=dev)
    row_t = torch.tensor(rows, device=dev)
    for n, ns in enumerate(needles):                     # needle at p itself: through k_new
        if ns is not None and ns == positions[n]:
            k_new[n, 0] = 2 * q[n, 0, head0]             # exact in bf16
    q_rot = _rope(q, cos, sin, pos)                      # bf16 [N,1,H,D]
    k_cache = rn(SLOTS, Tmax, Hkv, D).bfloat16()
    v_cache = rn(SLOTS, Tmax, Hkv, D).clamp(-3.9, 3.9).bfloat16()
    used = set(rows)
    for r in range(SLOTS):
        if r not in used:
            k_cache[r] = 4 * q_rot[0, 0, head0]
            v_cache[r] = 100.0
    for n, (r, p, ns) in enumerate(zip(rows, positions, needles)):
        k_cache[r, p:] = 4 * q_rot[n, 0, head0]
        v_cache[r, p:] = 100.0
        if ns is not None and ns < p:
            k_cache[r, ns] = 2 * q_rot[n, 0, head0]
    lengths = torch.arange(11, 11 + SLOTS, device=dev)
    return dict(q=q, k_new=k_new, v_new=v_new, k_cache=k_cache, v_cache=v_cache,
                cos=cos, sin=sin, pos=pos, rows=row_t, lengths=lengths, q_rot=q_rot,
                Tmax=Tmax, rep=rep, head0=head0)


def _kernel(c, **over):
    """One kernel call on clones of the case's cache -> (o, k, v, lengths)."""
    from lpp_amd import ops

    a = dict(c)
    a.update(over)
    k, v, ln = a["k_cache"].clone(), a["v_cache"].clone(), a["lengths"].clone()
    o = ops.decode_attention(a["q"], a["k_new"], a["v_new"], k, v, a["cos"], a["sin"],
                             a["pos"], rows=a["rows"], lengths=ln,
                             max_len=a.get("max_len"))
    return o, k, v, ln


def _eager_bf16(c):
    """The eager sequence the kernel replaces (ragged branch of
    LlamaAttention.forward), in bf16 -> (o, k, v)."""
    k, v = c["k_cache"].clone(), c["v_cache"].clone()
    pos, rows, rep = c["pos"], c["rows"], c["rep"]
    kr = _rope(c["k_new"], c["cos"], c["sin"], pos)
    k[rows, pos] = kr[:, 0]
    v[rows, pos] = c["v_new"][:, 0]
    T = int(pos.max()) + 1
    kt = k[rows, :T].transpose(1, 2).repeat_interleave(rep, dim=1)
    vt = v[rows, :T].transpose(1, 2).repeat_interleave(rep, dim=1)
    mask = (torch.arange(T, device=pos.device)[None, :] <= pos[:, None])[:, None, None, :]
    o = torch.nn.functional.scaled_dot_product_attention(
        c["q_rot"].transpose(1, 2), kt, vt, attn_mask=mask)
    return o.transpose(1, 2).contiguous(), k, v


def _ref_fp32(c, k, v):
    """fp32 attention of the bf16-rounded rotated operands: k/v are the cache
    after the eager write (rotated k_new rounded to bf16 at [row, p])."""
    rep = c["rep"]
    out = torch.empty(c["q"].shape, dtype=torch.float32, device=k.device)
    for n, (r, p) in enumerate(zip(c["rows"].tolist(), c["pos"].tolist())):
        kk = k[r, : p + 1].float().repeat_interleave(rep, dim=1)
        vv = v[r, : p + 1].float().repeat_interleave(rep, dim=1)
        s = torch.einsum("hd,thd->ht", c["q_rot"][n, 0].float(), kk) / D ** 0.5
        out[n, 0] = torch.einsum("ht,thd->hd", torch.softmax(s, dim=-1), vv)
    return out


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("H,Hkv", GEOMS)
def test_reference_needles_side_effects(H, Hkv, case):
    C = _chunk()
    rows, positions, needles = _cases(C)[case]
    c = _build(H, Hkv, rows, positions, needles)
    o, k, v, ln = _kernel(c, max_len=max(positions) + 1)
    o_e, k_e, v_e = _eager_bf16(c)
    ref = _ref_fp32(c, k_e, v_e)

    # --- against the fp32 reference, and against the eager path's own error
    err = float((o.float() - ref).abs().max())
    err_eager = float((o_e.float() - ref).abs().max())
    ulp = float(_bf16_ulp(ref.abs().max()))
    print(f"\ndecode H={H} Hkv={Hkv} case={case}: kernel err {err:.3e}  "
          f"eager err {err_eager:.3e}  max|ref| {float(ref.abs().max()):.3f}  ulp {ulp:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err < 3e-2
    assert err <= 2 * err_eager + ulp

    # --- needle rows: the group's first head returns the needle's value
    for n, (r, p, ns) in enumerate(zip(rows, positions, needles)):
        if ns is None:
            continue
        want = c["v_new"][n, 0] if ns == p else c["v_cache"][r, ns]   # [Hkv, D]
        dev_ref = float((ref[n, 0, c["head0"]] - want.float()).abs().max())
        dev_k = float((o[n, 0, c["head0"]].float() - want.float()).abs().max())
        print(f"  needle row {n} p={p} p*={ns}: |o - v[p*]| kernel {dev_k:.3e} ref {dev_ref:.3e}")
        assert dev_ref < 1e-4
        assert dev_k <= 2e-2

    # --- side effects
    pos, row_t = c["pos"], c["rows"]
    assert torch.equal(v[row_t, pos].view(torch.int16), c["v_new"][:, 0].view(torch.int16))
    k_want = _rope(c["k_new"], c["cos"], c["sin"], pos)[:, 0].float()
    assert bool(((k[row_t, pos].float() - k_want).abs() <= _bf16_ulp(k_want)).all())
    untouched = torch.ones(SLOTS, c["Tmax"], dtype=torch.bool, device="cuda")
    untouched[row_t, pos] = False
    for new, old in ((k, c["k_cache"]), (v, c["v_cache"])):
        assert torch.equal(new[untouched].view(torch.int16), old[untouched].view(torch.int16))
    want_len = c["lengths"].clone()
    want_len[row_t] = pos + 1
    assert torch.equal(ln, want_len)


@pytest.mark.parametrize("H,Hkv", GEOMS)
def test_batch_invariance(H, Hkv):
    """A row's output bits depend on that row alone: not on N, on the other
    rows, on the row order or on max_len."""
    C = _chunk()
    rows, positions, needles = _cases(C)["a"]
    c = _build(H, Hkv, rows, positions, needles, seed=1)
    o, k, v, ln = _kernel(c)                       # max_len = the cache length
    for n in range(len(rows)):
        s = slice(n, n + 1)
        o1, _, _, _ = _kernel(c, q=c["q"][s].contiguous(), k_new=c["k_new"][s].contiguous(),
                              v_new=c["v_new"][s].contiguous(), pos=c["pos"][s].clone(),
                              rows=c["rows"][s].clone(), max_len=positions[n] + 1)
        assert torch.equal(o1[0].view(torch.int16), o[n].view(torch.int16)), n
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    o2, k2, v2, ln2 = _kernel(c, q=c["q"][perm].contiguous(),
                              k_new=c["k_new"][perm].contiguous(),
                              v_new=c["v_new"][perm].contiguous(), pos=c["pos"][perm],
                              rows=c["rows"][perm], max_len=max(positions) + 1)
    assert torch.equal(o2.view(torch.int16), o[perm].view(torch.int16))
    assert torch.equal(k2.view(torch.int16), k.view(torch.int16))
    assert torch.equal(v2.view(torch.int16), v.view(torch.int16))
    assert torch.equal(ln2, ln)


def test_uniform_int_position_equals_constant_tensor():
    from lpp_amd import ops

    C = _chunk()
    H, Hkv, p = 8, 2, C + 1
    c = _build(H, Hkv, [0, 1, 2, 3, 4], [p] * 5, [None] * 5, seed=2)
    outs = []
    for positions in (p, torch.full((5,), p, device="cuda")):
        k, v = c["k_cache"].clone(), c["v_cache"].clone()
        o = ops.decode_attention(c["q"], c["k_new"], c["v_new"], k, v, c["cos"], c["sin"],
                                 positions, max_len=p + 1)
        outs.append((o, k, v))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.isfinite(outs[0][0].float()).all()


def test_short_row_next_to_long_row():
    C = _chunk()
    c = _build(16, 2, [3, 1], [0, 2 * C + 44], [None, None], seed=3)
    o, _, _, ln = _kernel(c)
    assert torch.isfinite(o.float()).all()
    # a row at p = 0 attends the new token alone
    assert torch.equal(o[0, 0].view(torch.int16),
                       c["v_new"][0, 0].repeat_interleave(8, dim=0).view(torch.int16))
    assert ln[3] == 1 and ln[1] == 2 * C + 45


def test_positions_sharing_storage_with_lengths():
    """A bare RaggedKVCache passes its lengths as the positions.  The kernel
    stores lengths[row] while other workgroups still read positions, so the op
    hands it a copy: same result as with separate tensors."""
    from lpp_amd import ops

    C = _chunk()
    positions = [C + 1, 0, 2 * C + 44, C - 1, 1]
    c = _build(8, 2, [0, 1, 2, 3, 4], positions, [None] * 5, seed=4)
    outs = []
    for alias in (False, True):
        k, v = c["k_cache"].clone(), c["v_cache"].clone()
        lengths = c["pos"].clone()
        pos = lengths if alias else lengths.clone()
        o = ops.decode_attention(c["q"], c["k_new"], c["v_new"], k, v, c["cos"], c["sin"],
                                 pos, lengths=lengths)
        assert lengths.tolist() == [p + 1 for p in positions]
        outs.append((o, k, v))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------------------------------------------------------------------------
# model level, head_dim 128
# ---------------------------------------------------------------------------

def _counting_ext(monkeypatch):
    """Wrap the extension so that calls of attention_decode are counted."""
    from lpp_amd import ops

    real = ops.extension()
    calls = []

    class Counting:
        def __getattr__(self, name):
            return getattr(real, name)

        def attention_decode(self, *a, **kw):
            calls.append(1)
            return real.attention_decode(*a, **kw)

    monkeypatch.setattr(ops, "_EXT", Counting())
    return calls


def _cfg128(**kw):
    from lpp_amd.config import model_config

    return model_config("llama-tiny", hidden_size=512, intermediate_size=1024, num_heads=4,
                        num_kv_heads=2, **kw)


def test_llama_attention_ragged_decode_kernel_vs_eager(monkeypatch):
    from lpp_amd.models.llama import GatherKVCache, LlamaAttention, RaggedKVCache

    cfg = _cfg128(num_layers=1, max_seq_len=128)
    torch.manual_seed(0)
    attn = LlamaAttention(cfg).to("cuda", torch.bfloat16)
    with torch.no_grad():
        for p in attn.parameters():
            p.normal_(0.0, 0.05)
        # hidden = H * D: an identity o_proj hands the attention output through
        # unchanged, so the attention bound applies to y as it stands
        attn.o_proj.weight.copy_(torch.eye(cfg.hidden_size))
    slots, active, lens = 4, [3, 1], [17, 40]

    def run():
        g = torch.Generator(device="cuda").manual_seed(5)
        cache = RaggedKVCache(slots, 64, cfg.kv_heads, cfg.head_dim, "cuda", torch.bfloat16)
        cache.k.copy_(torch.randn(cache.k.shape, generator=g, device="cuda"))
        cache.v.copy_(torch.randn(cache.v.shape, generator=g, device="cuda"))
        slot_t = torch.tensor(active, device="cuda")
        cache.lengths[slot_t] = torch.tensor(lens, device="cuda")
        view = GatherKVCache(cache, slot_t, total_hint=max(lens) + 1)
        x = torch.randn(2, 1, cfg.hidden_size, generator=g, device="cuda").bfloat16()
        with torch.no_grad():
            y = attn(x, cache=view)
        return y, cache

    calls = _counting_ext(monkeypatch)
    y_k, c_k = run()
    assert calls == [1]
    monkeypatch.setenv("LPP_FORCE_EAGER", "1")
    y_e, c_e = run()
    assert calls == [1]
    err = float((y_k.float() - y_e.float()).abs().max())
    print(f"\nLlamaAttention ragged decode, kernel vs eager: max |dy| {err:.3e}")
    assert torch.isfinite(y_k.float()).all()
    assert err < 3e-2
    assert torch.equal(c_k.lengths, c_e.lengths)
    assert c_k.lengths.tolist() == [0, 41, 0, 18]
    assert torch.equal(c_k.v.view(torch.int16), c_e.v.view(torch.int16))
    dk = (c_k.k.float() - c_e.k.float()).abs()
    assert bool((dk <= _bf16_ulp(c_e.k.float())).all())


def test_continuous_batching_engine_runs_decode_kernel(monkeypatch):
    from lpp_amd.models import LlamaForCausalLM, init_monolithic_weights
    from lpp_amd.serving import ContinuousBatchingEngine, Request

    cfg = _cfg128(num_layers=2, max_seq_len=128)
    m = LlamaForCausalLM(cfg)
    init_monolithic_weights(m, seed=9)
    m = m.to("cuda").to(torch.bfloat16)
    g = torch.Generator().manual_seed(4)
    prompts = [torch.randint(4, cfg.vocab_size, (n,), generator=g).cuda() for n in (5, 9, 3)]
    new = [4, 6, 5]
    calls = _counting_ext(monkeypatch)
    eng = ContinuousBatchingEngine(m, max_slots=2, max_seq_len=64)
    eng.submit(Request("r0", prompts[0], new[0]))
    eng.submit(Request("r1", prompts[1], new[1]))
    ticks = 0
    while eng.pending():
        eng.step()
        ticks += 1
        if ticks == 2:
            eng.submit(Request("r2", prompts[2], new[2]))   # staggered arrival
        assert ticks < 50
    for i in range(3):
        out = eng.results[f"r{i}"]
        assert out.numel() == prompts[i].numel() + new[i]
        assert torch.equal(out[: prompts[i].numel()], prompts[i].cpu())
        assert int(out.min()) >= 0 and int(out.max()) < cfg.vocab_size
    # every decode tick ran the kernel once per layer
    assert len(calls) > 0 and len(calls) % cfg.num_layers == 0
    # cache lengths of the slots last used: prompt + generated - 1 tokens cached
    # (the last sampled token is never fed), then freed
    assert all(int(c.lengths.sum()) == 0 for c in eng.caches)

    # uniform KVCache decode (generate) takes the same kernel
    n0 = len(calls)
    out = m.generate(prompts[0].view(1, -1), max_new_tokens=3)
    assert out.shape == (1, prompts[0].numel() + 3)
    assert len(calls) - n0 == 3 * cfg.num_layers   # one decode step per new token
