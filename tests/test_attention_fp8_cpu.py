"""FP8 (e4m3) KV cache on the CPU: the quantisation rule, the two references
over fp8 caches against float64 attention over the dequantised cache they
leave behind, and the serving engine with ``kv_dtype=torch.float8_e4m3fn``."""

import pytest
import torch

from lpp_amd import ops
from lpp_amd.config import model_config
from lpp_amd.models import LlamaForCausalLM, init_monolithic_weights
from lpp_amd.serving import ContinuousBatchingEngine, Request

FP8 = torch.float8_e4m3fn
D = 128


def test_quantisation_rule():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, D, generator=g) * torch.logspace(-20, 20, 64)[:, None]
    x[0] = 0.0                                      # a row of zeros
    for i, k in enumerate((-7, 0, 5), start=1):     # amax exactly 448 * 2^k
        x[i] = x[i].clamp(-1, 1) * 2.0 ** k
        x[i, 3] = -448.0 * 2.0 ** k
    x = x.bfloat16()
    b, s = ops.quantize_kv_rows_fp8(x)
    assert b.dtype is FP8 and s.dtype is torch.float32 and s.shape == (64,)
    assert torch.equal(torch.frexp(s)[0], torch.full((64,), 0.5))      # powers of two
    assert s[0] == 1.0 and not b[0].float().any()
    assert torch.equal(s[1:4], 2.0 ** torch.tensor([-7.0, 0.0, 5.0]))  # 448 itself fits
    # amax / scale lies in (224, 448]; its byte can round down to 224 itself
    # (225 is no e4m3 number: the step below 256 is 16)
    pre = (x.float().abs().amax(-1) / s)[1:]
    assert bool((pre > 224).all()) and bool((pre <= 448).all())
    top = b.float().abs().amax(-1)[1:]
    assert bool((top >= 224).all()) and bool((top <= 448).all())
    deq = b.float() * s[:, None]
    assert torch.equal(deq.bfloat16().float(), deq)                    # exact in bf16
    # half an e4m3 step at 448 is 16: 3 mantissa bits
    assert bool(((deq - x.float()).abs() <= 16 * s[:, None]).all())
    tiny = torch.full((1, D), 2.0 ** -120).bfloat16()                  # below the clamp
    assert ops.quantize_kv_rows_fp8(tiny)[1][0] == 2.0 ** -100


def _f64_attention(q_rot, k, v, ks, vs, r, T, rep):
    """float64 attention of rotated q [ln,H,D] at keys 0..T-ln+i over the
    dequantised cache row r."""
    kk = (k[r, :T].double() * ks[r, :, :T].T[..., None].double()).repeat_interleave(rep, 1)
    vv = (v[r, :T].double() * vs[r, :, :T].T[..., None].double()).repeat_interleave(rep, 1)
    ln = q_rot.shape[0]
    s = torch.einsum("ihd,thd->hit", q_rot.double(), kk) / D ** 0.5
    hidden = torch.arange(T)[None, :] > torch.arange(T - ln, T)[:, None]
    p = torch.softmax(s.masked_fill(hidden[None], float("-inf")), -1)
    return torch.einsum("hit,thd->ihd", p, vv)


@pytest.mark.parametrize("extend", [False, True])
def test_refs_attend_the_cache_they_leave(extend):
    H, Hkv, slots, Tmax, Sq = 4, 2, 4, 24, 5 if extend else 1
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g)
    rows, pos = torch.tensor([2, 0, 3]), torch.tensor([0, 7, 11])
    lens = torch.tensor([5, 1, 3]) if extend else torch.ones(3, dtype=torch.long)
    q, k_new, v_new = (rn(3, Sq, h, D).bfloat16() for h in (H, Hkv, Hkv))
    cos, sin = ops.build_rope_cache(Tmax, D, 10000.0, torch.device("cpu"))
    k0, ks0 = ops.quantize_kv_rows_fp8(rn(slots, Tmax, Hkv, D).bfloat16())
    v0, vs0 = ops.quantize_kv_rows_fp8(rn(slots, Tmax, Hkv, D).bfloat16())
    ks0, vs0 = ks0.transpose(1, 2).contiguous(), vs0.transpose(1, 2).contiguous()
    k, v, ks, vs = k0.clone(), v0.clone(), ks0.clone(), vs0.clone()
    ln = torch.zeros(slots, dtype=torch.long)
    kw = dict(rows=rows, lengths=ln, k_scale=ks, v_scale=vs)
    if extend:
        o = ops.extend_attention(q, k_new, v_new, k, v, cos, sin, pos, q_lens=lens, **kw)
    else:
        o = ops.decode_attention(q, k_new, v_new, k, v, cos, sin, pos, **kw)
    written = torch.zeros(slots, Tmax, dtype=torch.bool)
    for n, (r, p, l) in enumerate(zip(rows.tolist(), pos.tolist(), lens.tolist())):
        at = torch.arange(p, p + l)
        q_rot = ops.apply_rope_positions(q[n, :l].unsqueeze(1), cos, sin, at)[:, 0]
        ref = _f64_attention(q_rot, k, v, ks, vs, r, p + l, H // Hkv)
        # o is the bf16 rounding of an fp32 composition of these same numbers
        assert float((o[n, :l].double() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max())
        assert not o[n, l:].float().any()
        written[r, p : p + l] = True
        assert int(ln[r]) == p + l
        k_rot = ops.apply_rope_positions(k_new[n, :l].unsqueeze(1), cos, sin, at)[:, 0]
        for new, cache, scale in ((k_rot, k, ks), (v_new[n, :l], v, vs)):
            b, s = ops.quantize_kv_rows_fp8(new)
            assert torch.equal(cache[r, p : p + l].view(torch.uint8), b.view(torch.uint8))
            assert torch.equal(scale[r, :, p : p + l], s.T)
    for new, old in ((k, k0), (v, v0)):
        assert torch.equal(new.view(torch.uint8)[~written], old.view(torch.uint8)[~written])
    for new, old in ((ks, ks0), (vs, vs0)):
        assert torch.equal(new.transpose(1, 2)[~written], old.transpose(1, 2)[~written])


def test_fp8_cache_needs_both_scales():
    q = torch.zeros(1, 1, 2, D)
    kv = torch.zeros(1, 1, 2, D)
    cache = torch.zeros(1, 4, 2, D).to(FP8)
    cos, sin = ops.build_rope_cache(4, D, 10000.0, torch.device("cpu"))
    for fn in (ops.decode_attention, ops.extend_attention):
        with pytest.raises(ValueError, match="k_scale"):
            fn(q, kv, kv, cache, cache.clone(), cos, sin, 0, k_scale=torch.ones(1, 2, 4))
    with pytest.raises(ValueError, match="impl"):
        ops.decode_attention(q, kv, kv, cache, cache.clone(), cos, sin, 0, impl="mfma",
                             k_scale=torch.ones(1, 2, 4), v_scale=torch.ones(1, 2, 4))


def test_engine_serves_from_an_fp8_cache():
    cfg = model_config("llama-tiny", num_layers=2, max_seq_len=128)
    m = LlamaForCausalLM(cfg)
    init_monolithic_weights(m, seed=9)
    with pytest.raises(ValueError, match="prefill_chunk"):
        ContinuousBatchingEngine(m, max_slots=4, max_seq_len=64, kv_dtype=FP8)
    eng = ContinuousBatchingEngine(m, max_slots=2, max_seq_len=64, kv_dtype=FP8, prefill_chunk=4)
    assert eng.caches[0].k.dtype is FP8 and eng.caches[0].k_scale.shape == (2, cfg.kv_heads, 64)
    g = torch.Generator().manual_seed(4)
    want = {"a": (6, 5), "b": (3, 7), "c": (10, 2)}       # three requests over two slots
    for uid, (n, new) in want.items():
        eng.submit(Request(uid, torch.randint(4, cfg.vocab_size, (n,), generator=g), new))
    for _ in range(60):
        if not eng.pending():
            break
        eng.step()
    assert not eng.pending()
    for uid, (n, new) in want.items():
        assert eng.results[uid].numel() == n + new
