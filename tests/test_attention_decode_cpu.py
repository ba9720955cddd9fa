"""decode_attention_ref (the CPU path and the oracle of the fused decode
kernel) against the eager steps it stands for: apply_rope_positions, scatter
into the cache, masked SDPA."""

import pytest
import torch

from lpp_amd import ops
from lpp_amd.ops.attention import decode_attention_ref

SLOTS, TMAX, D = 5, 32, 16
ROWS = [4, 1, 2]
POSITIONS = [0, 7, 30]


def _inputs(H, Hkv, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = len(ROWS)
    q = torch.randn(N, 1, H, D, generator=g)
    k_new = torch.randn(N, 1, Hkv, D, generator=g)
    v_new = torch.randn(N, 1, Hkv, D, generator=g)
    # the whole cache is random: positions past a row's own are stale data
    k_cache = torch.randn(SLOTS, TMAX, Hkv, D, generator=g)
    v_cache = torch.randn(SLOTS, TMAX, Hkv, D, generator=g)
    lengths = torch.tensor([3, 7, 30, 9, 0])
    cos, sin = ops.build_rope_cache(TMAX, D, 10000.0, "cpu")
    return q, k_new, v_new, k_cache, v_cache, lengths, cos, sin


def _eager_steps(q, k_new, v_new, k_cache, v_cache, lengths, cos, sin, rows, pos):
    """The ragged branch of LlamaAttention.forward, step by step."""
    H, Hkv = q.shape[2], k_new.shape[2]
    qr = ops.apply_rope_positions(q, cos, sin, pos)
    kr = ops.apply_rope_positions(k_new, cos, sin, pos)
    k_cache[rows, pos] = kr[:, 0]
    v_cache[rows, pos] = v_new[:, 0]
    lengths[rows] = pos + 1
    T = int(pos.max()) + 1
    kt = k_cache[rows, :T].transpose(1, 2).repeat_interleave(H // Hkv, dim=1)
    vt = v_cache[rows, :T].transpose(1, 2).repeat_interleave(H // Hkv, dim=1)
    mask = (torch.arange(T)[None, :] <= pos[:, None])[:, None, None, :]
    o = torch.nn.functional.scaled_dot_product_attention(
        qr.transpose(1, 2), kt, vt, attn_mask=mask)
    return o.transpose(1, 2).contiguous()


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
def test_ref_matches_eager_steps(H, Hkv):
    q, k_new, v_new, kc, vc, lengths, cos, sin = _inputs(H, Hkv)
    rows, pos = torch.tensor(ROWS), torch.tensor(POSITIONS)
    kc2, vc2, len2 = kc.clone(), vc.clone(), lengths.clone()
    want = _eager_steps(q, k_new, v_new, kc2, vc2, len2, cos, sin, rows, pos)
    got = decode_attention_ref(q, k_new, v_new, kc, vc, cos, sin, pos,
                               rows=rows, lengths=lengths)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    assert torch.equal(lengths, len2)
    assert lengths.tolist() == [3, 8, 31, 9, 1]


def test_int_positions_equal_constant_tensor():
    q, k_new, v_new, kc, vc, lengths, cos, sin = _inputs(8, 2, seed=1)
    kc2, vc2, len2 = kc.clone(), vc.clone(), lengths.clone()
    a = decode_attention_ref(q, k_new, v_new, kc, vc, cos, sin, 7, lengths=lengths)
    b = decode_attention_ref(q, k_new, v_new, kc2, vc2, cos, sin,
                             torch.full((len(ROWS),), 7), lengths=len2)
    assert torch.equal(a, b)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2) and torch.equal(lengths, len2)
    assert lengths.tolist() == [8, 8, 8, 9, 0]  # rows=None: batch row n is cache row n


def test_cpu_tensors_dispatch_to_reference(monkeypatch):
    import lpp_amd.ops.attention as A

    calls = []
    real = A.decode_attention_ref

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(A, "decode_attention_ref", counting)
    q, k_new, v_new, kc, vc, lengths, cos, sin = _inputs(4, 4, seed=2)
    rows, pos = torch.tensor(ROWS), torch.tensor(POSITIONS)
    kc2, vc2, len2 = kc.clone(), vc.clone(), lengths.clone()
    assert not ops.decode_attention_hip_supported(q, 4)
    got = ops.decode_attention(q, k_new, v_new, kc, vc, cos, sin, pos,
                               rows=rows, lengths=lengths, max_len=31)
    assert calls == [1]
    want = real(q, k_new, v_new, kc2, vc2, cos, sin, pos, rows=rows, lengths=len2)
    assert torch.equal(got, want) and torch.equal(kc, kc2) and torch.equal(lengths, len2)
