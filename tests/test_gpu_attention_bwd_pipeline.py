"""The double-buffered attention-backward pipeline (dQ and dK/dV) at the
shapes where its staging or its tile classes change (pytest -m gpu).

Each shape runs the backward twice on the same inputs: the two results must
be bit-equal, finite, and agree with the fp32 autograd reference under the
criterion of tests/test_gpu_attention.py.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128

# name -> (B, S, H, Hkv)
SHAPES = {
    # one tile, only the masked path
    "one_tile": (1, 64, 2, 2),
    # one dK/dV block, two q tiles
    "one_kv_block": (2, 128, 4, 4),
    # five q tiles: odd count, both buffer parities, and the first dK/dV
    # blocks whose waves skip interior work
    "five_tiles": (1, 320, 2, 2),
    # tail rows, S not a multiple of any tile
    "tail_200": (1, 200, 2, 2),
    "tail_1": (1, 1, 2, 2),
    # interior, diagonal and tail tiles in one head
    "all_classes": (1, 576, 1, 1),
    # GQA: the g loop reuses the buffers across heads
    "gqa": (1, 320, 8, 2),
}


def _ref_attn(q, k, v):
    _, S, H, _ = q.shape
    Hkv = k.shape[2]
    qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v))
    if Hkv != H:
        kt = kt.repeat_interleave(H // Hkv, dim=1)
        vt = vt.repeat_interleave(H // Hkv, dim=1)
    scores = qt @ kt.transpose(-1, -2) / math.sqrt(D)
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device=q.device), 1)
    return (scores.masked_fill(mask, float("-inf")).softmax(-1) @ vt).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(two backward results, fp32 reference grads) of one shape, computed once."""
    from lpp_amd import ops

    ext = ops.extension()
    B, S, H, Hkv = SHAPES[name]
    g = torch.Generator().manual_seed(1000 + S + H)
    dev = torch.device("cuda", 0)
    q = torch.randn(B, S, H, D, generator=g).to(dev, torch.bfloat16)
    k = torch.randn(B, S, Hkv, D, generator=g).to(dev, torch.bfloat16)
    v = torch.randn(B, S, Hkv, D, generator=g).to(dev, torch.bfloat16)
    do = torch.randn(B, S, H, D, generator=g).to(dev, torch.bfloat16)
    o, lse2 = ext.attention_fwd(q, k, v)
    first = ext.attention_bwd(do, q, k, v, o, lse2)
    second = ext.attention_bwd(do, q, k, v, o, lse2)
    leaves = [t.float().detach().requires_grad_(True) for t in (q, k, v)]
    _ref_attn(*leaves).backward(do.float())
    return first, second, tuple(t.grad for t in leaves)


@pytest.mark.parametrize("name", list(SHAPES))
def test_matches_fp32_reference(name):
    first, _, ref = _case(name)
    for got, refg, gname in zip(first, ref, ("dq", "dk", "dv")):
        assert got.shape == refg.shape
        err = (got.float() - refg).abs().max()
        den = refg.abs().max().clamp(min=1.0)
        print(f"{name} {gname}: rel err {float(err / den):.3e}")
        assert err / den < 4e-2, f"{gname} rel err {err / den} (abs {err})"


@pytest.mark.parametrize("name", list(SHAPES))
def test_finite(name):
    first, _, _ = _case(name)
    for got, gname in zip(first, ("dq", "dk", "dv")):
        assert bool(torch.isfinite(got.float()).all()), gname


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_calls_bit_equal(name):
    first, second, _ = _case(name)
    for a, b, gname in zip(first, second, ("dq", "dk", "dv")):
        assert torch.equal(a, b), gname
