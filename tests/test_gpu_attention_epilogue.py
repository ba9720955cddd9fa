"""Epilogue stores of the three attention kernels at the sequence lengths where
they can go wrong: a single row, a tail inside a tile, a tail tile, a second q
block, a third kv block, and the GQA loop.  B = 2 throughout, so a store past
one batch's last row lands in rows of the next batch, which are checked
(pytest -m gpu)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, D = 2, 128


@pytest.fixture(scope="module")
def ext():
    from lpp_amd import ops

    return ops.extension()


def _ref_attn(q, k, v):
    Bq, Sq, Hq, Dq = q.shape
    Hkv = k.shape[2]
    qt = q.float().transpose(1, 2)
    kt = k.float().transpose(1, 2)
    vt = v.float().transpose(1, 2)
    if Hkv != Hq:
        rep = Hq // Hkv
        kt = kt.repeat_interleave(rep, dim=1)
        vt = vt.repeat_interleave(rep, dim=1)
    scores = qt @ kt.transpose(-1, -2) / math.sqrt(Dq)
    mask = torch.triu(torch.ones(Sq, Sq, dtype=torch.bool, device=q.device), 1)
    scores = scores.masked_fill(mask, float("-inf"))
    lse2 = torch.logsumexp(scores, -1) * math.log2(math.e)
    return (scores.softmax(-1) @ vt).transpose(1, 2), lse2


def _ref_attn_grads(q, k, v, do):
    """fp32 autograd reference for dq/dk/dv."""
    qf = q.float().detach().requires_grad_(True)
    kf = k.float().detach().requires_grad_(True)
    vf = v.float().detach().requires_grad_(True)
    out, _ = _ref_attn(qf, kf, vf)
    out.backward(do.float())
    return qf.grad, kf.grad, vf.grad


@pytest.mark.parametrize(
    "S,H,HKV",
    [(1, 2, 2), (37, 2, 2), (200, 2, 2), (320, 2, 2), (576, 2, 2), (320, 8, 2)],
    ids=["s1", "s37", "s200", "s320", "s576", "s320_gqa"],
)
def test_attention_epilogue_rows(ext, S, H, HKV):
    torch.manual_seed(30 + S + HKV)
    dev = torch.device("cuda", 0)
    q = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
    k = torch.randn(B, S, HKV, D, device=dev, dtype=torch.bfloat16)
    v = torch.randn_like(k)
    do = torch.randn_like(q)

    o, lse2 = ext.attention_fwd(q, k, v)
    dq, dk, dv = ext.attention_bwd(do, q, k, v, o, lse2)
    o2, lse2b = ext.attention_fwd(q, k, v)
    dq2, dk2, dv2 = ext.attention_bwd(do, q, k, v, o2, lse2b)
    for a, b_, name in ((o, o2, "o"), (lse2, lse2b, "lse2"), (dq, dq2, "dq"), (dk, dk2, "dk"),
                        (dv, dv2, "dv")):
        assert torch.equal(a, b_), f"{name}: two calls differ"

    ref, rlse2 = _ref_attn(q, k, v)
    rdq, rdk, rdv = _ref_attn_grads(q, k, v, do)
    oerr = (o.float() - ref).abs().max().item()
    assert oerr < 3e-2, oerr
    assert torch.allclose(lse2, rlse2, atol=1e-2, rtol=1e-2), (lse2 - rlse2).abs().max()
    for got, rg, name in ((dq, rdq, "dq"), (dk, rdk, "dk"), (dv, rdv, "dv")):
        err = (got.float() - rg).abs().max()
        den = rg.abs().max().clamp(min=1.0)
        assert err / den < 4e-2, f"{name} rel err {err / den} (abs {err})"
