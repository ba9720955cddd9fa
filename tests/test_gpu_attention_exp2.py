"""The tile loops' P = 2^x is one raw v_exp_f32 (attn_exp2, attn_tile.h): a
result below 2^-126 is flushed to 0 where exp2f() gave a subnormal.  Inputs with
large score spreads put more than half of all unmasked P there; the outputs
still match the fp32 reference at the tolerances of test_gpu_attention.py
(pytest -m gpu)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, S, H, D = 2, 200, 2, 128


@pytest.fixture(scope="module")
def ext():
    from lpp_amd import ops

    return ops.extension()


def _ref_attn(q, k, v):
    Bq, Sq, Hq, Dq = q.shape
    qt = q.float().transpose(1, 2)
    kt = k.float().transpose(1, 2)
    vt = v.float().transpose(1, 2)
    scores = qt @ kt.transpose(-1, -2) / math.sqrt(Dq)
    mask = torch.triu(torch.ones(Sq, Sq, dtype=torch.bool, device=q.device), 1)
    scores = scores.masked_fill(mask, float("-inf"))
    return (scores.softmax(-1) @ vt).transpose(1, 2)


def _ref_attn_grads(q, k, v, do):
    """fp32 autograd reference for dq/dk/dv."""
    qf = q.float().detach().requires_grad_(True)
    kf = k.float().detach().requires_grad_(True)
    vf = v.float().detach().requires_grad_(True)
    out = _ref_attn(qf, kf, vf)
    out.backward(do.float())
    return qf.grad, kf.grad, vf.grad


def _ref_exponents(q, k):
    """fp32 reference: lse2 [B,H,S] and, for every unmasked (q, k) pair, the
    exp2-domain exponent c*s - lse2 that the backward kernels exponentiate."""
    s2 = (q.float().transpose(1, 2) @ k.float().transpose(1, 2).transpose(-1, -2)) * (
        math.log2(math.e) / math.sqrt(D)
    )
    keep = torch.tril(torch.ones(S, S, dtype=torch.bool, device=q.device))
    lse2 = torch.logsumexp(s2.masked_fill(~keep, float("-inf")) * math.log(2.0), -1) / math.log(2.0)
    return lse2, (s2 - lse2[..., None])[..., keep]


@pytest.mark.parametrize(
    "gain,flushes", [(6.0, True), (3.0, False)], ids=["flushed_p", "normal_p"]
)
def test_attention_raw_exp2(ext, gain, flushes):
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    q = (gain * torch.randn(B, S, H, D)).to(torch.bfloat16).to(dev)
    k = (gain * torch.randn(B, S, H, D)).to(torch.bfloat16).to(dev)
    v = torch.randn(B, S, H, D).to(torch.bfloat16).to(dev)
    do = torch.randn(B, S, H, D).to(torch.bfloat16).to(dev)

    # the inputs themselves decide whether the flush is exercised
    rlse2, expo = _ref_exponents(q, k)
    share = (expo < -126.0).float().mean().item()
    print(f"\ngain {gain}: share of exponents below -126 = {share:.4f}, min = {expo.min().item():.1f}")
    if flushes:
        assert share >= 0.25, share
    else:
        assert share == 0.0, share

    o, lse2 = ext.attention_fwd(q, k, v)
    dq, dk, dv = ext.attention_bwd(do, q, k, v, o, lse2)
    o2, lse2b = ext.attention_fwd(q, k, v)
    dq2, dk2, dv2 = ext.attention_bwd(do, q, k, v, o2, lse2b)
    for a, b_, name in ((o, o2, "o"), (lse2, lse2b, "lse2"), (dq, dq2, "dq"), (dk, dk2, "dk"),
                        (dv, dv2, "dv")):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b_), f"{name}: two calls differ"

    ref = _ref_attn(q, k, v)
    rdq, rdk, rdv = _ref_attn_grads(q, k, v, do)
    oerr = (o.float() - ref).abs().max().item()
    lerr = (lse2 - rlse2).abs().max().item()
    print(f"o abs err {oerr:.3e}  lse2 abs err {lerr:.3e}")
    assert oerr < 3e-2, oerr
    assert torch.allclose(lse2, rlse2, atol=1e-2, rtol=1e-2), lerr
    for got, rg, name in ((dq, rdq, "dq"), (dk, rdk, "dk"), (dv, rdv, "dv")):
        err = (got.float() - rg).abs().max()
        den = rg.abs().max().clamp(min=1.0)
        print(f"{name} rel err {(err / den).item():.3e} (abs {err.item():.3e}, den {den.item():.3e})")
        assert err / den < 4e-2, f"{name} rel err {err / den} (abs {err})"
