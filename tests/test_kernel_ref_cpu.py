"""The float64 oracle of tests/kernel_ref.py, checked without a GPU.

(a) The bound is honest: for every case of the GPU matrix the project's own
    eager path, computed in fp32 and rounded to T, passes ``check`` with no
    exclusions.
(b) The bound bites: ``check`` rejects a list of small, classic mistakes.
"""

import pytest
import torch

from tests import kernel_ref as kr
from tests.kernel_ref import DTYPES, check, check_close, dtype_name

DT = pytest.mark.parametrize("dtype", DTYPES, ids=dtype_name)


# ----------------------------------------------------------------------
# (a) eager fp32 path vs float64 reference
# ----------------------------------------------------------------------
def _eager_rmsnorm(c, dtype):
    from lpp_amd.ops.rmsnorm import rmsnorm_ref

    y = rmsnorm_ref(c["x"], c["w"], kr.EPS)
    xf = c["x"].float().requires_grad_(True)
    wf = c["w"].clone().requires_grad_(True)
    d = kr.sum_partials(list(c["dys"]))
    rmsnorm_ref(xf, wf, kr.EPS).backward(d.float())
    dx = xf.grad.to(dtype)
    if c["dres"] is not None:
        dx = (dx.float() + c["dres"].float()).to(dtype)
    return y, dx, wf.grad


@DT
@pytest.mark.parametrize("rows,H", kr.RMSNORM_SHAPES)
def test_eager_rmsnorm(rows, H, dtype):
    c = kr.rmsnorm_case(rows, H, dtype)
    y, dx, dw = _eager_rmsnorm(c, dtype)
    check(y, c["y"], c["M_y"], dtype, op="rmsnorm y")
    check(dx, c["dx"], c["M_dx"], dtype, op="rmsnorm dx")
    check(dw, c["dw"], c["M_dw"], torch.float32, op="rmsnorm dw")
    inv = torch.rsqrt(c["x"].float().pow(2).mean(-1) + kr.EPS)
    check(inv, c["inv"], c["M_inv"], torch.float32, op="rmsnorm inv_rms")


@DT
def test_eager_rmsnorm_fused(dtype):
    c = kr.rmsnorm_case(2085, 2048, dtype, n_dy=3, with_res=True)
    _, dx, dw = _eager_rmsnorm(c, dtype)
    check(dx, c["dx"], c["M_dx"], dtype, op="rmsnorm fused dx", pre=c["pre_dx"])
    check(dw, c["dw"], c["M_dw"], torch.float32, op="rmsnorm fused dw")


@DT
@pytest.mark.parametrize("shape", kr.ROPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eager_rope(shape, dtype):
    from lpp_amd.ops.rope import apply_rope_ref

    B, S, H, D, pos, length = shape
    c = kr.rope_case(*shape, dtype)
    y = apply_rope_ref(c["x"], c["cos"], c["sin"], pos)
    check(y, c["y"], c["M_y"], dtype, op="rope fwd", C=kr.C_ROPE)
    xf = c["dy"].float().requires_grad_(True)  # any point: the op is linear
    apply_rope_ref(xf, c["cos"], c["sin"], pos).backward(c["dy"].float())
    check(xf.grad.to(dtype), c["dx"], c["M_dx"], dtype, op="rope bwd", C=kr.C_ROPE)


@DT
@pytest.mark.parametrize("n", kr.SWIGLU_NS)
def test_eager_swiglu(n, dtype):
    from lpp_amd.ops.swiglu import swiglu_ref

    c = kr.swiglu_case(n, dtype)
    check(swiglu_ref(c["g"], c["u"]), c["y"], c["M_y"], dtype, op="swiglu y", pre=c["pre_y"])
    gf = c["g"].float().requires_grad_(True)
    uf = c["u"].float().requires_grad_(True)
    swiglu_ref(gf, uf).backward(c["dy"].float())
    check(gf.grad.to(dtype), c["dg"], c["M_dg"], dtype, op="swiglu dg", pre=c["pre_dg"])
    check(uf.grad.to(dtype), c["du"], c["M_du"], dtype, op="swiglu du", pre=c["pre_du"])


def _eager_ce(c, dtype):
    from lpp_amd.ops.cross_entropy import shifted_cross_entropy_ref

    lf = c["logits"].float().requires_grad_(True)
    loss = shifted_cross_entropy_ref(lf, c["labels"])
    (loss * kr.CE_DLOSS).backward()
    V = lf.shape[-1]
    lse = torch.logsumexp(lf.detach()[:, :-1].reshape(-1, V), dim=-1)
    return loss.detach(), lse, lf.grad.to(dtype)


@DT
@pytest.mark.parametrize("rows,V", kr.CE_SHAPES)
def test_eager_cross_entropy(rows, V, dtype):
    c = kr.ce_case(rows, V, dtype)
    loss, lse, dl = _eager_ce(c, dtype)
    check(loss, c["loss"], c["M_loss"], torch.float32, op="ce loss")
    check(lse, c["lse"], c["M_lse"], torch.float32, op="ce lse")
    check(dl, c["dlogits"], c["M_dl"], dtype, op="ce dlogits", pre=c["pre_dl"])


@DT
def test_eager_cross_entropy_single_valid(dtype):
    c = kr.ce_case(5, 1001, dtype, single_valid=True)
    assert c["n_valid"] == 1
    loss, _, dl = _eager_ce(c, dtype)
    check(loss, c["loss"], c["M_loss"], torch.float32, op="ce loss")
    check(dl, c["dlogits"], c["M_dl"], dtype, op="ce dlogits", pre=c["pre_dl"])


def _eager_adamw(numels, dtype, wd, **shard):
    from lpp_amd.optim import MixedPrecisionAdamW

    c = kr.adamw_case(numels, dtype, wd)
    params = [torch.nn.Parameter(p.clone()) for p in c["params"]]
    opt = MixedPrecisionAdamW(params, weight_decay=wd, **kr.ADAMW_HP, **shard)
    kr.run_optimizer(opt, c["grads"])
    return c, opt


@DT
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_eager_adamw(dtype, wd):
    c, opt = _eager_adamw(kr.ADAMW_NUMELS, dtype, wd)
    for i, p in enumerate(opt.params):
        check_close(opt.masters[i], c["masters"][i], op=f"adamw master[{i}]")
        check_close(opt.exp_avg[i], c["exp_avg"][i], op=f"adamw exp_avg[{i}]")
        check_close(opt.exp_avg_sq[i], c["exp_avg_sq"][i], op=f"adamw exp_avg_sq[{i}]")
        assert torch.equal(p.data, opt.masters[i].to(dtype))


@DT
def test_eager_adamw_sharded(dtype):
    n = kr.ADAMW_SHARD_TOTAL
    c, opt = _eager_adamw((n,), dtype, 0.01, shard_world=2, shard_rank=1)
    lo = n // 2
    check_close(opt.masters[0], c["masters"][0][lo:], op="adamw shard master")
    check_close(opt.exp_avg[0], c["exp_avg"][0][lo:], op="adamw shard exp_avg")
    check_close(opt.exp_avg_sq[0], c["exp_avg_sq"][0][lo:], op="adamw shard exp_avg_sq")
    assert torch.equal(opt.param_shard, opt.masters[0].to(dtype))
    # the other rank's half is untouched
    assert torch.equal(opt.flat_params[:lo], c["params"][0][:lo])


@pytest.mark.parametrize("n", kr.ACCUM_NS)
def test_eager_accum(n):
    dst, src = kr.accum_inputs(n, 1, 1)
    r, M = kr.accum_ref(dst[1:], src[1:])
    check(dst[1:] + src[1:].float(), r, M, torch.float32, op="accum", C=0.0)


# ----------------------------------------------------------------------
# (b) the bound rejects small mistakes
# ----------------------------------------------------------------------
def _rejects(*args, **kw):
    with pytest.raises(AssertionError, match="out of bound"):
        check(*args, **kw)


def test_rejects_two_ulp_fp32():
    """With an fp32 output 2 ulp is 2**-22 of the value, below C * M for any
    op that is allowed C = 2**-13; the one IEEE add of accumulate (C = 0) is
    where two fp32 ulps must show."""
    dst, src = kr.accum_inputs(1000, 1, 1)
    r, M = kr.accum_ref(dst[1:], src[1:])
    bad = (dst[1:] + src[1:].float()).double()
    bad[321] += 2.0 * kr.ulp(r[321], torch.float32)
    _rejects(bad, r, M, torch.float32, C=0.0)


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=dtype_name)
def test_rejects_two_ulp(dtype):
    c = kr.swiglu_case(2056, dtype)
    good = c["y"].to(torch.float32).to(dtype)  # one rounding of the reference
    check(good, c["y"], c["M_y"], dtype, pre=c["pre_y"])
    i = 1234
    assert abs(float(c["y"][i])) > 1e-3  # an ordinary element
    bad = good.double()
    bad[i] += 2.0 * kr.ulp(c["y"][i], dtype)
    _rejects(bad, c["y"], c["M_y"], dtype, pre=c["pre_y"])
    _rejects(bad, c["y"], c["M_y"], dtype)


def test_ulp_values():
    r = torch.tensor([1.0, 1.5, 2.0, 0.0, 3e-39, 65504.0], dtype=torch.float64)
    assert kr.ulp(r, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6,
                                                  2.0 ** -133, 2.0 ** -133, 2.0 ** 8]
    assert kr.ulp(r, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9,
                                                 2.0 ** -24, 2.0 ** -24, 2.0 ** 5]
    assert kr.ulp(r[:3], torch.float32).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22]


def test_report_names_the_element():
    r = torch.zeros(3, 4, dtype=torch.float64) + 1.0
    k = r.clone()
    k[2, 1] = 1.0 + 3 * 2.0 ** -7
    with pytest.raises(AssertionError) as e:
        check(k, r, r.abs(), torch.bfloat16, op="demo")
    msg = str(e.value)
    assert "demo [bfloat16] shape (3, 4)" in msg and "row 2, col 1" in msg
    assert "3.000 ulp_T" in msg and "flat index 9" in msg


@DT
def test_rejects_dropped_dw_row(dtype):
    c = kr.rmsnorm_case(2085, 2048, dtype)
    x = c["x"].double()
    d = c["dys"][0].double()
    inv = c["inv"]
    row = 2084  # the second row of the block that loops
    bad = c["dw"] - d[row] * x[row] * inv[row]
    check(c["dw"].float(), c["dw"], c["M_dw"], torch.float32)
    _rejects(bad.float(), c["dw"], c["M_dw"], torch.float32)


@DT
def test_rejects_rope_sin_sign(dtype):
    shape = kr.ROPE_SHAPES[2]
    B, S, H, D, pos, length = shape
    c = kr.rope_case(*shape, dtype)
    sin = c["sin"].clone()
    sin[pos + 4] = -sin[pos + 4]
    bad, _ = kr.rope_ref(c["x"], c["cos"], sin, pos)
    _rejects(bad.float().to(dtype), c["y"], c["M_y"], dtype, C=kr.C_ROPE)


@DT
def test_rejects_ce_onehot_off_by_one(dtype):
    c = kr.ce_case(5, 1000, dtype)
    shifted = c["labels"].clone()
    live = shifted[0, 1:] >= 0
    shifted[0, 1:][live] = (shifted[0, 1:][live] + 1) % 1000
    bad = kr.ce_ref(c["logits"], shifted, kr.CE_DLOSS)["dlogits"]
    _rejects(bad.float().to(dtype), c["dlogits"], c["M_dl"], dtype, pre=c["pre_dl"])


@DT
def test_rejects_ce_mean_over_all_rows(dtype):
    c = kr.ce_case(5, 1000, dtype)
    rows = c["valid"].numel()
    assert c["n_valid"] < rows
    bad = c["loss"] * c["n_valid"] / rows
    _rejects(bad.float(), c["loss"], c["M_loss"], torch.float32)


@pytest.mark.parametrize("mistake", ["no_bias_correction", "decay_on_grad"])
def test_rejects_adamw_mistakes(mistake):
    numels = (1023,)
    c = kr.adamw_case(numels, torch.float32, 0.01)
    params, grads = kr.adamw_inputs(numels, torch.float32)
    if mistake == "no_bias_correction":
        grads = grads[:1]  # step 1
        good, _, _ = kr.adamw_ref(params, grads, weight_decay=0.01,
                                  grad_scale=kr.ADAMW_GRAD_SCALE, **kr.ADAMW_HP)
        bad, _, _ = kr.adamw_ref(params, grads, weight_decay=0.01, bias_correction=False,
                                 grad_scale=kr.ADAMW_GRAD_SCALE, **kr.ADAMW_HP)
    else:
        good = c["masters"]
        bad, _, _ = kr.adamw_ref(params, grads, weight_decay=0.01, decay_on_grad=True,
                                 grad_scale=kr.ADAMW_GRAD_SCALE, **kr.ADAMW_HP)
    check_close(good[0].float(), good[0])
    with pytest.raises(AssertionError, match="out of bound"):
        check_close(bad[0].float(), good[0])


@DT
def test_rejects_swiglu_dsilu_as_s(dtype):
    c = kr.swiglu_case(2056, dtype)
    s = torch.sigmoid(c["g"].double())
    bad = c["dy"].double() * c["u"].double() * s
    _rejects(bad.float().to(dtype), c["dg"], c["M_dg"], dtype, pre=c["pre_dg"])
