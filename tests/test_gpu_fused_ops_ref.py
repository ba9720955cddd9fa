"""The fused row / elementwise HIP kernels against the float64 oracle of
tests/kernel_ref.py: inputs built on the CPU from fixed seeds, reference in
float64 on the CPU, kernel on the GPU, compared with ``check``
(|k - r| <= 0.5 ulp_T(r) + 2**-13 M, see kernel_ref).  The case matrix lives
in kernel_ref so that tests/test_kernel_ref_cpu.py can hold the same cases to
the same bound through the eager path.  Shapes are the smallest that reach
each instantiation, row loop, tail and launcher branch."""

import pytest
import torch

from tests import kernel_ref as kr
from tests.kernel_ref import DTYPES, check, check_close, dtype_name

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", DTYPES, ids=dtype_name)


@pytest.fixture(scope="module")
def ext():
    from lpp_amd import ops

    return ops.extension()


def _g(t):
    return t.to("cuda")


def _offset_view(t, off=1):
    """A contiguous GPU copy of ``t`` that starts ``off`` elements into its
    storage (so it is not 16-byte aligned)."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == off
    return v


# ---------------------------------------------------------------- rmsnorm
def _check_rmsnorm(c, dtype, y, inv, dx, dw, tag):
    check(y, c["y"], c["M_y"], dtype, op=f"rmsnorm_fwd y {tag}")
    assert inv.dtype == torch.float32
    check(inv, c["inv"], c["M_inv"], torch.float32, op=f"rmsnorm_fwd inv_rms {tag}")
    check(dx, c["dx"], c["M_dx"], dtype, op=f"rmsnorm_bwd dx {tag}", pre=c["pre_dx"])
    assert dw.dtype == torch.float32
    check(dw, c["dw"], c["M_dw"], torch.float32, op=f"rmsnorm_bwd dw {tag}")


@DT
@pytest.mark.parametrize("rows,H", kr.RMSNORM_SHAPES)
def test_rmsnorm(ext, rows, H, dtype):
    c = kr.rmsnorm_case(rows, H, dtype)
    x, w, dy = _g(c["x"]), _g(c["w"]), _g(c["dys"][0])
    y, inv = ext.rmsnorm_fwd(x, w, kr.EPS)
    dx, dw = ext.rmsnorm_bwd(dy, x, w, inv)
    _check_rmsnorm(c, dtype, y, inv, dx, dw, f"({rows}, {H})")


@DT
def test_rmsnorm_fused_three_partials_and_residual(ext, dtype):
    c = kr.rmsnorm_case(2085, 2048, dtype, n_dy=3, with_res=True)
    x, w = _g(c["x"]), _g(c["w"])
    y, inv = ext.rmsnorm_fwd(x, w, kr.EPS)
    dx, dw, dxT = ext.rmsnorm_bwd_fused([_g(d) for d in c["dys"]], x, w, inv,
                                        _g(c["dres"]), False)
    assert dxT.numel() == 0
    _check_rmsnorm(c, dtype, y, inv, dx, dw, "fused (2085, 2048)")


@DT
def test_rmsnorm_views_at_storage_offset_one(ext, dtype):
    """x and dy start one element into their storage: no 16-byte packets."""
    c = kr.rmsnorm_case(3, 2048, dtype)
    x, dy, w = _offset_view(c["x"]), _offset_view(c["dys"][0]), _g(c["w"])
    y, inv = ext.rmsnorm_fwd(x, w, kr.EPS)
    dx, dw = ext.rmsnorm_bwd(dy, x, w, inv)
    _check_rmsnorm(c, dtype, y, inv, dx, dw, "offset-1 views (3, 2048)")


# ---------------------------------------------------------------- rope
@DT
@pytest.mark.parametrize("shape", kr.ROPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rope(ext, shape, dtype):
    B, S, H, D, pos, length = shape
    c = kr.rope_case(*shape, dtype)
    cos, sin = _g(c["cos"]), _g(c["sin"])
    y = ext.rope_fwd(_g(c["x"]), cos, sin, pos)
    check(y, c["y"], c["M_y"], dtype, op=f"rope_fwd {shape}", C=kr.C_ROPE)
    dx = ext.rope_bwd(_g(c["dy"]), cos, sin, pos)
    check(dx, c["dx"], c["M_dx"], dtype, op=f"rope_bwd {shape}", C=kr.C_ROPE)
    # the tiled backward (bf16, D = 128, tokens % 64 == 0) or its fallback
    out = ext.rope_bwd_t(_g(c["dy"]), cos, sin, pos)
    check(out[0], c["dx"], c["M_dx"], dtype, op=f"rope_bwd_t {shape}", C=kr.C_ROPE)
    if len(out) == 2:
        assert torch.equal(out[1], out[0].view(B * S, H * D).t())


def test_rope_rejects_bad_tables(ext):
    B, S, H, D = 1, 6, 2, 16
    x = torch.zeros(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    cos, sin = (_g(t) for t in kr.rope_table(8, D))
    ext.rope_fwd(x, cos, sin, 2)  # pos_offset + S == table length
    for fn in (ext.rope_fwd, ext.rope_bwd, ext.rope_bwd_t):
        with pytest.raises(RuntimeError):
            fn(x, cos, sin, -1)
        with pytest.raises(RuntimeError):
            fn(x, cos, sin, 3)  # one row short
        with pytest.raises(RuntimeError):
            fn(x, cos[:, : D // 2 - 4].contiguous(), sin[:, : D // 2 - 4].contiguous(), 0)
        with pytest.raises(RuntimeError):
            fn(x, cos, sin[:7].contiguous(), 0)
        with pytest.raises(RuntimeError):
            fn(x, cos.double(), sin.double(), 0)


# ---------------------------------------------------------------- swiglu
@DT
@pytest.mark.parametrize("n", kr.SWIGLU_NS)
def test_swiglu(ext, n, dtype):
    """n = 2059 is ragged for every dtype: the launchers must cover the tail
    (the one-element instantiation), not leave it uninitialised."""
    c = kr.swiglu_case(n, dtype)
    g, u, dy = _g(c["g"]), _g(c["u"]), _g(c["dy"])
    y = ext.swiglu_fwd(g, u)
    check(y, c["y"], c["M_y"], dtype, op=f"swiglu_fwd n={n}", pre=c["pre_y"])
    dg, du = ext.swiglu_bwd(dy, g, u)
    check(dg, c["dg"], c["M_dg"], dtype, op=f"swiglu_bwd dg n={n}", pre=c["pre_dg"])
    check(du, c["du"], c["M_du"], dtype, op=f"swiglu_bwd du n={n}", pre=c["pre_du"])
    out = ext.swiglu_bwd_t(dy, g, u)  # not tile-aligned: same kernel
    assert len(out) == 2 and torch.equal(out[0], dg) and torch.equal(out[1], du)


def test_swiglu_bwd_rejects_mismatched_dy(ext):
    g = torch.zeros(4, 16, device="cuda", dtype=torch.bfloat16)
    u = torch.zeros_like(g)
    with pytest.raises(RuntimeError):
        ext.swiglu_bwd(torch.zeros(4, 16, device="cuda", dtype=torch.float16), g, u)
    with pytest.raises(RuntimeError):
        ext.swiglu_bwd(torch.zeros(4, 8, device="cuda", dtype=torch.bfloat16), g, u)
    with pytest.raises(RuntimeError):
        ext.swiglu_bwd(torch.zeros(4, 16, device="cuda", dtype=torch.bfloat16), g,
                       torch.zeros(4, 16, device="cuda", dtype=torch.float32))


# ---------------------------------------------------------------- cross entropy
def _run_ce(ext, c, dtype, tag):
    from lpp_amd.ops.cross_entropy import shifted_cross_entropy

    logits = _g(c["logits"]).requires_grad_(True)
    labels = _g(c["labels"])
    loss = shifted_cross_entropy(logits, labels)
    (loss * kr.CE_DLOSS).backward()
    assert loss.dtype == torch.float32
    check(loss.detach(), c["loss"], c["M_loss"], torch.float32, op=f"ce loss {tag}")
    dl = logits.grad
    assert dl.dtype == dtype
    check(dl, c["dlogits"], c["M_dl"], dtype, op=f"ce dlogits {tag}", pre=c["pre_dl"])
    # ignored rows and the shifted-out last position: exactly zero
    dead = torch.ones(c["logits"].shape[1], dtype=torch.bool)
    dead[:-1] = ~c["valid"]
    assert dead[-1] and int(dead.sum()) == dead.numel() - c["n_valid"]
    assert int(torch.count_nonzero(dl[0, _g(dead)])) == 0
    V = c["logits"].shape[-1]
    loss_sum, lse, count = ext.cross_entropy_fwd(
        logits.detach()[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1))
    assert int(count) == c["n_valid"]
    check(lse, c["lse"], c["M_lse"], torch.float32, op=f"ce lse {tag}")


@DT
@pytest.mark.parametrize("rows,V", kr.CE_SHAPES)
def test_cross_entropy(ext, rows, V, dtype):
    _run_ce(ext, kr.ce_case(rows, V, dtype), dtype, f"({rows}, {V})")


@DT
def test_cross_entropy_single_valid_row(ext, dtype):
    c = kr.ce_case(5, 1001, dtype, single_valid=True)
    assert c["n_valid"] == 1
    _run_ce(ext, c, dtype, "(5, 1001) one valid row")


# ---------------------------------------------------------------- AdamW
def _run_adamw(numels, dtype, wd, **shard):
    from lpp_amd.optim import MixedPrecisionAdamW

    c = kr.adamw_case(numels, dtype, wd)
    params = [torch.nn.Parameter(_g(p)) for p in c["params"]]
    opt = MixedPrecisionAdamW(params, weight_decay=wd, **kr.ADAMW_HP, **shard)
    kr.run_optimizer(opt, c["grads"])
    return c, opt


@DT
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adamw(ext, dtype, wd):
    """[3, 5, 1] in front put every later grad view off the 16-byte grid;
    2101255 elements pass the 2048 x 256 x 4 grid once and leave a tail."""
    c, opt = _run_adamw(kr.ADAMW_NUMELS, dtype, wd)
    assert [g.data_ptr() % 16 for g in opt.grad_views] != [0] * len(kr.ADAMW_NUMELS)
    for i, p in enumerate(opt.params):
        check_close(opt.masters[i], c["masters"][i], op=f"adamw master[{i}]")
        check_close(opt.exp_avg[i], c["exp_avg"][i], op=f"adamw exp_avg[{i}]")
        check_close(opt.exp_avg_sq[i], c["exp_avg_sq"][i], op=f"adamw exp_avg_sq[{i}]")
        assert torch.equal(p.data, opt.masters[i].to(dtype)), i


@DT
def test_fused_adamw_zero1_shard_at_odd_element(ext, dtype):
    """shard_rank 1 of 2 over 1002 elements: the shard starts at element 501
    of the grads and of the flat parameters.  No process group: the
    all-gather returns early."""
    n = kr.ADAMW_SHARD_TOTAL
    c, opt = _run_adamw((n,), dtype, 0.01, shard_world=2, shard_rank=1)
    lo = n // 2
    assert opt.grad_shard.data_ptr() % 16 != 0
    check_close(opt.masters[0], c["masters"][0][lo:], op="adamw shard master")
    check_close(opt.exp_avg[0], c["exp_avg"][0][lo:], op="adamw shard exp_avg")
    check_close(opt.exp_avg_sq[0], c["exp_avg_sq"][0][lo:], op="adamw shard exp_avg_sq")
    assert torch.equal(opt.param_shard, opt.masters[0].to(dtype))
    assert torch.equal(opt.flat_params[:lo].cpu(), c["params"][0][:lo])


# ---------------------------------------------------------------- accumulate
@pytest.mark.parametrize("n", kr.ACCUM_NS)
def test_accum_bf16_f32_views(ext, n):
    """dst views at float offsets 1, 2, 3 and src at element offset 1; the
    fp32 add of two exact values is exact IEEE, so the result is bit-equal to
    the CPU's.  The floats outside the view stay untouched."""
    for dst_off, src_off in kr.ACCUM_OFFSETS:
        dst_c, src_c = kr.accum_inputs(n, dst_off, src_off)
        want = dst_c[dst_off:] + src_c[src_off:].float()
        dst, src = _g(dst_c), _g(src_c)
        ext.accum_bf16_f32(dst[dst_off:], src[src_off:])
        assert torch.equal(dst[dst_off:].cpu(), want), (n, dst_off, src_off)
        assert torch.equal(dst[:dst_off].cpu(), dst_c[:dst_off]), (n, dst_off, src_off)
