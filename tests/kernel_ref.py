"""Float64 oracle and error-bound checker for the fused row / elementwise
kernels (rmsnorm, rope, swiglu, shifted cross entropy, AdamW, accumulate).

Every reference here is written from the maths in float64 and calls none of
the project's ``*_ref`` functions nor the ``_foreach`` optimizer, so the eager
path can itself be checked against it (tests/test_kernel_ref_cpu.py) before
the HIP kernels are (tests/test_gpu_fused_ops_ref.py).

A reference returns, for each output, the float64 value ``r`` and a magnitude
``M`` of the same shape: the float64 sum of the absolute values of the terms
that the last add / subtract / reduction combines (for a pure product, ``|r|``).
``check`` then asserts

    |k - r| <= 0.5 * ulp_T(r) + C * M            C = 2**-13 unless stated

The first term is the one rounding to the output dtype ``T``.  The second
bounds the fp32 arithmetic in front of it:

* a thread adds at most 2**9 terms in sequence in any of these kernels
  (V = 128256 over 256 threads in cross entropy is the longest); each add
  rounds by 2**-24 of the running sum, which is <= M: 2**9 * 2**-24 = 2**-15;
  the wave / block trees and the <= 2**11 fp32 atomics or partial rows behind
  them add log-depth or, for the loss atomics, at most 2**11 * 2**-24 = 2**-13
  in the worst case on a sum of same-sign terms that M bounds from above;
* ``__expf(x)`` is ``exp2(x * log2(e))``: the product's rounding is
  2**-24 * |x| * log2(e) in the exponent, i.e. a relative 2**-24 * |x| in the
  result, 2**-17 at |x| = 128;
* the remaining handful of fp32 multiplies, one divide and one rsqrt / log
  at <= 2 ulp each stay below 2**-20.

Where M as defined above misses a term that fp32 demonstrably loses, the
reference says so next to the line that adds it (``+ 1`` in the logsumexp,
the whole ``sum |dy w x|`` in the rmsnorm dx).  ``pre`` is an absolute error
that is present before the final rounding and does not scale with M: the
2**-126 below which an fp32 intermediate flushes to zero (sigmoid(-90),
exp(x - lse) of a far-away logit), and the extra output rounding of the
fused rmsnorm backward.
"""

from __future__ import annotations

import functools
import math

import torch

C_DEFAULT = 2.0 ** -13
# rope: out = a*c -+ b*s is two fp32 products (2**-24 of |a c| and |b s| each,
# together <= 2**-24 * M) and the final add, which is the output rounding that
# the 0.5 ulp term already counts when T is fp32 and 2**-24 * |r| otherwise.
# 2**-23 * M in all; 2**-22 leaves one bit for an unfused multiply-add order.
C_ROPE = 2.0 ** -22
FP32_TINY = 2.0 ** -126

_FMT = {  # dtype -> (explicit mantissa bits, minimum normal exponent)
    torch.bfloat16: (7, -126),
    torch.float16: (10, -14),
    torch.float32: (23, -126),
}

SPECIALS = (0.0, -0.0, 2.0 ** -10, -(2.0 ** -10), 20.0, -20.0, 90.0, -90.0)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def dtype_name(dt) -> str:
    return str(dt).replace("torch.", "")


# --------------------------------------------------------------------------
# ulp and check
# --------------------------------------------------------------------------
def ulp(r: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of ``dtype`` at |r| (float64), with the subnormal floor."""
    mant, emin = _FMT[dtype]
    r = r.double().abs()
    _, e = torch.frexp(r)  # r = m * 2**e, m in [0.5, 1)
    e = torch.where(r == 0, torch.full_like(e, emin), e - 1)
    e = e.clamp(min=emin) - mant
    return torch.ldexp(torch.ones_like(r), e)


def _report(op, dtype, k, r, err, tol, unit):
    shape = tuple(r.shape)
    bad = err > tol
    over = torch.where(bad, err - tol, torch.zeros_like(err))
    flat = int(over.reshape(-1).argmax())
    cols = shape[-1] if len(shape) else 1
    row, col = divmod(flat, cols)
    kv = float(k.reshape(-1)[flat])
    rv = float(r.reshape(-1)[flat])
    u = float(unit.reshape(-1)[flat])
    return (f"{op} [{dtype_name(dtype)}] shape {shape}: {int(bad.sum())} of {r.numel()} "
            f"elements out of bound; worst flat index {flat} (row {row}, col {col}): "
            f"k={kv!r} r={rv!r} |k-r|={abs(kv - rv):.6g} = {abs(kv - rv) / u:.3f} ulp_T, "
            f"allowed {float(tol.reshape(-1)[flat]):.6g} = "
            f"{float(tol.reshape(-1)[flat]) / u:.3f} ulp_T")


def check(k, r, M, dtype, *, op="op", C=C_DEFAULT, pre=None):
    """Assert |k - r| <= 0.5 * ulp_T(r) + C * M elementwise.

    ``pre`` (float64, broadcastable) is an absolute error already present in
    the value that the kernel rounds to T.  The rounded value may then sit
    up to ``pre`` away from r, possibly in the next binade, so the rounding
    term is taken at |r| + pre + C*M and ``pre`` itself is added."""
    k = torch.as_tensor(k).detach().cpu().double()
    r = torch.as_tensor(r).double()
    M = torch.as_tensor(M).double().expand_as(r)
    assert k.shape == r.shape, f"{op}: shape {tuple(k.shape)} vs reference {tuple(r.shape)}"
    assert bool(torch.isfinite(r).all()), f"{op}: reference not finite"
    if pre is None:
        tol = 0.5 * ulp(r, dtype) + C * M
    else:
        slack = C * M + torch.as_tensor(pre).double().expand_as(r)
        tol = 0.5 * ulp(r.abs() + slack, dtype) + slack
    err = (k - r).abs()
    err = torch.where(torch.isfinite(k), err, torch.full_like(err, math.inf))
    if bool((err > tol).any()):
        raise AssertionError(_report(op, dtype, k, r, err, tol, ulp(r, dtype)))


def check_close(k, r, dtype=torch.float32, *, op="op", rtol=1e-5, atol=1e-5):
    """|k - r| <= atol + rtol * |r| with check's failure report (the AdamW
    fp32 master / moment comparison the suite already uses)."""
    k = torch.as_tensor(k).detach().cpu().double()
    r = torch.as_tensor(r).double()
    assert k.shape == r.shape, f"{op}: shape {tuple(k.shape)} vs reference {tuple(r.shape)}"
    tol = atol + rtol * r.abs()
    err = (k - r).abs()
    err = torch.where(torch.isfinite(k), err, torch.full_like(err, math.inf))
    if bool((err > tol).any()):
        raise AssertionError(_report(op, dtype, k, r, err, tol, ulp(r, dtype)))


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def special_indices(numel: int):
    """Flat indices that hold SPECIALS[i] (later ones win on a collision)."""
    return [(3 + 7919 * i) % numel for i in range(len(SPECIALS))]


def make_values(shape, dtype, seed, scale=4.0, specials=True) -> torch.Tensor:
    """scale * randn in ``dtype`` with SPECIALS spliced in at known indices."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype)
    if specials:
        flat = x.view(-1)
        for i, s in zip(special_indices(flat.numel()), SPECIALS):
            flat[i] = s
    return x


# --------------------------------------------------------------------------
# rmsnorm
# --------------------------------------------------------------------------
def rmsnorm_fwd_ref(x, w, eps):
    """x [rows, H] (any float dtype), w [H].  Returns (y, M_y, inv, M_inv)."""
    x = x.double()
    w = w.double()
    inv = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    y = x * inv * w
    return y, y.abs(), inv.squeeze(-1), inv.squeeze(-1).abs()


def sum_partials(dys):
    """The fused backward's dy: partials added in list order in fp32 with a
    rounding to T after each add (an fp32 add of two T values followed by
    the conversion, which is what the separate elementwise adds do)."""
    d = dys[0]
    for p in dys[1:]:
        d = (d.float() + p.float()).to(d.dtype)
    return d


def rmsnorm_bwd_ref(dys, x, w, eps, dres=None):
    """Returns (dx, M_dx, pre_dx, dw, M_dw).

    dx = dy w inv - x inv^3/H sum_j(dy_j w_j x_j);  dw = sum_rows dy x inv.
    M_dx carries the whole sum_j |dy_j w_j x_j| behind the second term: the
    row dot cancels, and what fp32 loses in it is relative to that sum, not
    to the dot.  With ``dres`` the kernel rounds dx to T, adds dres and
    rounds again; r is the exact dx + dres and ``pre_dx`` is the first
    rounding, 0.5 ulp_T(dx) (None without dres)."""
    T = x.dtype
    d = sum_partials(list(dys)).double()
    x = x.double()
    w = w.double()
    H = x.shape[-1]
    inv = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    t = d * w * x
    dot = t.sum(-1, keepdim=True)
    a = d * w * inv
    coef = x * inv ** 3 / H
    dx = a - coef * dot
    M_dx = a.abs() + coef.abs() * t.abs().sum(-1, keepdim=True)
    terms = d * x * inv
    dw = terms.sum(0)
    M_dw = terms.abs().sum(0)
    pre = None
    if dres is not None:
        pre = 0.5 * ulp(dx, T)
        dx = dx + dres.double()
        M_dx = M_dx + dres.double().abs()
    return dx, M_dx, pre, dw, M_dw


# --------------------------------------------------------------------------
# rope
# --------------------------------------------------------------------------
def rope_table(length, D, theta=10000.0):
    """fp32 cos / sin [length, D/2] (angles in float64, rounded once)."""
    inv_freq = theta ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.outer(torch.arange(length, dtype=torch.float64), inv_freq)
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def rope_ref(x, cos, sin, pos_offset, backward=False):
    """x [B, S, H, D], rotate_half pairs (d, d + D/2).  Backward is the
    rotation by the negated angle.  Returns (y, M)."""
    B, S, H, D = x.shape
    h = D // 2
    c = cos[pos_offset:pos_offset + S].double().view(1, S, 1, h)
    s = sin[pos_offset:pos_offset + S].double().view(1, S, 1, h)
    if backward:
        s = -s
    x = x.double()
    a, b = x[..., :h], x[..., h:]
    y = torch.cat((a * c - b * s, b * c + a * s), dim=-1)
    M = torch.cat(((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()), dim=-1)
    return y, M


# --------------------------------------------------------------------------
# swiglu
# --------------------------------------------------------------------------
def swiglu_fwd_ref(g, u):
    """y = g sigmoid(g) u.  Returns (y, M, pre); pre = 2**-126 |g u| is the
    sigmoid that fp32 flushes to zero below its smallest normal."""
    g = g.double()
    u = u.double()
    y = g * torch.sigmoid(g) * u
    return y, y.abs(), FP32_TINY * (g * u).abs()


def swiglu_bwd_ref(dy, g, u):
    """dg = dy u s (1 + g (1 - s)), du = dy g s.
    Returns (dg, M_dg, pre_dg, du, M_du, pre_du).  M_dg sums the two terms
    of the bracket, which cancel at g = -1.278."""
    dy = dy.double()
    g = g.double()
    u = u.double()
    s = torch.sigmoid(g)
    one_minus_s = torch.sigmoid(-g)
    dg = dy * u * s * (1.0 + g * one_minus_s)
    M_dg = (dy * u).abs() * s * (1.0 + g.abs() * one_minus_s)
    pre_dg = FP32_TINY * (dy * u).abs() * (1.0 + g.abs())
    du = dy * g * s
    return dg, M_dg, pre_dg, du, du.abs(), FP32_TINY * (dy * g).abs()


# --------------------------------------------------------------------------
# shifted cross entropy
# --------------------------------------------------------------------------
def ce_ref(logits, labels, dloss=1.0, ignore_index=-100):
    """logits [B, S, V], labels [B, S]; position t predicts token t+1, mean
    over the targets that are not ``ignore_index``.

    Returns a dict: loss, M_loss (scalars), lse, M_lse ([B*(S-1)]), dlogits,
    M_dl, pre_dl ([B, S, V]; dlogits is d(dloss * loss)/dlogits), valid
    ([B*(S-1)] bool), n_valid.

    M_lse = |max| + |log sum| + 1: the error of log(sum) is the *relative*
    error of the sum of exponentials (an all-positive reduction), so it does
    not shrink with |log sum| when one logit dominates and the sum is ~1.
    pre_dl = 2**-126 |scale|: exp(x - lse) of a logit more than 87 below lse
    is flushed to zero in fp32."""
    B, S, V = logits.shape
    x = logits[:, :-1, :].double().reshape(-1, V)
    lab = labels[:, 1:].reshape(-1)
    valid = lab != ignore_index
    n = int(valid.sum())
    m = x.max(-1).values
    ssum = torch.exp(x - m[:, None]).sum(-1)
    lse = m + torch.log(ssum)
    M_lse = m.abs() + torch.log(ssum).abs() + 1.0
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    gold = x.gather(1, safe[:, None]).squeeze(1)
    denom = max(n, 1)
    loss = torch.where(valid, lse - gold, torch.zeros_like(lse)).sum() / denom
    M_loss = torch.where(valid, M_lse + gold.abs(), torch.zeros_like(lse)).sum() / denom
    scale = float(dloss) / denom
    sm = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, safe[:, None], 1.0)
    d2 = scale * (sm - onehot) * valid[:, None]
    M2 = abs(scale) * (sm + onehot) * valid[:, None]
    dl = torch.zeros(B, S, V, dtype=torch.float64)
    M_dl = torch.zeros(B, S, V, dtype=torch.float64)
    dl[:, :-1] = d2.view(B, S - 1, V)
    M_dl[:, :-1] = M2.view(B, S - 1, V)
    return dict(loss=loss, M_loss=M_loss, lse=lse, M_lse=M_lse, dlogits=dl, M_dl=M_dl,
                pre_dl=FP32_TINY * abs(scale), valid=valid, n_valid=n)


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------
def adamw_ref(masters, grads_per_step, lr, betas, eps, weight_decay, grad_scale,
              decay_on_grad=False, bias_correction=True):
    """Float64 AdamW over a list of tensors: decoupled decay on the master,
    bias-corrected moments, gradients multiplied by ``grad_scale``.
    ``grads_per_step`` is [step][tensor].  Returns (masters, exp_avg,
    exp_avg_sq).  The two switches exist for the tests that show the
    comparison rejects the two classic mistakes."""
    b1, b2 = betas
    w = [t.double().clone() for t in masters]
    m = [torch.zeros_like(t) for t in w]
    v = [torch.zeros_like(t) for t in w]
    for step, grads in enumerate(grads_per_step, start=1):
        bias1 = 1.0 - b1 ** step if bias_correction else 1.0
        bias2 = 1.0 - b2 ** step if bias_correction else 1.0
        for i, g in enumerate(grads):
            g = g.double() * grad_scale
            if decay_on_grad:
                g = g + weight_decay * w[i]
            else:
                w[i] = w[i] * (1.0 - lr * weight_decay)
            m[i] = b1 * m[i] + (1.0 - b1) * g
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            w[i] = w[i] - (lr / bias1) * m[i] / (torch.sqrt(v[i] / bias2) + eps)
    return w, m, v


# --------------------------------------------------------------------------
# accumulate
# --------------------------------------------------------------------------
def accum_ref(dst, src):
    """dst + src.  Returns (r, M)."""
    return dst.double() + src.double(), dst.double().abs() + src.double().abs()


# --------------------------------------------------------------------------
# the case matrix (shared by the CPU honesty tests and the GPU tests)
# --------------------------------------------------------------------------
EPS = 1e-6

# (rows, H): N_IT=1; N_IT=3; vectorised row loop + dw registers; LDS fallback
# row loop + LDS dw; scalar forward row loop; forward row loop (> 4096); tiny.
RMSNORM_SHAPES = ((3, 2048), (3, 6144), (2085, 2048), (1061, 5120), (1061, 100),
                  (4133, 256), (5, 8))


@functools.lru_cache(maxsize=None)
def rmsnorm_case(rows, H, dtype, n_dy=1, with_res=False):
    """Inputs and float64 references of one rmsnorm case (shared, read-only)."""
    seed = 1000 + rows * 7 + H
    x = make_values((rows, H), dtype, seed, scale=6.0)
    w = make_values((H,), torch.float32, seed + 1, scale=1.0, specials=False)
    dys = tuple(make_values((rows, H), dtype, seed + 2 + i, scale=4.0) for i in range(n_dy))
    dres = make_values((rows, H), dtype, seed + 9, scale=4.0) if with_res else None
    y, M_y, inv, M_inv = rmsnorm_fwd_ref(x, w, EPS)
    dx, M_dx, pre_dx, dw, M_dw = rmsnorm_bwd_ref(dys, x, w, EPS, dres)
    return dict(x=x, w=w, dys=dys, dres=dres, y=y, M_y=M_y, inv=inv, M_inv=M_inv,
                dx=dx, M_dx=M_dx, pre_dx=pre_dx, dw=dw, M_dw=M_dw)


# (B, S, H, D, pos_offset, table length).  The [1, 2048, 17, 128] case has
# 557056 packets against the 524288-thread grid; its offset ends exactly at
# the table's last row.
ROPE_SHAPES = ((2, 5, 3, 8, 3, 16), (2, 7, 3, 64, 0, 7), (1, 9, 2, 72, 5, 20),
               (1, 2048, 17, 128, 5, 2053))


@functools.lru_cache(maxsize=None)
def rope_case(B, S, H, D, pos, length, dtype):
    x = make_values((B, S, H, D), dtype, 2000 + D + S, scale=4.0)
    dy = make_values((B, S, H, D), dtype, 2001 + D + S, scale=8.0)
    cos, sin = rope_table(length, D)
    y, M_y = rope_ref(x, cos, sin, pos)
    dx, M_dx = rope_ref(dy, cos, sin, pos, backward=True)
    return dict(x=x, dy=dy, cos=cos, sin=sin, y=y, M_y=M_y, dx=dx, M_dx=M_dx)


SWIGLU_NS = (8, 2056, 2059)  # 2059: ragged for every pack width


@functools.lru_cache(maxsize=None)
def swiglu_case(n, dtype):
    g = make_values((n,), dtype, 3000 + n, scale=4.0)
    u = make_values((n,), dtype, 3001 + n, scale=4.0)
    dy = make_values((n,), dtype, 3002 + n, scale=4.0)
    y, M_y, pre_y = swiglu_fwd_ref(g, u)
    dg, M_dg, pre_dg, du, M_du, pre_du = swiglu_bwd_ref(dy, g, u)
    return dict(g=g, u=u, dy=dy, y=y, M_y=M_y, pre_y=pre_y, dg=dg, M_dg=M_dg,
                pre_dg=pre_dg, du=du, M_du=M_du, pre_du=pre_du)


# (rows, V) of the shifted problem: logits are [1, rows + 1, V].
CE_SHAPES = ((5, 8), (5, 1000), (5, 1001), (5, 130), (5, 2056), (3, 128256), (2085, 1000))
CE_DLOSS = 3.0


def ce_labels(rows, V, logits, single_valid=False):
    """Targets of the shifted rows: column 0, V-1, the argmax of a row whose
    one logit is 60 above the rest, a run of -100, then a fixed pattern."""
    g = torch.Generator().manual_seed(4000 + rows + V)
    lab = torch.randint(0, V, (rows,), generator=g)
    lab[0] = 0
    lab[1] = V - 1
    lab[2] = int(logits[0, 2].argmax())
    if rows > 3:
        lab[3:5] = -100
    if rows > 64:
        lab[40:64] = -100
        lab[rows - 3:] = -100
    if single_valid:
        keep = int(lab[1])
        lab[:] = -100
        lab[1] = keep
    labels = torch.full((1, rows + 1), -100, dtype=torch.long)
    labels[0, 1:] = lab
    # labels[0, 0] is shifted out; give it a real token so that it would show
    labels[0, 0] = 1
    return labels


@functools.lru_cache(maxsize=None)
def ce_case(rows, V, dtype, single_valid=False):
    logits = make_values((1, rows + 1, V), dtype, 4000 + rows * 3 + V, scale=4.0)
    # row 2: one logit 60 above a flat rest
    hot = (7 * V) // 11
    logits[0, 2] = make_values((V,), dtype, 4100 + V, scale=0.5, specials=False)
    logits[0, 2, hot] = 60.0
    labels = ce_labels(rows, V, logits, single_valid)
    ref = ce_ref(logits, labels, CE_DLOSS)
    return dict(logits=logits, labels=labels, **ref)


ADAMW_NUMELS = (3, 5, 1, 1023, 4, 2101255)
ADAMW_STEPS = 3
ADAMW_HP = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-6)
ADAMW_GRAD_SCALE = 0.5
ADAMW_SHARD_TOTAL = 1002


def adamw_inputs(numels, dtype):
    """Initial parameters (in ``dtype``) and [step][tensor] fp32 gradients."""
    params = [make_values((n,), dtype, 5000 + i, scale=1.0, specials=False)
              for i, n in enumerate(numels)]
    grads = [[make_values((n,), torch.float32, 5100 + 10 * s + i, scale=4.0)
              for i, n in enumerate(numels)] for s in range(ADAMW_STEPS)]
    return params, grads


@functools.lru_cache(maxsize=None)
def adamw_case(numels, dtype, weight_decay):
    params, grads = adamw_inputs(numels, dtype)
    w, m, v = adamw_ref(params, grads, weight_decay=weight_decay,
                        grad_scale=ADAMW_GRAD_SCALE, **ADAMW_HP)
    return dict(params=params, grads=grads, masters=w, exp_avg=m, exp_avg_sq=v)


def run_optimizer(opt, grads):
    """Drive a MixedPrecisionAdamW through the case's steps: each step's
    gradients are written into the optimizer's flat buffer as one vector."""
    for step in grads:
        flat = torch.cat([g.reshape(-1) for g in step])
        opt.flat_grads[: flat.numel()].copy_(flat)
        opt.step(grad_scale=ADAMW_GRAD_SCALE)
        opt.zero_grad()


ACCUM_NS = (5, 1000, 4196709)
ACCUM_OFFSETS = ((1, 0), (2, 0), (3, 0), (0, 1), (1, 1))  # (dst floats, src elements)


def accum_inputs(n, dst_off, src_off):
    dst = make_values((n + dst_off,), torch.float32, 6000 + n, scale=4.0)
    src = make_values((n + src_off,), torch.bfloat16, 6001 + n, scale=4.0)
    return dst, src
