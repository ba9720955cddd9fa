"""Attention block order on the GPU: modes 0 and 1 must agree bit for bit.

The order only changes which workgroup computes which tile (attn_order.h),
so forward and backward outputs are compared with ``torch.equal``, and mode 1
is held to the fp32 reference at the tolerances of test_gpu_attention.py.
"""

import functools
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests.test_gpu_attention import _ref_attn, _ref_attn_grads

pytestmark = pytest.mark.gpu

REPO_ROOT = Path(__file__).resolve().parent.parent

# (B, H, HKV, S)
SHAPES = {
    "n_not_multiple_of_8": (1, 3, 3, 200),  # forward has nblk = 1
    "short_last_group": (3, 5, 5, 640),  # 15 heads, ragged last block
    "gqa": (2, 8, 2, 384),  # dK/dV maps over B*HKV = 4
    "aligned": (1, 16, 16, 1024),  # n a multiple of 8
}
NAMES = ("o", "lse2", "dq", "dk", "dv")


def _inputs(B, H, HKV, S):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000 * B + 10 * H + S)
    q = torch.randn(B, S, H, 128, device=dev, dtype=torch.bfloat16, generator=g)
    k = torch.randn(B, S, HKV, 128, device=dev, dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, S, HKV, 128, device=dev, dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, S, H, 128, device=dev, dtype=torch.bfloat16, generator=g)
    return q, k, v, do


def _run_mode(ext, mode, q, k, v, do):
    """(o, lse2, dq, dk, dv) under `mode`; the mode in force before is restored."""
    before = ext.attention_get_block_order()
    ext.attention_set_block_order(mode)
    try:
        o, lse2 = ext.attention_fwd(q, k, v)
        dq, dk, dv = ext.attention_bwd(do, q, k, v, o, lse2)
        torch.cuda.synchronize()
    finally:
        ext.attention_set_block_order(before)
    return o, lse2, dq, dk, dv


@functools.lru_cache(maxsize=None)
def _both_modes(name):
    from lpp_amd import ops

    ext = ops.extension()
    inputs = _inputs(*SHAPES[name])
    return inputs, _run_mode(ext, 0, *inputs), _run_mode(ext, 1, *inputs)


def _mismatches(name):
    _, legacy, remapped = _both_modes(name)
    return [n for n, a, b in zip(NAMES, legacy, remapped) if not torch.equal(a, b)]


def test_default_mode_is_1():
    from lpp_amd import ops

    if os.environ.get("LPP_ATTN_ORDER") is None:
        assert ops.extension().attention_get_block_order() == 1


@pytest.mark.parametrize("name", list(SHAPES))
def test_modes_agree_bit_for_bit(name):
    from lpp_amd import ops

    assert _mismatches(name) == []
    assert ops.extension().attention_get_block_order() == 1


def test_mode1_matches_fp32_reference():
    (q, k, v, do), _, (o, _lse2, dq, dk, dv) = _both_modes("short_last_group")
    ref = _ref_attn(q, k, v)
    assert (o.float() - ref).abs().max() < 3e-2
    rdq, rdk, rdv = _ref_attn_grads(q, k, v, do)
    for got, refg, gname in ((dq, rdq, "dq"), (dk, rdk, "dk"), (dv, rdv, "dv")):
        err = (got.float() - refg).abs().max()
        den = refg.abs().max().clamp(min=1.0)
        assert err / den < 4e-2, f"{gname} rel err {err / den} (abs {err})"


def test_modes_agree_double_buffered_variants():
    """LPP_ATTN_DBUF is read once per process, so the double-buffered dQ and
    dK/dV kernels (32 resident blocks per XCD, another G) run in a child."""
    code = (
        "import sys; sys.path.insert(0, sys.argv[1])\n"
        "from tests.test_gpu_attention_order import _mismatches\n"
        "bad = _mismatches('short_last_group')\n"
        "print('MISMATCH', bad)\n"
        "sys.exit(1 if bad else 0)\n"
    )
    env = dict(os.environ, LPP_ATTN_DBUF="1")
    env.pop("LPP_ATTN_ORDER", None)
    r = subprocess.run([sys.executable, "-c", code, str(REPO_ROOT)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "MISMATCH []" in r.stdout
