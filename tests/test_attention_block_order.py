"""Host-side checks of the attention block-order function (attn_order.h).

``attention_block_order`` evaluates on the CPU the same header function the
forward, dQ and dK/dV kernels run on the device, so what passes here is the
order the kernels launch with.  Needs the built extension, no GPU.
"""

import pytest
import torch

from lpp_amd.ops import build as kbuild

FWD_DQ, DKDV = 0, 1


@pytest.fixture(scope="module")
def ext():
    if not (kbuild.OUT_DIR / kbuild.SO_NAME).exists():
        pytest.skip("HIP extension not built (run __graft_entry__.build())")
    from lpp_amd import ops

    e = ops._load_extension()
    if e is None:
        pytest.skip(f"HIP extension does not import here: {ops._EXT_ERR}")
    return e


def _work(kind, nblk, blk):
    return blk + 1 if kind == FWD_DQ else nblk - blk


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", [FWD_DQ, DKDV])
def test_order_is_a_permutation(ext, kind, mode):
    for nblk in (1, 2, 3, 5, 16, 32, 64):
        for nheads in (1, 3, 8, 15, 64, 256):
            n = nblk * nheads
            for G in (1, 2, 4, nheads, nheads + 3):
                bh = ext.attention_block_order(kind, nblk, nheads, G, mode).long()
                assert bh.shape == (n, 2) and bh.dtype == torch.int64
                blk, head = bh[:, 0], bh[:, 1]
                assert blk.min() >= 0 and blk.max() < nblk, (nblk, nheads, G)
                assert head.min() >= 0 and head.max() < nheads, (nblk, nheads, G)
                flat = (head * nblk + blk).sort().values
                assert torch.equal(flat, torch.arange(n)), (nblk, nheads, G)


@pytest.mark.parametrize("kind", [FWD_DQ, DKDV])
def test_mode0_is_the_2d_grid_order(ext, kind):
    for nblk, nheads in ((1, 3), (5, 15), (16, 256), (32, 8)):
        bh = ext.attention_block_order(kind, nblk, nheads, 4, 0).long()
        L = torch.arange(nblk * nheads)
        assert torch.equal(bh[:, 0], L % nblk)
        assert torch.equal(bh[:, 1], L // nblk)


# the production launches at S=4096, B=4, H=64: (kind, nblk, nheads, G)
PRODUCTION = [(FWD_DQ, 16, 256, 4), (DKDV, 32, 256, 2)]


@pytest.mark.parametrize("kind,nblk,nheads,G", PRODUCTION)
def test_mode1_balances_the_xcd_labels(ext, kind, nblk, nheads, G):
    bh = ext.attention_block_order(kind, nblk, nheads, G, 1).long()
    work = _work(kind, nblk, bh[:, 0])
    per_label = [int(work[k::8].sum()) for k in range(8)]
    assert len(set(per_label)) == 1, per_label
    assert per_label[0] * 8 == nheads * nblk * (nblk + 1) // 2


@pytest.mark.parametrize("kind,nblk,nheads,G", PRODUCTION)
def test_mode1_runs_heavy_blocks_first_per_group(ext, kind, nblk, nheads, G):
    bh = ext.attention_block_order(kind, nblk, nheads, G, 1).long()
    for k in range(8):
        blk, head = bh[k::8, 0], bh[k::8, 1]
        work = _work(kind, nblk, blk)
        grp = head // G
        for g in grp.unique().tolist():
            w = work[grp == g]
            assert w.numel() == G * nblk  # a label works through whole groups
            assert bool((w[1:] <= w[:-1]).all()), (k, g, w.tolist())
