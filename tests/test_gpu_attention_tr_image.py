"""The attention kernels' B-fragments as they read them from the dual-use LDS
image (csrc/attn_tile.h): one workgroup stages a [64][128] tile with the
kernels' ds_write_b128 staging and reads every fragment back with the
kernels' ds_read_b64_tr_b16 address functions (pytest -m gpu).  Exact: the
reads move bits."""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from lpp_amd import ops

    return ops.extension()


@pytest.fixture(scope="module")
def tile():
    """8192 distinct int16 values, not a linear ramp in either index."""
    g = torch.Generator().manual_seed(77)
    vals = torch.randperm(64 * 128, generator=g) - 4096
    return vals.to(torch.int16).view(64, 128).cuda()


def _want(tile, shape):
    """[16, 64, 8] = tile[k, n] by the MFMA B-operand maps:
    32x32x16, frag = dt*4 + ks:   k = ks*16 + (lane>>5)*8 + j,   n = dt*32 + (lane&31)
    16x16x32, frag = dt*2 + half: k = half*32 + (lane>>4)*8 + j, n = dt*16 + (lane&15)"""
    dev = tile.device
    frag = torch.arange(16, device=dev).view(16, 1, 1)
    lane = torch.arange(64, device=dev).view(1, 64, 1)
    j = torch.arange(8, device=dev).view(1, 1, 8)
    if shape == 32:
        k = (frag & 3) * 16 + (lane >> 5) * 8 + j
        n = (frag >> 2) * 32 + (lane & 31)
    else:
        k = (frag & 1) * 32 + (lane >> 4) * 8 + j
        n = (frag >> 1) * 16 + (lane & 15)
    k, n = torch.broadcast_tensors(k, n)
    return tile[k, n]


@pytest.mark.parametrize("buf", [0, 1])
@pytest.mark.parametrize("shape", [32, 16])
def test_fragments_equal_operand_map(ext, tile, shape, buf):
    got = ext.attn_tile_test_tr_fragments(tile, shape, 64, buf)
    assert got.shape == (16, 64, 8) and got.dtype == torch.int16
    assert torch.equal(got, _want(tile, shape))


@pytest.mark.parametrize("shape", [32, 16])
@pytest.mark.parametrize("nrows", [1, 37])
def test_clamped_rows(ext, tile, shape, nrows):
    """Rows past the sequence end are staged as copies of the last row (the
    kernels' clamped loads): nrows = 1 is the S = 1 tile, all one row."""
    clamped = tile[torch.arange(64, device=tile.device).clamp(max=nrows - 1)]
    got = ext.attn_tile_test_tr_fragments(tile, shape, nrows, 1)
    assert torch.equal(got, _want(clamped, shape))


def test_round_trip_from_one_image(ext, tile):
    """The tile through row reads and its transpose through transposed reads,
    both from the same image."""
    normal, transposed = ext.attn_tile_test_roundtrip(tile)
    assert torch.equal(normal, tile)
    assert torch.equal(transposed, tile.t().contiguous())
