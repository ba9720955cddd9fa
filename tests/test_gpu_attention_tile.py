"""The attention kernels' shared tile helpers (csrc/attn_tile.h), each run on
its own by a tiny test kernel in mfma_test.hip that calls the real function
(pytest -m gpu).  Every check is exact: the helpers move or round bits, they
do no arithmetic that could differ by a tolerance."""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from lpp_amd import ops

    return ops.extension()


def _dev():
    return torch.device("cuda", 0)


def test_tile_image_round_trip(ext):
    """512 threads stage a [64][128] tile of 8192 distinct values with
    stage_normal / stage_transposed under the kernels' row assignment; reading
    the images back through rswz / tswz gives the tile and its transpose."""
    tile = torch.arange(64 * 128, dtype=torch.int16, device=_dev()).view(64, 128)
    normal, transposed = ext.attn_tile_test_roundtrip(tile)
    assert normal.shape == (64, 128) and transposed.shape == (128, 64)
    assert torch.equal(normal, tile)
    assert torch.equal(transposed, tile.t().contiguous())


def test_pack_pair_fragments(ext):
    """pack_pair: p[r] = X[crow32(r, lane>>5)][lane&31] (32x32 C layout) ->
    A[m = lane&31][k = ksl*16 + (lane>>5)*8 + j] of X^T, in bf16 (RNE)."""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(32, 32, generator=g).to(_dev())
    got = ext.attn_tile_test_pack_pair(x).view(torch.bfloat16)  # [64, 2, 8]
    assert got.shape == (64, 2, 8)
    lane = torch.arange(64, device=_dev()).view(64, 1, 1)
    ksl = torch.arange(2, device=_dev()).view(1, 2, 1)
    j = torch.arange(8, device=_dev()).view(1, 1, 8)
    k = ksl * 16 + (lane >> 5) * 8 + j
    want = x.to(torch.bfloat16)[k, (lane & 31).expand_as(k)]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_pack_frag16_fragments(ext):
    """pack_frag16: p[qs][r] = X[qs*16 + (lane>>4)*4 + r][lane&15] (two 16x16
    C tiles) -> A[m = lane&15][k = (lane>>4)*8 + j] of X^T, in bf16 (RNE)."""
    g = torch.Generator().manual_seed(32)
    x = torch.randn(32, 16, generator=g).to(_dev())
    got = ext.attn_tile_test_pack_frag16(x).view(torch.bfloat16)  # [64, 8]
    assert got.shape == (64, 8)
    lane = torch.arange(64, device=_dev()).view(64, 1)
    j = torch.arange(8, device=_dev()).view(1, 8)
    k = (lane >> 4) * 8 + j
    want = x.to(torch.bfloat16)[k, (lane & 15).expand_as(k)]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
