"""Backward producers that hand the wgrad its transposed operand, and the
norm backward with the gradient adds fused in: every new output must be
bit-identical to the separate kernels it replaces (pytest -m gpu)."""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from lpp_amd import ops

    return ops.extension()


def _bf16(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda", dtype=torch.float32) * scale).to(torch.bfloat16)


# ---------------- swiglu ----------------
@pytest.mark.parametrize("T,I", [(128, 384), (64, 22016)])
def test_swiglu_bwd_t_aligned(ext, T, I):
    torch.manual_seed(1)
    dy, g, u = _bf16(T, I), _bf16(T, I, scale=2.0), _bf16(T, I)
    dg0, du0 = ext.swiglu_bwd(dy, g, u)
    out = ext.swiglu_bwd_t(dy, g, u)
    assert len(out) == 4
    dg, du, dgT, duT = out
    assert torch.equal(dg, dg0) and torch.equal(du, du0)
    assert dgT.shape == (I, T) and duT.shape == (I, T)
    assert torch.equal(dgT, dg0.t().contiguous())
    assert torch.equal(duT, du0.t().contiguous())


def test_swiglu_bwd_t_3d_input(ext):
    """[B, S, I] is flattened to [B*S, I] for the images."""
    torch.manual_seed(2)
    dy, g, u = _bf16(2, 64, 128), _bf16(2, 64, 128), _bf16(2, 64, 128)
    dg0, du0 = ext.swiglu_bwd(dy, g, u)
    dg, du, dgT, duT = ext.swiglu_bwd_t(dy, g, u)
    assert dg.shape == g.shape and torch.equal(dg, dg0) and torch.equal(du, du0)
    assert torch.equal(dgT, dg0.view(128, 128).t().contiguous())
    assert torch.equal(duT, du0.view(128, 128).t().contiguous())


def test_swiglu_bwd_t_unaligned(ext):
    torch.manual_seed(3)
    dy, g, u = _bf16(96, 200), _bf16(96, 200), _bf16(96, 200)
    dg0, du0 = ext.swiglu_bwd(dy, g, u)
    out = ext.swiglu_bwd_t(dy, g, u)
    assert len(out) == 2  # no images
    assert torch.equal(out[0], dg0) and torch.equal(out[1], du0)


# ---------------- rope ----------------
@pytest.mark.parametrize("pos_offset", [0, 5])
def test_rope_bwd_t(ext, pos_offset):
    from lpp_amd.ops.rope import build_rope_cache

    torch.manual_seed(4)
    B, S, H, D = 2, 64, 2, 128
    cos, sin = build_rope_cache(S + 8, D, 10000.0, torch.device("cuda", 0))
    dy = _bf16(B, S, H, D)
    dx0 = ext.rope_bwd(dy, cos, sin, pos_offset)
    out = ext.rope_bwd_t(dy, cos, sin, pos_offset)
    assert len(out) == 2
    dx, dxT = out
    assert torch.equal(dx, dx0)
    assert dxT.shape == (H * D, B * S)
    assert torch.equal(dxT, dx0.view(B * S, H * D).t().contiguous())


def test_rope_bwd_t_unaligned(ext):
    """D != 128 or B*S not a multiple of 64: the plain kernel, no image."""
    from lpp_amd.ops.rope import build_rope_cache

    torch.manual_seed(5)
    for B, S, H, D in ((1, 40, 2, 128), (2, 64, 2, 64)):
        cos, sin = build_rope_cache(S, D, 10000.0, torch.device("cuda", 0))
        dy = _bf16(B, S, H, D)
        out = ext.rope_bwd_t(dy, cos, sin, 0)
        assert len(out) == 1
        assert torch.equal(out[0], ext.rope_bwd(dy, cos, sin, 0))


# ---------------- fused norm backward ----------------
def _norm_case(ext, T, H, n):
    x = _bf16(T, H)
    w = (1.0 + 0.1 * torch.randn(H, device="cuda")).to(torch.bfloat16)
    _, inv = ext.rmsnorm_fwd(x, w, 1e-6)
    dys = [_bf16(T, H) for _ in range(n)]
    dres = _bf16(T, H)
    return x, w, inv, dys, dres


def _unfused(ext, dys, x, w, inv, dres):
    """The separate kernels: elementwise bf16 adds of the partials in list
    order, rmsnorm_bwd, elementwise add of the residual gradient."""
    dy = dys[0]
    for d in dys[1:]:
        dy = dy + d
    dx, dw = ext.rmsnorm_bwd(dy, x, w, inv)
    if dres is not None:
        dx = dx + dres
    return dx, dw


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("T", [64, 128])
@pytest.mark.parametrize("H", [256, 8192])
def test_rmsnorm_bwd_fused(ext, H, T, n, with_res):
    torch.manual_seed(6)
    x, w, inv, dys, dres = _norm_case(ext, T, H, n)
    if not with_res:
        dres = None
    dx0, dw0 = _unfused(ext, dys, x, w, inv, dres)
    dx, dw, dxT = ext.rmsnorm_bwd_fused(dys, x, w, inv, dres, True)
    assert torch.equal(dx, dx0)
    assert torch.equal(dw, dw0)
    _, dw2, _ = ext.rmsnorm_bwd_fused(dys, x, w, inv, dres, True)
    assert torch.equal(dw, dw2)
    assert dxT.shape == (H, T)
    assert torch.equal(dxT, dx0.t().contiguous())
    # no image unless asked for
    assert ext.rmsnorm_bwd_fused(dys, x, w, inv, dres, False)[2].numel() == 0


@pytest.mark.parametrize("n", [1, 2, 3])
def test_rmsnorm_bwd_fused_ragged(ext, n):
    torch.manual_seed(7)
    x, w, inv, dys, dres = _norm_case(ext, 7, 100, n)
    dx0, dw0 = _unfused(ext, dys, x, w, inv, dres)
    dx, dw, dxT = ext.rmsnorm_bwd_fused(dys, x, w, inv, dres, True)
    assert torch.equal(dx, dx0)
    assert torch.equal(dw, dw0)
    assert dxT.numel() == 0  # ragged: no image


def test_rmsnorm_bwd_fused_rejects_mismatched(ext):
    x, w, inv, dys, dres = _norm_case(ext, 64, 256, 1)
    with pytest.raises(RuntimeError):
        ext.rmsnorm_bwd_fused([dys[0][:32]], x, w, inv, None, False)
    with pytest.raises(RuntimeError):
        ext.rmsnorm_bwd_fused(dys * 4, x, w, inv, None, False)
    with pytest.raises(RuntimeError):
        ext.rmsnorm_bwd_fused(dys, x, w, inv, dres.float(), False)


# ---------------- whole layer ----------------
def _cfg():
    from lpp_amd.config import ModelConfig

    return ModelConfig(name="tiny", hidden_size=256, intermediate_size=384, num_layers=2,
                       num_heads=2, vocab_size=64, max_seq_len=64)


def _make_layers(n, ckpt):
    from lpp_amd.models.llama import DecoderLayerPipe

    torch.manual_seed(8)
    layers = []
    for _ in range(n):
        layer = DecoderLayerPipe(_cfg(), activation_checkpointing=ckpt)
        layer = layer.to(device="cuda", dtype=torch.bfloat16).train()
        with torch.no_grad():
            for norm in (layer.input_layernorm, layer.post_attention_layernorm):
                norm.weight.copy_(1.0 + 0.1 * torch.randn_like(norm.weight))
        for p in layer.parameters():
            if p.dim() == 2:
                p.main_grad = torch.zeros(p.shape, device="cuda", dtype=torch.float32)
        layers.append(layer)
    return layers


def _run_layers(layers, x0, dout, hidden_hook=None):
    """Forward + backward from a clean slate -> every tensor the step produces."""
    from lpp_amd.ops import linear as L

    L.clear_backward_caches()
    for layer in layers:
        for p in layer.parameters():
            p.grad = None
            if hasattr(p, "main_grad"):
                p.main_grad.zero_()
    x = x0.clone().requires_grad_(True)
    h = x
    for i, layer in enumerate(layers):
        h = layer(h)
        if hidden_hook is not None and i + 1 < len(layers):
            h.register_hook(hidden_hook)
    h.backward(dout)
    res = {"out": h.detach().clone(), "dx": x.grad.clone()}
    for li, layer in enumerate(layers):
        for name, p in layer.named_parameters():
            g = p.main_grad if hasattr(p, "main_grad") else p.grad
            res[f"{li}.{name}"] = g.clone()
    return res


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("n_layers", [1, 2])
def test_layer_matches_unfused(ext, monkeypatch, n_layers, ckpt):
    """Switch on == switch off, bit for bit: output, input gradient, every
    main_grad and both norm-weight gradients.  This also pins the order in
    which the fork backward sums the q/k/v partials."""
    layers = _make_layers(n_layers, ckpt)
    torch.manual_seed(9)
    x0 = _bf16(2, 64, 256)
    dout = _bf16(2, 64, 256)
    monkeypatch.setenv("LPP_BWD_HANDOFF", "0")
    ref = _run_layers(layers, x0, dout)
    monkeypatch.setenv("LPP_BWD_HANDOFF", "1")
    got = _run_layers(layers, x0, dout)
    assert set(ref) == set(got) and len(ref) == 2 + 9 * n_layers
    for key in ref:
        assert torch.equal(ref[key], got[key]), key


def test_two_layers_handoff_hits(ext, monkeypatch):
    """Which wgrads take a handed-over image and which still transpose."""
    from lpp_amd.ops import linear as L

    layers = _make_layers(2, False)
    torch.manual_seed(10)
    x0 = _bf16(2, 64, 256)
    dout = _bf16(2, 64, 256)
    monkeypatch.setenv("LPP_BWD_HANDOFF", "1")
    _run_layers(layers, x0, dout)  # warm-up: caches the weight transposes

    transposed = []
    real_transpose = ext.transpose2d

    def counting_transpose(t):
        transposed.append(t.data_ptr())
        return real_transpose(t)

    takes = []
    real_take = L._HandoffCache.take

    def recording_take(self, dy2):
        img = real_take(self, dy2)
        takes.append((dy2.data_ptr(), img is not None))
        return img

    boundary = []  # gradient that crosses from layer 1 into layer 0
    monkeypatch.setattr(ext, "transpose2d", counting_transpose)
    monkeypatch.setattr(L._HandoffCache, "take", recording_take)
    try:
        _run_layers(layers, x0, dout, hidden_hook=lambda g: boundary.append(g.data_ptr()))
    finally:
        monkeypatch.undo()

    assert len(boundary) == 1
    # 7 wgrads per layer, in backward order; the boundary gradient is the dy
    # of layer 0's down_proj and must have been handed over by layer 1's
    # input-norm backward
    assert len(takes) == 14
    assert takes[7] == (boundary[0], True)
    hits = sum(1 for _, hit in takes if hit)
    # per layer q, k, gate, up, o_proj; plus layer 0's down_proj.  Misses:
    # dv of each layer and the top down_proj, whose dy comes from outside.
    assert hits == 11
    miss_ptrs = [p for p, hit in takes if not hit]
    assert len(miss_ptrs) == 3
    # transpose2d ran for those three dy and for the four activation
    # transposes of each layer (norm1 out, attention out, norm2 out, swiglu
    # out), nothing else
    assert len(transposed) == 3 + 8
    assert all(p in transposed for p in miss_ptrs)
    assert len(L._handoff) == 0  # nothing left behind
