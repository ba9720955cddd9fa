"""MXFP4 weight-only linear (linear_fp4w.hip) on the GPU.

Weights are random bf16 (base magnitude 2^-10, x at 2^-4) with every 32-block
of every row multiplied by its own power of two in 2^-10 .. 2^10, so a scale
byte read from the wrong row, block or lane group shows.  The reference is
float64 x @ deq^T and the criterion the project's own: err <= 2 * err_eager +
ulp(max|ref|) and err < 3e-2, err_eager being bf16 F.linear over the
dequantised weight.  max|ref| lies between 1.1 and 4.3 over these shapes.

Shapes, by the kernel's split rule (a workgroup owns 64 rows and a K-slice of
L steps of 128 k, L = 4 here, the smallest): (128, 16) one step, one row
group; (384, 48) an odd step count and a partial workgroup, one slice;
(2176, 272) 17 steps and 17 row groups, 5 slices; (1152, 64) 9 steps = 3
slices through the fp32 workspace and the combine launch, the last slice a
single step.
"""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(128, 16), (384, 48), (2176, 272), (1152, 64)]
GRID = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])


def _bf16_ulp(x):
    _, e = torch.frexp(x.float())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 8)


def _dequant(wq, scale):
    """By hand: element 2i in the low nibble of byte i, scale 2^(b-127) per 32."""
    out, half = wq.shape
    val = torch.stack((GRID[(wq & 15).long()], GRID[(wq >> 4).long()]), -1).view(out, -1, 32)
    return (val * torch.exp2(scale.float() - 127)[..., None]).view(out, 2 * half)


@functools.lru_cache(maxsize=None)
def _case(inn, out):
    """x [65, in], the quantised weight, its exact bf16 dequantisation (by torch)."""
    from lpp_amd import ops

    g = torch.Generator().manual_seed(inn + out)
    e = torch.randint(-10, 11, (out, inn // 32, 1), generator=g).float()
    w = torch.randn(out, inn // 32, 32, generator=g) * 2.0 ** -10 * torch.exp2(e)
    wq, scale = ops.quantize_weight_fp4(w.view(out, inn).bfloat16())
    deq = _dequant(wq, scale)
    assert torch.equal(deq.bfloat16().float(), deq)
    x = (torch.randn(65, inn, generator=g) * 2.0 ** -4).bfloat16()
    return x.to(DEV), wq.to(DEV), scale.to(DEV), deq.bfloat16().to(DEV)


def _check(y, x, deq, tag):
    ref = x.double() @ deq.double().T
    err = float((y.double() - ref).abs().max())
    err_eager = float((F.linear(x, deq).double() - ref).abs().max())
    top = ref.abs().max()
    print(f"\n{tag}: kernel err {err:.3e}  eager err {err_eager:.3e}  max|ref| {float(top):.3f}")
    assert err < 3e-2
    assert err <= 2 * err_eager + float(_bf16_ulp(top))


@pytest.mark.parametrize("inn,out", SHAPES)
@pytest.mark.parametrize("M", [1, 5, 16, 17, 64])
def test_kernel_against_float64(M, inn, out):
    from lpp_amd import ops

    x, wq, scale, deq = _case(inn, out)
    y = ops.linear_fp4w(x[:M].view(1, M, inn), wq, scale)       # a leading dim rides along
    assert y.shape == (1, M, out) and y.dtype is torch.bfloat16
    _check(y[0], x[:M], deq, f"M={M} in={inn} out={out}")


def test_batch_invariance():
    from lpp_amd import ops

    x, wq, scale, _ = _case(2176, 272)
    full = ops.linear_fp4w(x[:64], wq, scale)
    for m in (1, 5, 17):
        assert torch.equal(ops.linear_fp4w(x[:m], wq, scale), full[:m])


def test_above_64_rows_dequantises_for_hipblaslt():
    from lpp_amd import ops

    x, wq, scale, deq = _case(2176, 272)
    w = ops.extension().linear_fp4w_dequant(wq, scale)
    assert torch.equal(w, deq)                   # pins the nibble order and the scale indexing
    assert torch.equal(ops.linear_fp4w(x, wq, scale), F.linear(x, w))      # M = 65


def test_launcher_rejects_before_launching():
    from lpp_amd import ops

    x, wq, scale, _ = _case(384, 48)
    ext = ops.extension()
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.linear_fp4w(x[:16:2], wq, scale)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ext.linear_fp4w(x[:8, :192].contiguous(), wq[:, :96].contiguous(),
                        scale[:, :6].contiguous())
    with pytest.raises(RuntimeError, match="scale must be"):
        ext.linear_fp4w(x[:8], wq, scale[:, :8].contiguous())


def test_one_engine_tick():
    from lpp_amd import ops
    from lpp_amd.config import model_config
    from lpp_amd.models import LlamaForCausalLM, init_monolithic_weights
    from lpp_amd.serving import ContinuousBatchingEngine, Request

    cfg = model_config("llama-tiny", hidden_size=256, num_heads=2, intermediate_size=384,
                       num_layers=2, max_seq_len=64)
    m = LlamaForCausalLM(cfg).bfloat16()
    init_monolithic_weights(m, seed=5)
    twin = copy.deepcopy(m)                      # the dequantised weights, on the CPU
    with torch.no_grad():
        for layer in twin.layers[1:]:
            for mod in layer.modules():
                if isinstance(mod, torch.nn.Linear):
                    mod.weight.copy_(_dequant(*ops.quantize_weight_fp4(mod.weight)))
    eng = ContinuousBatchingEngine(m.to(DEV), max_slots=2, max_seq_len=32,
                                   weight_dtype=torch.float4_e2m1fn_x2)
    prompt = torch.randint(4, cfg.vocab_size, (7,), generator=torch.Generator().manual_seed(3))
    eng.submit(Request("a", prompt, 4))
    eng.step()                                   # prefill, first token, one decode tick
    ids = torch.cat([prompt, torch.tensor(eng.active[0].generated)])[None]
    got = eng._last_logits[0].cpu().double()
    with torch.no_grad():
        eager = twin(ids)[0, -1].double()
        ref = twin.double()(ids)[0, -1]
    err, err_eager = float((got - ref).abs().max()), float((eager - ref).abs().max())
    print(f"\nengine tick: err {err:.3e}  eager err {err_eager:.3e}  "
          f"max|ref| {float(ref.abs().max()):.3f}")
    assert err < 3e-2
    assert err <= 2 * err_eager + float(_bf16_ulp(ref.abs().max()))
