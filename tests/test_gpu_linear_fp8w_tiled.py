"""Tiled FP8 weight-only linear (linear_fp8w_tiled_kernel) on the GPU.

Data and criterion are those of test_gpu_linear_fp8w.py: every 128-block of
every weight row carries its own power of two in 2^-10 .. 2^10 (weights at
2^-10, x at 2^-4), the reference is float64 x @ deq^T, and the kernel passes
with err <= 2 * err_eager + ulp(max|ref|) and err < 3e-2, err_eager being bf16
F.linear over the dequantised weight.

A workgroup owns 128 tokens x 128 output rows and one K-slice of whole
128-blocks.  M = 65 is a partial token tile, 128 exactly one, 129 one plus a
row.  (in, out, slices): (128, 16, rule) one block, less than one output tile;
(384, 144, 1) three blocks, a full output tile and one of 16 rows; (384, 144,
3) one block per slice through the workspace and the combine launch; (1152,
272, rule) nine blocks under the rule's own split; (1152, 144, 2) uneven
slices of 5 + 4 blocks.
"""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(128, 16, 0), (384, 144, 1), (384, 144, 3), (1152, 272, 0), (1152, 144, 2)]


def _bf16_ulp(x):
    _, e = torch.frexp(x.float())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 8)


@functools.lru_cache(maxsize=None)
def _case(inn, out):
    """x [129, in], the quantised weight, its exact bf16 dequantisation (by torch)."""
    from lpp_amd import ops

    g = torch.Generator().manual_seed(inn + out)
    e = torch.randint(-10, 11, (out, inn // 128, 1), generator=g).float()
    w = torch.randn(out, inn // 128, 128, generator=g) * 2.0 ** -10 * torch.exp2(e)
    wq, scale = ops.quantize_weight_fp8(w.view(out, inn).bfloat16())
    deq = (wq.float().view(out, -1, 128) * scale[..., None]).view(out, inn).bfloat16()
    x = (torch.randn(129, inn, generator=g) * 2.0 ** -4).bfloat16()
    return x.to(DEV), wq.to(DEV), scale.to(DEV), deq.to(DEV)


def _check(got, ref, eager, tag):
    err = float((got.double() - ref).abs().max())
    err_eager = float((eager.double() - ref).abs().max())
    top = ref.abs().max()
    print(f"\n{tag}: kernel err {err:.3e}  eager err {err_eager:.3e}  max|ref| {float(top):.3f}")
    assert err < 3e-2
    assert err <= 2 * err_eager + float(_bf16_ulp(top))


@pytest.mark.parametrize("inn,out,slices", CASES)
@pytest.mark.parametrize("M", [65, 128, 129])
def test_kernel_against_float64(M, inn, out, slices):
    from lpp_amd import ops

    x, wq, scale, deq = _case(inn, out)
    ext = ops.extension()
    y = ext.linear_fp8w_tiled(x[:M], wq, scale, slices)
    assert y.shape == (M, out) and y.dtype is torch.bfloat16
    assert torch.equal(ext.linear_fp8w_tiled(x[:M], wq, scale, slices), y)
    _check(y, x[:M].double() @ deq.double().T, F.linear(x[:M], deq),
           f"M={M} in={inn} out={out} slices={slices}")


def test_routing():
    from lpp_amd import ops

    x, wq, scale, _ = _case(1152, 272)
    ext = ops.extension()
    assert torch.equal(ops.linear_fp8w(x, wq, scale, tiled=True),
                       ext.linear_fp8w_tiled(x, wq, scale, 0))            # M = 129
    assert torch.equal(ops.linear_fp8w(x[:64], wq, scale, tiled=True),
                       ext.linear_fp8w(x[:64], wq, scale))


def test_launcher_rejects_before_launching():
    from lpp_amd import ops

    x, wq, scale, _ = _case(384, 144)
    ext = ops.extension()
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.linear_fp8w_tiled(x[::2], wq, scale, 0)
    with pytest.raises(RuntimeError, match="slices"):
        ext.linear_fp8w_tiled(x, wq, scale, -1)
    with pytest.raises(RuntimeError, match="slices"):
        ext.linear_fp8w_tiled(x, wq, scale, 4)


def test_one_engine_prefill_tick(monkeypatch):
    from lpp_amd import ops
    from lpp_amd.config import model_config
    from lpp_amd.models import LlamaForCausalLM, init_monolithic_weights
    from lpp_amd.serving import ContinuousBatchingEngine, Request

    monkeypatch.setenv("LPP_FP8W_TILED", "1")
    cfg = model_config("llama-tiny", hidden_size=256, num_heads=2, intermediate_size=384,
                       num_layers=2, max_seq_len=128)
    m = LlamaForCausalLM(cfg).bfloat16()
    init_monolithic_weights(m, seed=5)
    twin = copy.deepcopy(m)                      # the dequantised weights, on the CPU
    with torch.no_grad():
        for layer in twin.layers[1:]:
            for mod in layer.modules():
                if isinstance(mod, torch.nn.Linear):
                    wq, sc = ops.quantize_weight_fp8(mod.weight)
                    mod.weight.copy_((wq.float().view(*sc.shape, 128) * sc[..., None])
                                     .view_as(mod.weight))
    eng = ContinuousBatchingEngine(m.to(DEV), max_slots=2, max_seq_len=128, prefill_chunk=128,
                                   weight_dtype=torch.float8_e4m3fn)
    prompt = torch.randint(4, cfg.vocab_size, (70,), generator=torch.Generator().manual_seed(3))
    eng.submit(Request("a", prompt, 4))
    eng.step()                                   # 70-row prefill, first token, one decode tick
    ids = torch.cat([prompt, torch.tensor(eng.active[0].generated)])[None]
    with torch.no_grad():
        eager = twin(ids)[0, -1]
        ref = twin.double()(ids)[0, -1]
    _check(eng._last_logits[0].cpu(), ref, eager, "engine prefill tick")
