"""FP8 weight-only linear on the CPU: the quantisation rule, the reference op
and a greedy engine over quantised weights against one over their dequantised
values."""

import copy

import pytest
import torch
import torch.nn.functional as F

from lpp_amd import ops
from lpp_amd.config import model_config
from lpp_amd.models import LlamaForCausalLM, init_monolithic_weights
from lpp_amd.ops.linear import LPLinear
from lpp_amd.serving import ContinuousBatchingEngine, Request

FP8 = torch.float8_e4m3fn


def _dequant(wq, scale):
    out, inn = wq.shape
    return (wq.float().view(out, -1, 128) * scale[..., None]).view(out, inn)


def test_quantize_weight_fp8_rule():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(32, 384, generator=g) * 0.05).bfloat16()
    w[3, 128:256] = 0                                    # a zero block
    wq, scale = ops.quantize_weight_fp8(w)
    assert wq.dtype is FP8 and wq.shape == (32, 384)
    assert scale.dtype is torch.float32 and scale.shape == (32, 3)
    deq = _dequant(wq, scale)
    assert torch.equal(deq.bfloat16().float(), deq)      # exact in bf16
    amax = w.float().view(32, 3, 128).abs().amax(-1, keepdim=True)
    assert bool(((w.float() - deq).view(32, 3, 128).abs() <= amax / 16).all())
    assert scale[3, 1] == 1 and not deq[3, 128:256].any()
    assert torch.equal(torch.frexp(scale)[0], torch.full_like(scale, 0.5))   # powers of two
    for shape in ((32, 192), (24, 128)):
        with pytest.raises(ValueError, match="128"):
            ops.quantize_weight_fp8(torch.zeros(shape, dtype=torch.bfloat16))


def test_linear_fp8w_ref_is_linear_over_the_dequantised_weight():
    g = torch.Generator().manual_seed(1)
    wq, scale = ops.quantize_weight_fp8(torch.randn(48, 256, generator=g).bfloat16())
    x = torch.randn(2, 3, 256, generator=g).bfloat16()
    want = F.linear(x, _dequant(wq, scale).bfloat16())
    assert torch.equal(ops.linear_fp8w_ref(x, wq, scale), want)
    assert torch.equal(ops.linear_fp8w(x, wq, scale), want)          # the CPU path


def test_engine_with_fp8_weights_matches_the_dequantised_model():
    cfg = model_config("llama-tiny", hidden_size=256, num_heads=2, intermediate_size=384,
                       num_layers=2, max_seq_len=64)
    m = LlamaForCausalLM(cfg).bfloat16()
    init_monolithic_weights(m, seed=5)
    twin = copy.deepcopy(m)                      # holds the dequantised weights
    quantised = [mod for layer in twin.layers[1:] for mod in layer.modules()
                 if isinstance(mod, torch.nn.Linear)]
    assert len(quantised) == 2 * 7 + 1
    with torch.no_grad():
        for mod in quantised:
            mod.weight.copy_(_dequant(*ops.quantize_weight_fp8(mod.weight)))
    g = torch.Generator().manual_seed(2)
    prompts = {"a": torch.randint(4, cfg.vocab_size, (6,), generator=g),
               "b": torch.randint(4, cfg.vocab_size, (9,), generator=g)}
    results = []
    for model, wd in ((m, FP8), (twin, None)):
        eng = ContinuousBatchingEngine(model, max_slots=2, max_seq_len=32, prefill_chunk=4,
                                       weight_dtype=wd)
        for uid, p in prompts.items():
            eng.submit(Request(uid, p, 5))
        for _ in range(40):
            if not eng.pending():
                break
            eng.step()
        assert not eng.pending()
        results.append(eng.results)
    for uid in prompts:
        assert torch.equal(results[0][uid], results[1][uid])
    for mod in m.modules():
        if isinstance(mod, LPLinear) or mod is m.layers[-1]:
            assert mod.weight is None and mod.weight_fp8.dtype is FP8
            assert mod.weight_scale.shape == (mod.out_features, mod.in_features // 128)
    assert m.layers[0].weight.dtype is torch.bfloat16                # the embedding stays
    with pytest.raises(RuntimeError, match="inference-only"):
        m.layers[1].mlp.up_proj(torch.zeros(1, 256, dtype=torch.bfloat16))
