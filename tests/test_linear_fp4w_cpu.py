"""MXFP4 weight-only linear on the CPU: the quantisation rule, the reference op
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

FP4 = torch.float4_e2m1fn_x2
GRID = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])


def _dequant(wq, scale):
    """By hand: element 2i in the low nibble of byte i, scale 2^(b-127) per 32."""
    out, half = wq.shape
    val = torch.stack((GRID[(wq & 15).long()], GRID[(wq >> 4).long()]), -1).view(out, -1, 32)
    return (val * torch.exp2(scale.float() - 127)[..., None]).view(out, 2 * half)


def test_quantize_weight_fp4_rule():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(32, 384, generator=g) * 0.05).bfloat16()
    w[3, 128:160] = 0                                    # a zero block
    # a block of amax 6 (scale 1) holding the seven ties and their even neighbours
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    even = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0])
    w[5, 0:32] = 0
    w[5, 0:7], w[5, 7:14], w[5, 14] = ties, -ties, 6.0
    wq, scale = ops.quantize_weight_fp4(w)
    assert wq.dtype is torch.uint8 and wq.shape == (32, 192)
    assert scale.dtype is torch.uint8 and scale.shape == (32, 12)
    deq = _dequant(wq, scale)
    assert torch.equal(deq.bfloat16().float(), deq)      # exact in bf16
    amax = w.float().view(32, 12, 32).abs().amax(-1, keepdim=True)
    assert bool(((w.float() - deq).view(32, 12, 32).abs() <= amax / 4).all())
    assert scale[3, 4] == 127 and not wq[3, 64:80].any()
    assert int(scale.min()) >= 27 and int(scale.max()) <= 227
    assert scale[5, 0] == 127
    assert torch.equal(deq[5, 0:7], even) and torch.equal(deq[5, 7:14], -even)
    for shape in ((32, 192), (24, 128)):
        with pytest.raises(ValueError, match="128"):
            ops.quantize_weight_fp4(torch.zeros(shape, dtype=torch.bfloat16))


def test_linear_fp4w_ref_is_linear_over_the_dequantised_weight():
    g = torch.Generator().manual_seed(1)
    wq, scale = ops.quantize_weight_fp4(torch.randn(48, 256, generator=g).bfloat16())
    x = torch.randn(2, 3, 256, generator=g).bfloat16()
    want = F.linear(x, _dequant(wq, scale).bfloat16())
    assert torch.equal(ops.linear_fp4w_ref(x, wq, scale), want)
    assert torch.equal(ops.linear_fp4w(x, wq, scale), want)          # the CPU path


def test_engine_with_fp4_weights_matches_the_dequantised_model():
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
            mod.weight.copy_(_dequant(*ops.quantize_weight_fp4(mod.weight)))
    g = torch.Generator().manual_seed(2)
    prompts = {"a": torch.randint(4, cfg.vocab_size, (6,), generator=g),
               "b": torch.randint(4, cfg.vocab_size, (9,), generator=g)}
    results = []
    for model, wd in ((m, FP4), (twin, None)):
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
            assert mod.weight is None and mod.weight_fp4.dtype is torch.uint8
            assert mod.weight_fp4.shape == (mod.out_features, mod.in_features // 2)
            assert mod.weight_scale.shape == (mod.out_features, mod.in_features // 32)
    assert m.layers[0].weight.dtype is torch.bfloat16                # the embedding stays
    with pytest.raises(RuntimeError, match="inference-only"):
        m.layers[1].mlp.up_proj(torch.zeros(1, 256, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="float4_e2m1fn_x2"):
        ContinuousBatchingEngine(twin, max_slots=1, max_seq_len=8, weight_dtype=torch.int8)
