"""Extend attention (several new tokens per row over the ragged KV cache) on
the CPU, fp32: the reference against single-token decode, chunked prefill
through the model, and the serving engine's ``prefill_chunk``."""

import pytest
import torch

from lpp_amd import ops
from lpp_amd.config import model_config
from lpp_amd.models import LlamaForCausalLM, init_monolithic_weights
from lpp_amd.models.llama import DecoderLayerPipe, KVCache
from lpp_amd.serving import ContinuousBatchingEngine, Request


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
def test_ref_equals_token_by_token_decode(H, Hkv):
    D, slots, Tmax, Sq = 16, 4, 24, 5
    g = torch.Generator().manual_seed(0)
    rows = torch.tensor([2, 0, 3])
    pos = torch.tensor([0, 7, 11])
    q_lens = torch.tensor([5, 1, 3])
    q = torch.randn(3, Sq, H, D, generator=g)
    k_new = torch.randn(3, Sq, Hkv, D, generator=g)
    v_new = torch.randn(3, Sq, Hkv, D, generator=g)
    cos, sin = ops.build_rope_cache(Tmax, D, 10000.0, torch.device("cpu"))
    k0 = torch.randn(slots, Tmax, Hkv, D, generator=g)
    v0 = torch.randn(slots, Tmax, Hkv, D, generator=g)
    len0 = torch.tensor([7, 50, 0, 11])

    k1, v1, len1 = k0.clone(), v0.clone(), len0.clone()
    o = ops.extend_attention(q, k_new, v_new, k1, v1, cos, sin, pos, q_lens=q_lens,
                             rows=rows, lengths=len1)
    k2, v2, len2 = k0.clone(), v0.clone(), len0.clone()
    for i in range(Sq):
        live = q_lens > i                         # rows that still have a token i
        oi = ops.decode_attention_ref(q[live, i : i + 1], k_new[live, i : i + 1],
                                      v_new[live, i : i + 1], k2, v2, cos, sin, pos[live] + i,
                                      rows=rows[live], lengths=len2)
        assert float((o[live, i : i + 1] - oi).abs().max()) < 1e-5
        assert not o[~live, i].any()              # past a row's length: zero
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    assert torch.equal(len1, len2) and len1.tolist() == [8, 50, 5, 14]


def _step(m, caches, ids):
    x, li = ids, 0
    for layer in m.layers:
        if isinstance(layer, DecoderLayerPipe):
            x = layer(x, cache=caches[li])
            li += 1
        else:
            x = layer(x)
    return x


def test_chunked_prefill_through_kvcache_matches_whole_prompt():
    cfg = model_config("llama-tiny", num_layers=2, max_seq_len=128)
    m = LlamaForCausalLM(cfg).eval()
    init_monolithic_weights(m, seed=9)
    ids = torch.randint(4, cfg.vocab_size, (2, 11), generator=torch.Generator().manual_seed(1))
    new = lambda: [KVCache(2, 16, cfg.kv_heads, cfg.head_dim, "cpu", torch.float32)
                   for _ in range(cfg.num_layers)]
    with torch.no_grad():
        whole = _step(m, new(), ids)[:, -1]
        caches = new()
        for a, b in ((0, 4), (4, 5), (5, 11)):
            last = _step(m, caches, ids[:, a:b])[:, -1]
    assert float((last - whole).abs().max()) < 1e-4


@pytest.mark.parametrize("lens,chunk", [((3, 7, 10), 4), ((5, 1, 9), 4), ((3, 7, 10), 1)])
def test_engine_prefill_chunk_matches_default_engine(lens, chunk):
    """Prompts of lengths 3, 7 and 10 arrive while another request decodes;
    greedy tokens equal the default engine's exactly (seed 9 / 4: no argmax
    tie met).  Lengths 5, 1 and 9 (and a chunk of 1) end in prefill ticks whose
    longest chunk is a single token."""
    cfg = model_config("llama-tiny", num_layers=2, max_seq_len=128)
    m = LlamaForCausalLM(cfg)
    init_monolithic_weights(m, seed=9)
    g = torch.Generator().manual_seed(4)
    prompts = [torch.randint(4, cfg.vocab_size, (n,), generator=g) for n in (6, *lens)]
    new = [9, 4, 6, 5]

    def run(**kw):
        eng = ContinuousBatchingEngine(m, max_slots=4, max_seq_len=64, **kw)
        eng.submit(Request("r0", prompts[0], new[0]))
        ticks = 0
        while eng.pending():
            eng.step()
            ticks += 1
            if ticks == 2:                        # r0 is decoding by now
                for i in (1, 2, 3):
                    eng.submit(Request(f"r{i}", prompts[i], new[i]))
            assert ticks < 60
        return eng

    ref, eng = run(), run(prefill_chunk=chunk)
    for i in range(4):
        assert torch.equal(eng.results[f"r{i}"], ref.results[f"r{i}"]), i
    assert all(int(c.lengths.sum()) == 0 for c in eng.caches)
