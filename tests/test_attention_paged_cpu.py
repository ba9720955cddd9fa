"""Paged KV cache on the CPU: the references over a shuffled, interleaved block
table against the same references over a slot cache holding the same data, and
the engine serving from pages."""

import pytest
import torch

from lpp_amd import ops
from lpp_amd.config import model_config
from lpp_amd.models import LlamaForCausalLM, init_monolithic_weights
from lpp_amd.serving import ContinuousBatchingEngine, Request

D = 128


def scatter_into_pages(slot_tensors, page, seed=0, spare=3):
    """A slot cache as a pool under a non-monotone table.  slot_tensors: caches
    [slots,T,Hkv,D] and scales [slots,Hkv,T] (T a multiple of page).  Returns
    (pools, table, gather): page m of slot r is pool page table[r, m], the
    pages of the rows interleaved and shuffled, with `spare` pages no row owns;
    those keep a sentinel pattern (0x5b bytes: finite in bf16, e4m3 and fp32).
    gather(pools) is the slot-layout view of pools, for comparing afterwards."""
    slots, dev = slot_tensors[0].shape[0], slot_tensors[0].device
    T = slot_tensors[0].shape[1] if slot_tensors[0].dim() == 4 else slot_tensors[0].shape[2]
    M = T // page
    g = torch.Generator().manual_seed(seed)
    ids = torch.randperm(slots * M + spare, generator=g)[: slots * M]
    table = ids.view(M, slots).T.contiguous().to(torch.int32).to(dev)   # rows interleaved
    bt = table.long()

    def to_pool(x):
        shape = [page, *x.shape[2:]] if x.dim() == 4 else [x.shape[1], page]
        shape[-1] *= x.element_size()
        pool = torch.full((slots * M + spare, *shape), 0x5b, dtype=torch.uint8,
                          device=dev).view(x.dtype)
        if x.dim() == 4:
            pool.view(torch.uint8)[bt] = x.view(slots, M, page, *x.shape[2:]).view(torch.uint8)
        else:
            pool[bt] = x.view(slots, x.shape[1], M, page).transpose(1, 2)
        return pool

    def gather(pools):
        return [p.view(torch.uint8)[bt].flatten(1, 2).view(p.dtype) if p.dim() == 4
                else p[bt].transpose(1, 2).flatten(2, 3) for p in pools]

    return [to_pool(x) for x in slot_tensors], table, gather


@pytest.mark.parametrize("page", [4, 64])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("extend", [False, True])
def test_refs_over_pages_equal_refs_over_slots(extend, fp8, page):
    H, Hkv, slots, T, Sq = 4, 2, 4, 2 * 64, 5 if extend else 1
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g)
    rows = torch.tensor([2, 0, 3])
    pos = torch.tensor([0, page - 2, page + 3])          # new tokens cross a page boundary
    lens = torch.tensor([5, 4, 3]) if extend else torch.ones(3, dtype=torch.long)
    q, k_new, v_new = (rn(3, Sq, h, D).bfloat16() for h in (H, Hkv, Hkv))
    cos, sin = ops.build_rope_cache(T, D, 10000.0, torch.device("cpu"))
    slot = [rn(slots, T, Hkv, D).bfloat16(), rn(slots, T, Hkv, D).bfloat16()]
    if fp8:
        (k, ks), (v, vs) = (ops.quantize_kv_rows_fp8(x) for x in slot)
        slot = [k, v, ks.transpose(1, 2).contiguous(), vs.transpose(1, 2).contiguous()]
    pools, table, gather = scatter_into_pages(slot, page)
    before = [p.clone() for p in pools]
    fn = ops.extend_attention if extend else ops.decode_attention
    kw = dict(q_lens=lens) if extend else {}
    outs = []
    for c, extra in ((slot, {}), (pools, dict(block_table=table))):
        ln = torch.arange(11, 11 + slots)
        if fp8:
            extra = dict(extra, k_scale=c[2], v_scale=c[3])
        outs.append((fn(q, k_new, v_new, c[0], c[1], cos, sin, pos, rows=rows, lengths=ln,
                        **kw, **extra), ln))
    (o_slot, ln_slot), (o_page, ln_page) = outs
    assert torch.equal(o_page, o_slot) and torch.equal(ln_page, ln_slot)
    for got, want in zip(gather(pools), slot):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    owned = torch.zeros(pools[0].shape[0], dtype=torch.bool)
    owned[table.long().flatten()] = True
    for p, b in zip(pools, before):                      # pages of no row: untouched
        assert torch.equal(p.view(torch.uint8)[~owned], b.view(torch.uint8)[~owned])


def test_engine_serves_from_pages():
    cfg = model_config("llama-tiny", num_layers=2, max_seq_len=128)
    m = LlamaForCausalLM(cfg)
    init_monolithic_weights(m, seed=9)
    with pytest.raises(ValueError, match="prefill_chunk"):
        ContinuousBatchingEngine(m, max_slots=3, max_seq_len=32, kv_page_size=4, kv_pages=7)
    g = torch.Generator().manual_seed(4)
    want = {"a": (6, 5), "b": (3, 7), "c": (10, 2), "d": (1, 9)}   # 3, 3, 3, 3 pages
    prompts = {u: torch.randint(4, cfg.vocab_size, (n,), generator=g) for u, (n, _) in want.items()}
    results = []
    for paged in (dict(), dict(kv_page_size=4, kv_pages=7)):
        eng = ContinuousBatchingEngine(m, max_slots=3, max_seq_len=32, prefill_chunk=4, **paged)
        for uid, (_, new) in want.items():
            eng.submit(Request(uid, prompts[uid], new))
        waited = False
        for _ in range(80):
            if not eng.pending():
                break
            eng.step()
            # a free slot, yet the head of the queue waits: it waits for pages
            waited |= bool(eng.waiting) and bool(eng.free_slots)
        assert not eng.pending()
        results.append(eng.results)
        if paged:
            assert waited
            assert eng.caches[0].k.shape[:2] == (7, 4) and eng.caches[1].block_table is eng.block_table
            assert sorted(eng.free_pages) == list(range(7)) and not eng.slot_pages
            with pytest.raises(ValueError, match="KV pages"):
                eng.submit(Request("big", torch.zeros(20, dtype=torch.long), 12))   # 8 pages
    for uid in want:
        assert torch.equal(results[1][uid], results[0][uid]), uid
