"""The wgrad handoff cache alone (no GPU): producers register a gradient
with its transposed image, the consuming wgrad takes it by identity."""

import torch

from lpp_amd.ops import linear as L


def _pair(rows=4, cols=6, dtype=torch.bfloat16):
    nat = torch.randn(rows, cols).to(dtype)
    return nat, nat.t().contiguous()


def test_hit_takes_the_entry():
    c = L._HandoffCache()
    nat, img = _pair()
    c.put(nat, img)
    # looked up through a fresh view of the same storage, as the wgrad does
    got = c.take(nat.reshape(-1, nat.shape[-1]))
    assert got is img
    assert len(c) == 0 and c.hits == 1
    assert c.take(nat) is None  # one consumer per gradient
    assert c.misses == 1


def test_miss_on_pointer_shape_dtype():
    c = L._HandoffCache()
    nat, img = _pair(4, 6)
    c.put(nat, img)
    assert c.take(nat.clone()) is None                      # other storage
    assert c.take(nat.view(6, 4)) is None                   # same pointer, other shape
    assert c.take(nat.view(torch.float16)) is None          # same pointer, other dtype
    assert c.take(nat[1:]) is None                          # offset into the storage
    assert len(c) == 1 and c.misses == 4 and c.hits == 0
    assert c.take(nat) is img


def test_strong_reference_keeps_the_key_alive():
    c = L._HandoffCache()
    nat, img = _pair()
    ptr = nat.data_ptr()
    c.put(nat, img)
    del nat
    # the storage cannot have been recycled under the key
    assert c.entries[0][0].data_ptr() == ptr


def test_eviction_at_four_entries_oldest_first():
    c = L._HandoffCache()
    pairs = [_pair() for _ in range(5)]
    for nat, img in pairs:
        c.put(nat, img)
    assert len(c) == 4 == L._HandoffCache.CAPACITY
    assert c.take(pairs[0][0]) is None
    for nat, img in pairs[1:]:
        assert c.take(nat) is img
    assert len(c) == 0


def test_clear_and_module_helpers(monkeypatch):
    L._handoff.clear()
    nat, img = _pair(8, 3)
    L.register_handoff(nat.view(2, 4, 3), img)  # producers pass the natural N-d tensor
    assert len(L._handoff) == 1
    assert L._handoff.entries[0][0].shape == (8, 3)
    L.clear_backward_caches()
    assert len(L._handoff) == 0 and L._xt_cache.x is None
    assert L._handoff.take(nat) is None

    monkeypatch.delenv("LPP_BWD_HANDOFF", raising=False)
    assert L.bwd_handoff_enabled()
    monkeypatch.setenv("LPP_BWD_HANDOFF", "0")
    assert not L.bwd_handoff_enabled()
