"""Continuous batching for single-device serving.

Requests arrive at any time; each is prefetched into a free KV-cache slot
(its prefill runs through the flash-attention path via a slot row-view)
and then decodes in ONE batched single-token step per engine tick together
with every other active request — finished requests retire and free their
slot immediately, so short requests never wait for long ones (the
"continuous"/in-flight batching of production serving stacks).  Decode
attention is the ragged per-row-length branch of ``LlamaAttention``: for
bf16 / head_dim 128 one fused gfx950 kernel per layer (``ops.decode_attention``
- RoPE, cache write and GQA attention over each row's own prefix, read
straight from the slot cache), eager SDPA otherwise.  With ``prefill_chunk``
set, prompts of any lengths prefill together a chunk per tick through
``ops.extend_attention`` while the active rows keep decoding.

The reference has no inference capability at all (training-only template,
SURVEY.md §0); this extends the framework's own ``generate``/
``pipeline_generate`` serving story.

Usage:
    eng = ContinuousBatchingEngine(model, max_slots=8, max_seq_len=512)
    eng.submit(Request("a", prompt_ids_a, max_new_tokens=32))
    eng.submit(Request("b", prompt_ids_b, max_new_tokens=8))
    while eng.pending():
        eng.step()
    eng.results["a"]  # full sequence tensor (prompt + generated)
"""

from __future__ import annotations

from collections import deque
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from .models.llama import (DecoderLayerPipe, GatherKVCache, LMHeadPipe, MultiSlotKVCache,
                           RaggedKVCache)
from .ops.linear import LPLinear


@dataclass
class Request:
    uid: str
    prompt: torch.Tensor  # [S0] long
    max_new_tokens: int
    temperature: float = 0.0
    # filled by the engine
    slot: int = -1
    generated: List[int] = field(default_factory=list)
    finished: bool = False


class ContinuousBatchingEngine:
    def __init__(self, model, max_slots: int, max_seq_len: int,
                 eos_token_id: Optional[int] = None,
                 generator: Optional[torch.Generator] = None,
                 prefill_chunk: Optional[int] = None,
                 kv_dtype: Optional[torch.dtype] = None,
                 kv_page_size: Optional[int] = None,
                 kv_pages: Optional[int] = None,
                 weight_dtype: Optional[torch.dtype] = None):
        """``prefill_chunk``: None admits as before (equal-length prompts
        prefill together, each in one piece).  A value admits prompts of any
        lengths together and prefills them at most that many tokens per row
        per tick through ``ops.extend_attention``, while the rows already
        decoding keep decoding every tick.

        ``kv_dtype``: None keeps the cache in the model dtype.
        ``torch.float8_e4m3fn`` (opt-in) halves its bytes: e4m3 rows with one
        power-of-two scale per (slot, kv head, token), see ``RaggedKVCache``.
        It needs ``prefill_chunk``, because the one-piece admission writes the
        cache without quantising.

        ``kv_page_size`` with ``kv_pages`` (opt-in) pages the cache: every
        layer's K/V is a pool of ``kv_pages`` pages of ``kv_page_size`` tokens
        and one block table, shared by all layers, names each slot's pages.  A
        request waits until ``ceil((prompt + max_new_tokens) / kv_page_size)``
        pages are free, holds them until it finishes, and is rejected at
        ``submit`` if it asks for more than ``kv_pages``.  How many requests
        fit is then decided by the tokens they hold, not by ``max_seq_len``
        per slot.  It needs ``prefill_chunk`` for the reason fp8 does; the
        gfx950 kernels serve a page of 64 tokens.

        ``weight_dtype``: None keeps the model's weights.
        ``torch.float8_e4m3fn`` (opt-in) quantises every projection of the
        decoder layers and the LM head IN PLACE (``LPLinear.quantize_fp8_``:
        e4m3 bytes and one power-of-two scale per 128 inputs of a row, half
        the weight memory); embedding and norms stay as they are.  Decode
        ticks then run ``ops.linear_fp8w``.  ``torch.float4_e2m1fn_x2``
        (opt-in) does the same in the MXFP4 format (``LPLinear.quantize_fp4_``:
        e2m1 nibbles and one e8m0 scale byte per 32 inputs of a row, a good
        quarter of the bf16 memory; round-to-nearest, no calibration) and
        decode ticks run ``ops.linear_fp4w``.  Independent of ``kv_dtype`` and
        paging."""
        if weight_dtype not in (None, torch.float8_e4m3fn, torch.float4_e2m1fn_x2):
            raise ValueError("weight_dtype must be None, float8_e4m3fn or float4_e2m1fn_x2, "
                             f"got {weight_dtype}")
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError(f"prefill_chunk must be >= 1, got {prefill_chunk}")
        if (kv_page_size is None) != (kv_pages is None):
            raise ValueError("kv_page_size and kv_pages go together")
        if kv_page_size is not None and prefill_chunk is None:
            raise ValueError("a paged KV cache needs prefill_chunk: the one-piece admission "
                             "writes the cache contiguously")
        if kv_dtype is torch.float8_e4m3fn and prefill_chunk is None:
            raise ValueError("an fp8 KV cache needs prefill_chunk: only the chunked prefill "
                             "(ops.extend_attention) quantises what it appends")
        self.prefill_chunk = prefill_chunk
        self.prefilling: Dict[int, list] = {}  # slot -> [request, prompt tokens cached]
        self.model = model
        self.model.eval()
        self.max_slots = max_slots
        self.max_seq_len = max_seq_len
        self.eos_token_id = eos_token_id
        self.generator = generator
        p = next(model.parameters())
        self.device = p.device
        cfg = model.cfg
        self.decoders = [l for l in model.layers if isinstance(l, DecoderLayerPipe)]
        if weight_dtype is not None:
            for layer in model.layers:
                if isinstance(layer, (DecoderLayerPipe, LMHeadPipe)):
                    for m in layer.modules():
                        if isinstance(m, (LPLinear, LMHeadPipe)):
                            if weight_dtype is torch.float8_e4m3fn:
                                m.quantize_fp8_()
                            else:
                                m.quantize_fp4_()
        self.caches = [
            RaggedKVCache(max_slots, max_seq_len, cfg.kv_heads, cfg.head_dim,
                          self.device, p.dtype, kv_dtype=kv_dtype,
                          page_size=kv_page_size, num_pages=kv_pages)
            for _ in self.decoders
        ]
        self.kv_page_size = kv_page_size
        self.kv_pages = kv_pages
        self.free_pages: deque[int] = deque(range(kv_pages or 0))
        self.slot_pages: Dict[int, List[int]] = {}  # slot -> the pages it holds
        self.block_table = None
        if kv_page_size is not None:
            self.block_table = self.caches[0].block_table
            for c in self.caches:
                c.block_table = self.block_table  # one table for every layer
        self.free_slots = deque(range(max_slots))
        self.active: Dict[int, Request] = {}  # slot -> request
        self.waiting: deque[Request] = deque()
        self.results: Dict[str, torch.Tensor] = {}
        self._last_logits: Dict[int, torch.Tensor] = {}  # slot -> [V]

    # ------------------------------------------------------------------
    def submit(self, req: Request) -> None:
        if req.prompt.numel() + req.max_new_tokens > self.max_seq_len:
            raise ValueError(
                f"request {req.uid}: prompt+new "
                f"{req.prompt.numel() + req.max_new_tokens} > max_seq_len "
                f"{self.max_seq_len}")
        if self.block_table is not None and self._pages_needed(req) > self.kv_pages:
            raise ValueError(
                f"request {req.uid}: needs {self._pages_needed(req)} KV pages, the pool has "
                f"{self.kv_pages}")
        self.waiting.append(req)

    def _pages_needed(self, req: Request) -> int:
        return -(-(req.prompt.numel() + req.max_new_tokens) // self.kv_page_size)

    def pending(self) -> int:
        return len(self.waiting) + len(self.prefilling) + len(self.active)

    # ------------------------------------------------------------------
    def _run_layers(self, x: torch.Tensor, caches) -> torch.Tensor:
        ci = 0
        for layer in self.model.layers:
            if isinstance(layer, DecoderLayerPipe):
                x = layer(x, cache=caches[ci])
                ci += 1
            else:
                x = layer(x)
        return x

    @torch.no_grad()
    def _admit(self) -> None:
        """Move waiting requests into free slots; requests with EQUAL
        prompt lengths prefill together as one batched flash forward."""
        while self.waiting and self.free_slots:
            group = [self.waiting.popleft()]
            S0 = group[0].prompt.numel()
            while (self.waiting and len(group) < len(self.free_slots)
                   and self.waiting[0].prompt.numel() == S0):
                group.append(self.waiting.popleft())
            slots = [self.free_slots.popleft() for _ in group]
            for c in self.caches:
                for s in slots:
                    c.free(s)
            slot_t = torch.tensor(slots, dtype=torch.long, device=self.device)
            views = [MultiSlotKVCache(c, slot_t) for c in self.caches]
            ids = torch.stack([r.prompt for r in group]).to(self.device)
            logits = self._run_layers(ids, views)[:, -1]
            for i, (req, slot) in enumerate(zip(group, slots)):
                req.slot = slot
                self._last_logits[slot] = logits[i]
                self.active[slot] = req

    @torch.no_grad()
    def _prefill_tick(self) -> None:
        """Chunked admission: waiting requests of any prompt length take the
        free slots, and every row still prefilling advances by at most
        ``prefill_chunk`` tokens in ONE ragged extend forward (q_lens padded
        to the longest chunk of the group).  A row whose prompt completes
        becomes active; its first token is sampled from the logits of its
        last prompt token."""
        while self.waiting and self.free_slots:
            if self.block_table is not None:
                # first come, first served: the head of the queue waits for its pages
                need = self._pages_needed(self.waiting[0])
                if need > len(self.free_pages):
                    break
            req, slot = self.waiting.popleft(), self.free_slots.popleft()
            if self.block_table is not None:
                pages = [self.free_pages.popleft() for _ in range(need)]
                self.slot_pages[slot] = pages
                self.block_table[slot, :need] = torch.tensor(pages, dtype=torch.int32)
            for c in self.caches:
                c.free(slot)
            req.slot = slot
            self.prefilling[slot] = [req, 0]
        if not self.prefilling:
            return
        slots = sorted(self.prefilling)
        done = [self.prefilling[s][1] for s in slots]
        lens = [min(self.prefill_chunk, self.prefilling[s][0].prompt.numel() - d)
                for s, d in zip(slots, done)]
        ids = torch.zeros(len(slots), max(lens), dtype=torch.long)
        for i, (s, d, n) in enumerate(zip(slots, done, lens)):
            ids[i, :n] = self.prefilling[s][0].prompt.view(-1)[d : d + n]

        class _Tick:
            pass

        tick = _Tick()
        tick.pos = torch.tensor(done, dtype=torch.long, device=self.device)
        tick.q_lens = torch.tensor(lens, dtype=torch.long, device=self.device)
        slot_t = torch.tensor(slots, dtype=torch.long, device=self.device)
        views = [GatherKVCache(c, slot_t, total_hint=max(d + n for d, n in zip(done, lens)))
                 for c in self.caches]
        for v in views:
            v.tick = tick
        logits = self._run_layers(ids.to(self.device), views)
        for i, (s, d, n) in enumerate(zip(slots, done, lens)):
            req = self.prefilling[s][0]
            if d + n == req.prompt.numel():
                del self.prefilling[s]
                self._last_logits[s] = logits[i, n - 1]
                self.active[s] = req
            else:
                self.prefilling[s][1] = d + n

    def _sample_batched(self, slots: List[int]) -> List[int]:
        """One device->host sync per tick (per-slot .item() calls dominated
        the first version's decode time)."""
        logits = torch.stack([self._last_logits[s] for s in slots])  # [N, V]
        if all(self.active[s].temperature == 0 for s in slots):
            return logits.argmax(dim=-1).tolist()
        temps = torch.tensor([self.active[s].temperature for s in slots],
                             device=logits.device)
        toks = logits.argmax(dim=-1)
        if bool((temps > 0).any()):
            probs = torch.softmax(
                logits.float() / temps.clamp(min=1e-6)[:, None], dim=-1)
            gen = self.generator if (self.generator is not None and
                                     str(self.generator.device) ==
                                     str(logits.device)) else None
            sampled = torch.multinomial(probs, 1, generator=gen).squeeze(-1)
            toks = torch.where(temps > 0, sampled, toks)
        return toks.tolist()

    @torch.no_grad()
    def step(self) -> List[str]:
        """One engine tick: admit -> sample each active slot's pending
        logits (batched, one sync) -> retire finished -> ONE batched
        ragged decode for the rest.  Returns the uids finished this tick."""
        if self.prefill_chunk is None:
            self._admit()
        else:
            self._prefill_tick()
        done: List[str] = []
        slots = sorted(self.active)
        if not slots:
            return done
        # sample from the logits produced by the previous forward (the
        # prefill for newly admitted requests)
        for slot, tok in zip(slots, self._sample_batched(slots)):
            req = self.active[slot]
            req.generated.append(tok)
            if ((self.eos_token_id is not None and tok == self.eos_token_id)
                    or len(req.generated) >= req.max_new_tokens):
                req.finished = True
                self.results[req.uid] = torch.cat(
                    [req.prompt.view(-1).cpu(),
                     torch.tensor(req.generated, dtype=torch.long)])
                done.append(req.uid)
                del self.active[slot]
                del self._last_logits[slot]
                for c in self.caches:
                    c.free(slot)
                self.free_slots.append(slot)
                self.free_pages.extend(self.slot_pages.pop(slot, ()))
        if not self.active:
            return done
        # one batched ragged decode over every active slot (views memoized
        # per active-set; contiguous slot ranges decode zero-copy)
        slots = sorted(self.active)
        key = tuple(slots)
        if getattr(self, "_views_key", None) != key:
            slot_t = torch.tensor(slots, dtype=torch.long, device=self.device)
            rng = ((slots[0], slots[-1] + 1)
                   if slots == list(range(slots[0], slots[-1] + 1)) else None)
            self._views = [GatherKVCache(c, slot_t, contiguous_range=rng)
                           for c in self.caches]
            self._views_key = key
        # host-side per-tick tensors, shared by EVERY layer: max length,
        # gathered RoPE phases at each row's position, key-validity mask —
        # rebuilding these per layer made the decode tick launch-bound
        # the token being fed is generated[-1]: its position = tokens
        # already in the cache = prompt + len(generated) - 1
        lens_h = [self.active[s].prompt.numel() + len(self.active[s].generated) - 1
                  for s in slots]
        total = max(lens_h) + 1
        from lpp_amd import ops

        cfg = self.model.cfg
        cos, sin = ops.build_rope_cache(cfg.max_seq_len, cfg.head_dim,
                                        cfg.rope_theta, self.device)
        pos = torch.tensor(lens_h, dtype=torch.long, device=self.device)

        class _Tick:
            pass

        tick = _Tick()
        tick.cos = cos[pos].view(len(slots), 1, 1, -1)
        tick.sin = sin[pos].view(len(slots), 1, 1, -1)
        tick.mask = (torch.arange(total, device=self.device)[None, :]
                     <= pos[:, None])[:, None, None, :]
        tick.pos = pos  # the fused decode kernel gathers RoPE phases itself
        for v in self._views:
            v.total_hint = total
            v.tick = tick
        toks = torch.tensor([self.active[s].generated[-1] for s in slots],
                            dtype=torch.long, device=self.device).view(-1, 1)
        logits = self._run_layers(toks, self._views)[:, -1]
        for i, s in enumerate(slots):
            self._last_logits[s] = logits[i]
        return done
