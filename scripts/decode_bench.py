"""Single-token decode attention: the fused gfx950 kernel against the eager
sequence it replaces, one process, device events.

Per point (geometry H/Hkv, batch N, mixed row lengths up to L):
  kernel  ops.decode_attention on the slot cache (kernel + combine), and the
          same op at the other compiled chunk sizes (the C sweep);
  model   the ragged branch of LlamaAttention.forward with the projections
          stubbed out, once on the kernel path and once under LPP_FORCE_EAGER
          (eager RoPE, two scatters, slice, repeat_interleave, masked SDPA).
Prints microseconds per layer-step and the KV bytes/s they amount to, bytes
from shapes: sum over rows of (p + 1) * Hkv * 128 * 2 B, for K and for V.

    python scripts/decode_bench.py [--reps 200] [--quick]
"""

from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lpp_amd import ops  # noqa: E402
from lpp_amd.config import ModelConfig  # noqa: E402
from lpp_amd.models.llama import GatherKVCache, LlamaAttention, RaggedKVCache  # noqa: E402

D = 128


class _Fixed(torch.nn.Module):
    """Stands in for a projection: returns a fixed tensor (or its input)."""

    def __init__(self, out=None):
        super().__init__()
        self.out = out

    def forward(self, x):
        return x if self.out is None else self.out


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def point(H, Hkv, N, L, reps, sweep):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    pos_h = [L - 1] if N == 1 else [int(L // 4 + (L - 1 - L // 4) * i / (N - 1)) for i in range(N)]
    total = max(pos_h) + 1
    cache = RaggedKVCache(N, L, Hkv, D, dev, torch.bfloat16)
    cache.k.copy_(torch.randn(cache.k.shape, generator=g, device=dev))
    cache.v.copy_(torch.randn(cache.v.shape, generator=g, device=dev))
    pos = torch.tensor(pos_h, device=dev)
    q = torch.randn(N, 1, H, D, generator=g, device=dev).bfloat16()
    k = torch.randn(N, 1, Hkv, D, generator=g, device=dev).bfloat16()
    v = torch.randn(N, 1, Hkv, D, generator=g, device=dev).bfloat16()
    cos, sin = ops.build_rope_cache(L, D, 10000.0, dev)
    kv_bytes = sum(p + 1 for p in pos_h) * Hkv * D * 2 * 2
    ext = ops.extension()
    out = {}

    def op(chunk):
        return lambda: ext.attention_decode(q, k, v, cache.k, cache.v, cos, sin, pos, None,
                                            cache.lengths, 0, total, chunk)

    out["kernel"] = _time(op(0), 20, reps)
    if sweep:
        for c in (128, 256, 512):
            out[f"C{c}"] = _time(op(c), 20, reps)

    # the model branch, projections stubbed
    cfg = ModelConfig(hidden_size=H * D, num_heads=H, num_kv_heads=Hkv, max_seq_len=L)
    with torch.device("meta"):
        attn = LlamaAttention(cfg)
    attn.q_proj, attn.k_proj, attn.v_proj = (_Fixed(t.view(N, 1, -1)) for t in (q, k, v))
    attn.o_proj = _Fixed()
    view = GatherKVCache(cache, torch.arange(N, device=dev), contiguous_range=(0, N),
                         total_hint=total)

    class _Tick:
        pass

    tick = _Tick()
    tick.cos = cos[pos].view(N, 1, 1, -1)
    tick.sin = sin[pos].view(N, 1, 1, -1)
    tick.mask = (torch.arange(total, device=dev)[None, :] <= pos[:, None])[:, None, None, :]
    tick.pos = pos
    view.tick = tick
    x = torch.zeros(N, 1, H * D, device=dev, dtype=torch.bfloat16)

    def branch():
        cache.lengths.copy_(pos)  # the eager branch appends at lengths
        with torch.no_grad():
            return attn(x, cache=view)

    def copy_only():
        cache.lengths.copy_(pos)

    t_copy = _time(copy_only, 20, reps)
    out["model_kernel"] = _time(branch, 20, reps) - t_copy
    os.environ["LPP_FORCE_EAGER"] = "1"
    try:
        out["model_eager"] = _time(branch, 20, reps) - t_copy
    finally:
        del os.environ["LPP_FORCE_EAGER"]
    return out, kv_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="one geometry, no chunk sweep")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decode_bench needs a GPU"
    C = ops.extension().attention_decode_chunk()
    print(f"# decode attention, bf16, D=128, compiled chunk C={C}, reps={args.reps}")
    print("# us per layer-step (TB/s of KV read in brackets)")
    geoms = [(64, 8)] if args.quick else [(32, 32), (64, 64), (64, 8)]
    hdr = f"{'H/Hkv':>7} {'N':>3} {'L':>5} {'KV MB':>8} | {'kernel':>15} {'model+kernel':>15} {'model eager':>15} {'x':>6}"
    if not args.quick:
        hdr += f" | {'C=128':>8} {'C=256':>8} {'C=512':>8}"
    print(hdr, flush=True)
    for H, Hkv in geoms:
        for L in (512, 4096):
            for N in (1, 8, 32):
                r, b = point(H, Hkv, N, L, args.reps, not args.quick)
                f = lambda k: f"{r[k]:8.1f} ({b / r[k] * 1e-6:5.2f})"
                line = (f"{H:>4}/{Hkv:<2} {N:>3} {L:>5} {b / 1e6:8.2f} | {f('kernel')} "
                        f"{f('model_kernel')} {f('model_eager')} "
                        f"{r['model_eager'] / r['model_kernel']:6.1f}")
                if not args.quick:
                    line += " | " + " ".join(f"{r[k]:8.1f}" for k in ("C128", "C256", "C512"))
                print(line, flush=True)


if __name__ == "__main__":
    main()
