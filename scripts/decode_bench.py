"""Single-token decode attention: the fused gfx950 kernel against the eager
sequence it replaces, one process, device events.

Per point (geometry H/Hkv, batch N, mixed row lengths up to L):
  kernel  ops.decode_attention on the slot cache (kernel + combine), and the
          same op at the other compiled chunk sizes (the C sweep);
  valu/mfma  (--impl both, H/Hkv = 8) the vector-ALU and the MFMA kernel named
          explicitly, alternating in two passes - both passes are printed;
  model   the ragged branch of LlamaAttention.forward with the projections
          stubbed out, once on the kernel path and once under LPP_FORCE_EAGER
          (eager RoPE, two scatters, slice, repeat_interleave, masked SDPA).
Prints microseconds per layer-step and the KV bytes/s they amount to, bytes
from shapes: sum over rows of (p + 1) * Hkv * 128 * 2 B, for K and for V.
--kv-dtype fp8 runs the e4m3 cache instead (attention_decode_fp8.hip, one kernel
for every group size, so no --impl): (p + 1) * Hkv * (128 + 4) B per cache, the
4 being the row's scale; that cache has no eager branch to compare with.

    python scripts/decode_bench.py [--reps 200] [--quick] [--impl valu|mfma|both]
                                   [--kv-dtype bf16|fp8]
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


_IMPL = {"default": 0, "valu": 1, "mfma": 2}


def point(H, Hkv, N, L, reps, sweep, impl="default", fp8=False):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    pos_h = [L - 1] if N == 1 else [int(L // 4 + (L - 1 - L // 4) * i / (N - 1)) for i in range(N)]
    total = max(pos_h) + 1
    cache = RaggedKVCache(N, L, Hkv, D, dev, torch.bfloat16,
                          kv_dtype=ops.FP8_KV_DTYPE if fp8 else None)
    for dst, scale in ((cache.k, cache.k_scale), (cache.v, cache.v_scale)):
        x = torch.randn(dst.shape, generator=g, device=dev).bfloat16()
        if fp8:
            x, sc = ops.quantize_kv_rows_fp8(x)
            scale.copy_(sc.transpose(1, 2))
        dst.copy_(x)
    pos = torch.tensor(pos_h, device=dev)
    q = torch.randn(N, 1, H, D, generator=g, device=dev).bfloat16()
    k = torch.randn(N, 1, Hkv, D, generator=g, device=dev).bfloat16()
    v = torch.randn(N, 1, Hkv, D, generator=g, device=dev).bfloat16()
    cos, sin = ops.build_rope_cache(L, D, 10000.0, dev)
    kv_bytes = sum(p + 1 for p in pos_h) * Hkv * ((D + 4) if fp8 else D * 2) * 2
    ext = ops.extension()
    out = {}

    def op(chunk, which="default"):
        if fp8:
            return lambda: ext.attention_decode_fp8(q, k, v, cache.k, cache.v, cache.k_scale,
                                                    cache.v_scale, cos, sin, pos, None,
                                                    cache.lengths, 0, total, chunk)
        return lambda: ext.attention_decode(q, k, v, cache.k, cache.v, cos, sin, pos, None,
                                            cache.lengths, 0, total, chunk, _IMPL[which])

    if impl == "both":
        # the two kernels of a group of 8 in one process, alternating; a group
        # of 16 has the MFMA kernel only
        names = ("valu", "mfma") if H // Hkv == 8 else ("mfma",)
        for name in names * 2:
            out.setdefault(name, []).append(_time(op(0, name), 20, reps))
        impl = "default"
    out["kernel"] = _time(op(0, impl), 20, reps)
    if sweep:
        for c in (128, 256, 512):
            out[f"C{c}"] = _time(op(c, impl), 20, reps)

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
    if fp8:
        out["model_eager"] = float("nan")
        return out, kv_bytes
    os.environ["LPP_FORCE_EAGER"] = "1"
    try:
        out["model_eager"] = _time(branch, 20, reps) - t_copy
    finally:
        del os.environ["LPP_FORCE_EAGER"]
    return out, kv_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--quick", action="store_true",
                    help="the GQA geometries (64/8, 128/8) only, no chunk sweep")
    ap.add_argument("--impl", choices=["default", "valu", "mfma", "both"], default="default",
                    help="kernel of the 'kernel' column (geometries it does not serve are "
                         "left out); both: valu and mfma alternating, then the default")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: the e4m3 cache and its kernel (with --impl default only)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decode_bench needs a GPU"
    fp8 = args.kv_dtype == "fp8"
    assert not fp8 or args.impl == "default", "the fp8 cache has one kernel: no --impl"
    C = ops.extension().attention_decode_chunk()
    print(f"# decode attention, {args.kv_dtype} cache, D=128, compiled chunk C={C}, "
          f"reps={args.reps}")
    print("# us per layer-step (TB/s of KV read in brackets)")
    geoms = [(64, 8), (128, 8)] if args.quick else [(32, 32), (64, 64), (64, 8), (128, 8)]
    serves = {"default": (1, 2, 4, 8, 16), "both": (8, 16), "valu": (1, 2, 4, 8),
              "mfma": (8, 16)}[args.impl]
    geoms = [g for g in geoms if g[0] // g[1] in serves]
    hdr = f"{'H/Hkv':>7} {'N':>3} {'L':>5} {'KV MB':>8} | {'kernel':>15} {'model+kernel':>15} {'model eager':>15} {'x':>6}"
    if not args.quick:
        hdr += f" | {'C=128':>8} {'C=256':>8} {'C=512':>8}"
    print(hdr, flush=True)
    for H, Hkv in geoms:
        for L in (512, 4096):
            for N in (1, 8, 32):
                r, b = point(H, Hkv, N, L, args.reps, not args.quick, args.impl, fp8)
                f = lambda k: f"{r[k]:8.1f} ({b / r[k] * 1e-6:5.2f})"
                line = (f"{H:>4}/{Hkv:<2} {N:>3} {L:>5} {b / 1e6:8.2f} | {f('kernel')} "
                        f"{f('model_kernel')} {f('model_eager')} "
                        f"{r['model_eager'] / r['model_kernel']:6.1f}")
                if not args.quick:
                    line += " | " + " ".join(f"{r[k]:8.1f}" for k in ("C128", "C256", "C512"))
                for name in ("valu", "mfma"):
                    if name in r:
                        line += f" | {name} " + " ".join(
                            f"{t:7.1f} ({b / t * 1e-6:4.2f})" for t in r[name])
                print(line, flush=True)


if __name__ == "__main__":
    main()
