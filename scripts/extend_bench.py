"""Extend attention (Sq new tokens per row over the slot cache): the gfx950
kernels against the eager branch they replace, one process, device events.

Per point (70B geometry H 64 / Hkv 8; N rows, Sq new tokens, p tokens cached):
  kernel  ops.extend_attention (append + attention [+ combine]) on the path
          the row count selects, then the direct path and the split path at
          every compiled chunk size (the sweep behind the threshold and C);
  eager   LlamaAttention.forward on a uniform KVCache with the projections
          stubbed out, under LPP_FORCE_EAGER: eager RoPE, cache append,
          repeat_interleave, [Sq, total] mask, SDPA (at p = 0: causal SDPA).
Prints microseconds per layer-step and executed TF/s, operations from shapes:
4 * 128 * H * sum over rows and tokens of (p + i + 1).
Yardstick: (1, 4096, 0) against causal_attention's forward kernel.

--kv-dtype fp8 runs the kernels over the e4m3 cache (the append quantises, the
attention kernel dequantises into LDS); that cache has no eager branch.

    python scripts/extend_bench.py [--reps 50] [--quick | --sweep] [--kv-dtype bf16|fp8]
"""

from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lpp_amd import ops  # noqa: E402
from lpp_amd.config import ModelConfig  # noqa: E402
from lpp_amd.models.llama import KVCache, LlamaAttention  # noqa: E402

D, H, HKV = 128, 64, 8
POINTS = [(1, 512, 0), (1, 512, 3584), (4, 128, 2048), (8, 8, 4000)]
CHUNKS = (128, 256, 512, 1024)
# --sweep: the points behind the split threshold and C (profiles/README.md,
# Round 11): R = Sq * 8 from 64 to 2048 at one and several rows, a short cache
SWEEP = [(1, 8, 4000), (8, 8, 4000), (32, 8, 4000), (1, 32, 4000), (8, 32, 4000),
         (1, 64, 2048), (4, 64, 2048), (1, 96, 2048), (4, 96, 2048), (1, 128, 2048),
         (4, 128, 2048), (1, 256, 2048), (4, 256, 2048), (1, 8, 500), (8, 8, 500)]


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


def _flops(N, Sq, p):
    return 4 * D * H * N * sum(p + i + 1 for i in range(Sq))


FP8 = False  # --kv-dtype fp8


def _inputs(N, Sq, p):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev).bfloat16()
    L = p + Sq
    cache = KVCache(N, L, HKV, D, dev, torch.bfloat16)
    cache.k.copy_(rn(*cache.k.shape))
    cache.v.copy_(rn(*cache.v.shape))
    cache.scales = {}
    if FP8:
        (cache.k, ks), (cache.v, vs) = (ops.quantize_kv_rows_fp8(t) for t in (cache.k, cache.v))
        cache.scales = dict(k_scale=ks.transpose(1, 2).contiguous(),
                            v_scale=vs.transpose(1, 2).contiguous())
    cos, sin = ops.build_rope_cache(L, D, 10000.0, dev)
    return cache, rn(N, Sq, H, D), rn(N, Sq, HKV, D), rn(N, Sq, HKV, D), cos, sin, L


def point(N, Sq, p, reps, sweep, eager=True):
    cache, q, k, v, cos, sin, L = _inputs(N, Sq, p)
    out = {}

    def op(chunk, split):
        return lambda: ops.extend_attention(q, k, v, cache.k, cache.v, cos, sin, p,
                                            max_len=L, chunk=chunk, split=split,
                                            **cache.scales)

    out["kernel"] = _time(op(0, None), 10, reps)
    if sweep:
        out["direct"] = _time(op(0, False), 10, reps)
        for c in CHUNKS:
            out[f"C{c}"] = _time(op(c, True), 10, reps)
    if not eager or FP8:
        out["eager"] = float("nan")
        return out

    cfg = ModelConfig(hidden_size=H * D, num_heads=H, num_kv_heads=HKV, max_seq_len=L)
    with torch.device("meta"):
        attn = LlamaAttention(cfg)
    attn.q_proj, attn.k_proj, attn.v_proj = (_Fixed(t.view(N, Sq, -1)) for t in (q, k, v))
    attn.o_proj = _Fixed()
    x = torch.zeros(N, Sq, H * D, device="cuda", dtype=torch.bfloat16)

    def branch():
        cache.length = p
        with torch.no_grad():
            return attn(x, cache=cache)

    os.environ["LPP_FORCE_EAGER"] = "1"
    try:
        out["eager"] = _time(branch, 5, max(reps // 5, 5))
    finally:
        del os.environ["LPP_FORCE_EAGER"]
    return out


def yardstick(reps):
    """(1, 4096, 0): the direct path against the training forward kernel."""
    N, Sq = 1, 4096
    cache, q, k, v, cos, sin, L = _inputs(N, Sq, 0)
    ext = ops.extension()
    t_ext = _time(lambda: ops.extend_attention(q, k, v, cache.k, cache.v, cos, sin, 0,
                                               max_len=L, **cache.scales), 10, reps)
    t_fwd = _time(lambda: ext.attention_fwd(q, k, v), 10, reps)
    f = _flops(N, Sq, 0)
    print(f"# yardstick (1, 4096, 0): extend (RoPE + append + attention) {t_ext:9.1f} us "
          f"{f / t_ext * 1e-6:6.1f} TF/s | causal forward {t_fwd:9.1f} us "
          f"{f / t_fwd * 1e-6:6.1f} TF/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="no path / chunk sweep")
    ap.add_argument("--sweep", action="store_true",
                    help="the threshold / C sweep points instead: the op alone, every path")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "extend_bench needs a GPU"
    global FP8
    FP8 = args.kv_dtype == "fp8"
    C = ops.extension().attention_extend_chunk()
    print(f"# extend attention, {args.kv_dtype} cache, D=128, H/Hkv {H}/{HKV}, compiled chunk C={C}, "
          f"reps={args.reps}")
    if args.sweep:
        print(f"# us, the op alone | {'N':>3} {'Sq':>5} {'p':>5} {'R':>5} | {'kernel':>9} "
              f"{'direct':>9} " + " ".join(f"{'C=' + str(c):>9}" for c in CHUNKS), flush=True)
        for N, Sq, p in SWEEP:
            r = point(N, Sq, p, args.reps, True, eager=False)
            print(f"{N:>3} {Sq:>5} {p:>5} {Sq * H // HKV:>5} | {r['kernel']:9.1f} "
                  f"{r['direct']:9.1f} " + " ".join(f"{r[f'C{c}']:9.1f}" for c in CHUNKS),
                  flush=True)
        return
    print("# us per layer-step (executed TF/s in brackets)")
    hdr = f"{'N':>3} {'Sq':>5} {'p':>5} | {'kernel':>16} {'eager':>16} {'x':>6}"
    if not args.quick:
        hdr += f" | {'direct':>9} " + " ".join(f"{'C=' + str(c):>9}" for c in CHUNKS)
    print(hdr, flush=True)
    for N, Sq, p in POINTS:
        r = point(N, Sq, p, args.reps, not args.quick)
        f = _flops(N, Sq, p)
        cell = lambda key: f"{r[key]:9.1f} ({f / r[key] * 1e-6:5.1f})"
        line = (f"{N:>3} {Sq:>5} {p:>5} | {cell('kernel')} {cell('eager')} "
                f"{r['eager'] / r['kernel']:6.1f}")
        if not args.quick:
            line += f" | {r['direct']:9.1f} " + " ".join(f"{r[f'C{c}']:9.1f}" for c in CHUNKS)
        print(line, flush=True)
    yardstick(args.reps)


if __name__ == "__main__":
    main()
