#!/usr/bin/env python
"""Per-op timing of the FP8 and MXFP4 weight-only linears (ops.linear_fp8w,
ops.linear_fp4w) against the bf16 F.linear they replace, at the 7B and 70B
projection shapes (1 GPU).

Each shape is timed with device events over a ring of weight copies larger
than the last-level cache (--ring-mb, counted in each path's own bytes), so
every call streams its weight from HBM as a decode tick does; the three paths
alternate inside each of --rounds rounds.  Times are means over the rounds;
fp4 against fp8 is given with its lowest and highest ratio over the rounds.
TB/s counts the weight bytes alone (2 per element for bf16, 1 + 4/128 for fp8,
1/2 + 1/32 for fp4).

A second table (--tiled-ms, rows above 64) times three paths per point, in
--rounds alternating rounds: bf16 F.linear, dequantise + F.linear (the default
route of ops.linear_fp8w above 64 rows) and the tiled fp8 kernel.  Each time is
the mean over the rounds; the ratio of the tiled kernel against dequantise +
F.linear is given with its lowest and highest value over the rounds, each
round's ratio taken from that round's own two timings.

Usage (GPU box):  python scripts/linear_fp8w_bench.py [--reps 20]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch
import torch.nn.functional as F

from lpp_amd import ops

# (name, in, out)
SHAPES = [
    ("7b qkvo", 4096, 4096), ("7b gate/up", 4096, 11008), ("7b down", 11008, 4096),
    ("7b lm_head", 4096, 32000),
    ("70b q/o", 8192, 8192), ("70b k/v", 8192, 1024), ("70b gate/up", 8192, 28672),
    ("70b down", 28672, 8192), ("70b lm_head", 8192, 32000),
]


def _time(fn, ring, reps):
    """Mean ms per call over reps passes of the ring, device events."""
    for w in ring[:2]:
        fn(w)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        for w in ring:
            fn(w)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / (reps * len(ring))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ring-mb", type=int, default=768)
    ap.add_argument("--ms", type=int, nargs="*", default=[1, 8, 16, 64])
    ap.add_argument("--tiled-ms", type=int, nargs="*", default=[65, 128, 256, 512, 1024, 2048])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=None, help="names to keep (default all)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "run on the GPU box"
    g = torch.Generator().manual_seed(0)
    shapes = [sh for sh in SHAPES if args.shapes is None or sh[0] in args.shapes]
    if args.ms:
        print("| shape | in x out | M | bf16 F.linear us | TB/s | fp8w us | TB/s | fp4w us | TB/s | "
              "fp8 vs bf16 | fp4 vs bf16 | fp4 vs fp8 | over the rounds |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    tiled_rows = []
    for name, inn, out in shapes:
        w = (torch.randn(out, inn, generator=g) * 0.02).bfloat16().cuda()
        wq, sc = ops.quantize_weight_fp8(w)
        w4, s4 = ops.quantize_weight_fp4(w)
        # weight bytes of one call, and a ring of copies larger than the cache for each path
        by_bf, by_q, by_4 = 2 * inn * out, inn * out + 4 * inn * out // 128, inn * out // 2 + inn * out // 32
        n_bf, n_q, n_4 = (max(2, -(-args.ring_mb * 2**20 // b)) for b in (by_bf, by_q, by_4))
        ring_bf = [w.clone() for _ in range(n_bf)]
        ring_q = [(wq.clone(), sc.clone()) for _ in range(n_q)]
        ring_4 = [(w4.clone(), s4.clone()) for _ in range(n_4)]
        for M in args.ms:
            x = (torch.randn(M, inn, generator=g)).bfloat16().cuda()
            paths = [(lambda t: F.linear(x, t), ring_bf),
                     (lambda t: ops.linear_fp8w(x, *t), ring_q),
                     (lambda t: ops.linear_fp4w(x, *t), ring_4)]
            # the three paths alternate inside a round
            ms = [[_time(fn, ring, args.reps) for fn, ring in paths] for _ in range(args.rounds)]
            bf, q8, q4 = (sum(r[i] for r in ms) / len(ms) for i in range(3))
            ratios = [r[1] / r[2] for r in ms]
            print(f"| {name} | {inn} x {out} | {M} | {bf * 1e3:.1f} | {by_bf / bf / 1e9:.2f} | "
                  f"{q8 * 1e3:.1f} | {by_q / q8 / 1e9:.2f} | {q4 * 1e3:.1f} | {by_4 / q4 / 1e9:.2f} | "
                  f"{bf / q8:.2f}x | {bf / q4:.2f}x | {q8 / q4:.2f}x | "
                  f"{min(ratios):.2f} .. {max(ratios):.2f} |", flush=True)
        del ring_4
        for M in args.tiled_ms:
            x = (torch.randn(M, inn, generator=g)).bfloat16().cuda()
            paths = [(lambda t: F.linear(x, t), ring_bf),
                     (lambda t: ops.linear_fp8w(x, *t, tiled=False), ring_q),
                     (lambda t: ops.linear_fp8w(x, *t, tiled=True), ring_q)]
            ms = [[_time(fn, ring, args.reps) for fn, ring in paths] for _ in range(args.rounds)]
            bf, dq, tl = (sum(r[i] for r in ms) / len(ms) for i in range(3))
            ratios = [r[1] / r[2] for r in ms]
            tiled_rows.append(
                f"| {name} | {inn} x {out} | {M} | {bf * 1e3:.1f} | {dq * 1e3:.1f} | "
                f"{tl * 1e3:.1f} | {dq / tl:.2f}x | {min(ratios):.2f} .. {max(ratios):.2f} | "
                f"{bf / tl:.2f}x |")
            print("tiled " + tiled_rows[-1], flush=True)
        del ring_bf, ring_q
    if tiled_rows:
        print("\n| shape | in x out | M | bf16 F.linear us | dequant + F.linear us | tiled us | "
              "tiled vs dequant | over the rounds | tiled vs bf16 |")
        print("|---|---|---|---|---|---|---|---|---|")
        print("\n".join(tiled_rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
