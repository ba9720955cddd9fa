#!/usr/bin/env python
"""Per-op timing of the FP8 weight-only linear (ops.linear_fp8w) against the
bf16 F.linear it replaces, at the 7B and 70B projection shapes (1 GPU).

Each shape is timed with device events over a ring of weight copies larger
than the last-level cache (--ring-mb), so every call streams its weight from
HBM as a decode tick does; the two paths alternate inside one run.  TB/s counts
the weight bytes alone (1 byte + 4/128 per element for fp8, 2 for bf16).

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
    ap.add_argument("--ms", type=int, nargs="+", default=[1, 8, 16, 64])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "run on the GPU box"
    g = torch.Generator().manual_seed(0)
    print("| shape | in x out | M | bf16 F.linear us | TB/s | fp8w us | TB/s | speedup |")
    print("|---|---|---|---|---|---|---|---|")
    for name, inn, out in SHAPES:
        w = (torch.randn(out, inn, generator=g) * 0.02).bfloat16().cuda()
        wq, sc = ops.quantize_weight_fp8(w)
        n = max(2, -(-args.ring_mb * 2**20 // (2 * inn * out)))
        ring_bf = [w.clone() for _ in range(n)]
        ring_q = [(wq.clone(), sc.clone()) for _ in range(n)]
        for M in args.ms:
            x = (torch.randn(M, inn, generator=g)).bfloat16().cuda()
            ms_bf = ms_q = 0.0
            for _ in range(2):           # the two paths alternate
                ms_bf += _time(lambda t: F.linear(x, t), ring_bf, args.reps) / 2
                ms_q += _time(lambda t: ops.linear_fp8w(x, *t), ring_q, args.reps) / 2
            tb_bf = 2 * inn * out / ms_bf / 1e9
            tb_q = (inn * out + 4 * inn * out // 128) / ms_q / 1e9
            print(f"| {name} | {inn} x {out} | {M} | {ms_bf * 1e3:.1f} | {tb_bf:.2f} | "
                  f"{ms_q * 1e3:.1f} | {tb_q:.2f} | {ms_bf / ms_q:.2f}x |", flush=True)
        del ring_bf, ring_q
    return 0


if __name__ == "__main__":
    sys.exit(main())
