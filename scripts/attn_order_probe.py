#!/usr/bin/env python
"""Attention forward+backward probe for the block-order work (sibling of
attn_bwd_probe.py), production shape B=4, S=4096, H=64, D=128, bf16.

default   run forward+backward a few times under the process order
          (LPP_ATTN_ORDER=0|1), for one `rocprofv3 --kernel-trace --stats`
          run per mode, each its own process.
--ab      per-kernel device-timed A/B: hipEvent pairs around every launch
          (attention_time_kernel), the orders alternated round by round so
          clock drift hits all of them alike.  Prints one JSON line.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from lpp_amd import ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--heads", type=int, default=64)
    ap.add_argument("--kv-heads", type=int, default=0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--groups", type=str, default="1,0",
                    help="--ab: mode-1 heads per group to time (0 = the computed one)")
    ap.add_argument("--rounds", type=int, default=4, help="--ab: alternations")
    ap.add_argument("--reps", type=int, default=6, help="--ab: launches per round")
    args = ap.parse_args()

    ext = ops.extension()
    B, S, H = args.batch, args.seq, args.heads
    HKV = args.kv_heads or H
    torch.manual_seed(0)
    q = torch.randn(B, S, H, 128, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, S, HKV, 128, device="cuda", dtype=torch.bfloat16)
    v, do_ = torch.randn_like(k), torch.randn_like(q)
    o, lse = ext.attention_fwd(q, k, v)

    if not args.ab:
        for _ in range(args.iters):
            o, lse = ext.attention_fwd(q, k, v)
            ext.attention_bwd(do_, q, k, v, o, lse)
        torch.cuda.synchronize()
        print(f"attn order probe done (mode {ext.attention_get_block_order()})")
        return

    # label -> (mode, G); G 0 = the group the launch computes itself,
    # G = nheads is fully block-major (best balance, no head locality)
    def orders(nheads):
        cand = {"mode0": (0, 0)}
        for g in (int(x) for x in args.groups.split(",")):
            cand[f"mode1_G{g}" if g else "mode1_Gauto"] = (1, g)
        cand["mode1_Gall"] = (1, nheads)
        return cand

    flops = {"fwd": 4, "dq": 6, "dkdv": 8}  # causal GEMMs x 2 flops, x S*S*D/2
    result = {"shape": {"B": B, "S": S, "H": H, "HKV": HKV}, "kernels": {}}
    for kern in ("fwd", "dq", "dkdv"):
        cand = orders(B * (HKV if kern == "dkdv" else H))
        times = {name: [] for name in cand}
        for rnd in range(args.rounds):
            for name, (mode, G) in cand.items():
                times[name] += ext.attention_time_kernel(
                    kern, do_, q, k, v, o, lse, mode, G, 2 if rnd == 0 else 1, args.reps)
        rows = {}
        for name, ts in times.items():
            med = statistics.median(ts)
            rows[name] = {
                "median_ms": round(med, 4), "min_ms": round(min(ts), 4),
                "max_ms": round(max(ts), 4), "launches": len(ts),
                # spread of the per-round medians = repeat-to-repeat spread
                "round_medians_ms": [round(statistics.median(ts[i:i + args.reps]), 4)
                                     for i in range(0, len(ts), args.reps)],
                "tflops": round(flops[kern] * B * H * S * S * 128 / 2 / med / 1e9, 1),
            }
        result["kernels"][kern] = rows
    print(json.dumps(result))


if __name__ == "__main__":
    main()
