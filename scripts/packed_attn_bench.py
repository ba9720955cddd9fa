#!/usr/bin/env python
"""Time the document-masked attention kernels on packed-row layouts against
the plain causal kernels (attention_time_kernel: one hipEvent pair per launch,
median of the reps), next to the ideal work ratio sum(len^2) / S^2.

    python scripts/packed_attn_bench.py [--B 4 --S 4096 --H 64 --HKV 64]
                                        [--warmup 5 --reps 20] [--json OUT]

Layouts: one document of S (the cost of the mask bookkeeping), S/512 documents
of 512, S/128 of 128, and a seeded FLAN-like mix (log-normal lengths, median
~180 tokens, clipped to 8..2048, drawn until the row is full; the last one is
cut to fit).  The same layout is used in every batch row except for the mix.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def flan_like_lengths(S, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    out, left = [], S
    while left:
        n = int(torch.exp(torch.randn((), generator=g) * 0.9 + 5.2).clamp(8, 2048))
        n = min(n, left)
        out.append(n)
        left -= n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--S", type=int, default=4096)
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--HKV", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    a = ap.parse_args()

    import torch

    from lpp_amd import ops

    ext = ops.extension()
    B, S = a.B, a.S
    g = torch.Generator().manual_seed(0)
    q, do_ = (torch.randn(B, S, a.H, 128, generator=g).to(torch.bfloat16).cuda()
              for _ in range(2))
    k, v = (torch.randn(B, S, a.HKV, 128, generator=g).to(torch.bfloat16).cuda()
            for _ in range(2))
    mode = ext.attention_get_block_order()

    layouts = {"plain": None, f"1x{S}": [[S]] * B}
    for n in (512, 128):
        if S % n == 0 and S > n:
            layouts[f"{S // n}x{n}"] = [[n] * (S // n)] * B
    layouts["flan_like_mix"] = [flan_like_lengths(S, 40 + b) for b in range(B)]

    rows, plain = [], {}
    for name, lengths in layouts.items():
        docs = None if lengths is None else ops.DocLayout.from_lengths(lengths, S, "cuda")
        if docs is None:
            o, lse = ext.attention_fwd(q, k, v)
            extra, ideal = {}, 1.0
        else:
            o, lse = ext.attention_fwd_docs(q, k, v, docs.doc_start)
            extra = {"doc_start": docs.doc_start, "doc_end": docs.doc_end}
            ideal = sum(n * n for row in lengths for n in row) / (B * S * S)
        row = {"layout": name, "ideal_ratio": ideal,
               "docs_per_row": None if lengths is None
               else sum(len(r) for r in lengths) / B}
        for kern in ("fwd", "dq", "dkdv"):
            ms = ext.attention_time_kernel(kern, do_, q, k, v, o, lse, mode, 0,
                                           a.warmup, a.reps, **extra)
            row[kern] = statistics.median(ms)
            if docs is None:
                plain[kern] = row[kern]
            row[kern + "_ratio"] = row[kern] / plain[kern]
        rows.append(row)
        print(f"{name:>14}  ideal {ideal:6.4f}  " + "  ".join(
            f"{kern} {row[kern]:7.3f} ms ({row[kern + '_ratio']:5.3f}x)"
            for kern in ("fwd", "dq", "dkdv")), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(
            {"B": B, "S": S, "H": a.H, "HKV": a.HKV, "warmup": a.warmup, "reps": a.reps,
             "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
