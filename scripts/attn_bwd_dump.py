#!/usr/bin/env python
"""Dump the attention backward's outputs for a build-to-build comparison.

Inputs come from a seeded CPU generator, so two builds of the extension see
the same bits: S=320 (MHA and GQA) and S=576, bf16, D=128.  Writes
<case>_{dq,dk,dv}.npy (bf16 bit patterns as int16) into the directory.

    python scripts/attn_bwd_dump.py OUT_DIR            # in each checkout
    python scripts/attn_bwd_dump.py --compare DIR_A DIR_B
"""
import argparse
import sys
from pathlib import Path

import numpy as np

CASES = {"s320_mha": (1, 320, 4, 4), "s320_gqa": (1, 320, 8, 2), "s576": (1, 576, 2, 2)}


def dump(out_dir):
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import torch

    from lpp_amd import ops

    ext = ops.extension()
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    for name, (B, S, H, HKV) in CASES.items():
        g = torch.Generator().manual_seed(20 + S + HKV)
        q = torch.randn(B, S, H, 128, generator=g).to(torch.bfloat16).cuda()
        k = torch.randn(B, S, HKV, 128, generator=g).to(torch.bfloat16).cuda()
        v = torch.randn(B, S, HKV, 128, generator=g).to(torch.bfloat16).cuda()
        do_ = torch.randn(B, S, H, 128, generator=g).to(torch.bfloat16).cuda()
        o, lse = ext.attention_fwd(q, k, v)
        for t, tname in zip(ext.attention_bwd(do_, q, k, v, o, lse), ("dq", "dk", "dv")):
            np.save(out / f"{name}_{tname}.npy", t.cpu().view(torch.int16).numpy())
    print(f"wrote {3 * len(CASES)} arrays to {out}")


def compare(a, b):
    bad = []
    for name in CASES:
        for tname in ("dq", "dk", "dv"):
            f = f"{name}_{tname}.npy"
            same = np.array_equal(np.load(Path(a) / f), np.load(Path(b) / f))
            print(f"{f}: {'equal' if same else 'DIFFERENT'}")
            if not same:
                bad.append(f)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("dirs", nargs="+")
    args = ap.parse_args()
    if args.compare:
        if len(args.dirs) != 2:
            ap.error("--compare takes two directories")
        sys.exit(compare(*args.dirs))
    dump(args.dirs[0])


if __name__ == "__main__":
    main()
