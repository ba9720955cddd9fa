#!/usr/bin/env python
"""Dump the attention forward's and backward's outputs for a build-to-build
comparison.

Inputs come from a seeded CPU generator, so two builds of the extension see
the same bits: S=1, S=200, S=320 (MHA and GQA) and S=576, bf16, D=128.  Writes
<case>_{o,lse2,dq,dk,dv}.npy (bit patterns: bf16 as int16, fp32 as int32) into
the directory.  --digest prints one sha256 per array instead, for shapes too
large to keep (the production shape by default).

    python scripts/attn_dump.py OUT_DIR            # in each checkout
    python scripts/attn_dump.py --compare DIR_A DIR_B
    python scripts/attn_dump.py --digest [B S H HKV]
"""
import argparse
import hashlib
import sys
from pathlib import Path

import numpy as np

CASES = {
    "s1": (1, 1, 2, 2),
    "s200": (1, 200, 2, 2),
    "s320_mha": (1, 320, 4, 4),
    "s320_gqa": (1, 320, 8, 2),
    "s576": (1, 576, 2, 2),
}
ARRAYS = ("o", "lse2", "dq", "dk", "dv")


def run_case(B, S, H, HKV):
    """name -> numpy array of bit patterns, for one seeded case."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import torch

    from lpp_amd import ops

    ext = ops.extension()
    g = torch.Generator().manual_seed(20 + S + HKV)
    q = torch.randn(B, S, H, 128, generator=g).to(torch.bfloat16).cuda()
    k = torch.randn(B, S, HKV, 128, generator=g).to(torch.bfloat16).cuda()
    v = torch.randn(B, S, HKV, 128, generator=g).to(torch.bfloat16).cuda()
    do_ = torch.randn(B, S, H, 128, generator=g).to(torch.bfloat16).cuda()
    o, lse = ext.attention_fwd(q, k, v)
    dq, dk, dv = ext.attention_bwd(do_, q, k, v, o, lse)
    bits = {"o": o.view(torch.int16), "lse2": lse.view(torch.int32)}
    bits.update({n: t.view(torch.int16) for n, t in (("dq", dq), ("dk", dk), ("dv", dv))})
    return {n: t.cpu().numpy() for n, t in bits.items()}


def dump(out_dir):
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    for name, shape in CASES.items():
        for tname, arr in run_case(*shape).items():
            np.save(out / f"{name}_{tname}.npy", arr)
    print(f"wrote {len(ARRAYS) * len(CASES)} arrays to {out}")


def digest(shape):
    for tname, arr in run_case(*shape).items():
        print(f"{'x'.join(map(str, shape))}_{tname} {hashlib.sha256(arr.tobytes()).hexdigest()}")


def compare(a, b):
    bad = []
    for name in CASES:
        for tname in ARRAYS:
            f = f"{name}_{tname}.npy"
            same = np.array_equal(np.load(Path(a) / f), np.load(Path(b) / f))
            print(f"{f}: {'equal' if same else 'DIFFERENT'}")
            if not same:
                bad.append(f)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("args", nargs="*")
    args = ap.parse_args()
    if args.compare:
        if len(args.args) != 2:
            ap.error("--compare takes two directories")
        sys.exit(compare(*args.args))
    if args.digest:
        if len(args.args) not in (0, 4):
            ap.error("--digest takes B S H HKV, or nothing for 4 4096 64 64")
        return digest(tuple(int(x) for x in args.args) or (4, 4096, 64, 64))
    if len(args.args) != 1:
        ap.error("one output directory")
    dump(args.args[0])


if __name__ == "__main__":
    main()
