#!/usr/bin/env python
"""Paged against slot KV cache: decode and extend attention at the points
scripts/decode_bench.py (--quick) and scripts/extend_bench.py sweep.

Both layouts hold the same data (the pool is the slot cache cut into 64-token
pages under a shuffled table), run in one process and alternate, three windows
each, so the spread shows next to the difference.  Device events around
`reps` launches (extend: a quarter of that), so that a window is tens of
milliseconds; us per call.  --direct calls the extension, not the ops, which
leaves out the Python wrapper's share of a small call.

    python scripts/paged_attn_bench.py [--reps 4000] [--kv-dtype fp8] [--direct]
"""

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from lpp_amd import ops  # noqa: E402

D, PAGE = 128, 64
EXTEND_POINTS = [(1, 512, 0), (1, 512, 3584), (4, 128, 2048), (8, 8, 4000)]  # N, Sq, p; 64/8


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
    return e0.elapsed_time(e1) * 1e3 / reps


def _caches(N, L, Hkv, fp8, g, dev):
    """(slot args, pool args, table): the same random cache in both layouts."""
    L = -(-L // PAGE) * PAGE
    M = L // PAGE
    kv = [torch.randn(N, L, Hkv, D, generator=g, device=dev).bfloat16() for _ in range(2)]
    scales = []
    if fp8:
        (k, ks), (v, vs) = (ops.quantize_kv_rows_fp8(t) for t in kv)
        kv, scales = [k, v], [ks.transpose(1, 2).contiguous(), vs.transpose(1, 2).contiguous()]
    table = torch.randperm(N * M, generator=torch.Generator().manual_seed(0)).view(M, N).T
    table = table.contiguous().to(torch.int32).to(dev)
    bt = table.long()
    pool = []
    for x in kv:
        p = torch.empty(N * M, PAGE, Hkv, D, dtype=x.dtype, device=dev)
        p.view(torch.uint8)[bt] = x.view(N, M, PAGE, Hkv, D).view(torch.uint8)
        pool.append(p)
    for s in scales:
        p = torch.empty(N * M, Hkv, PAGE, device=dev)
        p[bt] = s.view(N, Hkv, M, PAGE).transpose(1, 2)
        pool.append(p)
    return kv + scales, pool, table


def _row(label, fns, reps):
    t = {name: [] for name in fns}
    for _ in range(3):
        for name, fn in fns.items():
            t[name].append(_time(fn, 50, reps))
    s, p = t["slot"], t["paged"]
    print(f"{label} | {s[0]:8.2f} {s[1]:8.2f} {s[2]:8.2f} | {p[0]:8.2f} {p[1]:8.2f} {p[2]:8.2f} | "
          f"{min(p) / min(s):6.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4000)
    ap.add_argument("--direct", action="store_true", help="call the extension, not the ops")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "paged_attn_bench needs a GPU"
    fp8 = args.kv_dtype == "fp8"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev).bfloat16()
    kw = lambda c: dict(k_scale=c[2], v_scale=c[3]) if fp8 else {}
    ext = ops.extension()
    print(f"# paged vs slot, {args.kv_dtype} cache, {'extension' if args.direct else 'ops'} calls, "
          f"us per call, three windows each, alternating; ratio = best paged / best slot")
    print(f"# decode   {'H/Hkv':>7} {'N':>3} {'L':>5} | {'slot':>26} | {'paged':>26} | ratio")
    for H, Hkv in ((64, 8), (128, 8)):
        for L in (512, 4096):
            for N in (1, 8, 32):
                pos_h = [L - 1] if N == 1 else [int(L // 4 + (L - 1 - L // 4) * i / (N - 1))
                                                for i in range(N)]
                slot, pool, table = _caches(N, L, Hkv, fp8, g, dev)
                pos = torch.tensor(pos_h, device=dev)
                q, k, v = rn(N, 1, H, D), rn(N, 1, Hkv, D), rn(N, 1, Hkv, D)
                cos, sin = ops.build_rope_cache(L, D, 10000.0, dev)
                call = lambda c, **t: lambda: ops.decode_attention(
                    q, k, v, c[0], c[1], cos, sin, pos, max_len=max(pos_h) + 1, **kw(c), **t)
                if args.direct and fp8:
                    call = lambda c, block_table=None: lambda: ext.attention_decode_fp8(
                        q, k, v, c[0], c[1], c[2], c[3], cos, sin, pos, None, None, 0,
                        max(pos_h) + 1, 0, block_table)
                elif args.direct:
                    call = lambda c, block_table=None: lambda: ext.attention_decode(
                        q, k, v, c[0], c[1], cos, sin, pos, None, None, 0, max(pos_h) + 1, 0, 0,
                        block_table)
                _row(f"  decode   {H:>4}/{Hkv:<2} {N:>3} {L:>5}",
                     dict(slot=call(slot), paged=call(pool, block_table=table)), args.reps)
    print(f"# extend 64/8 {'N':>3} {'Sq':>4} {'p':>5} | {'slot':>26} | {'paged':>26} | ratio")
    for N, Sq, p in EXTEND_POINTS:
        slot, pool, table = _caches(N, p + Sq, 8, fp8, g, dev)
        q, k, v = rn(N, Sq, 64, D), rn(N, Sq, 8, D), rn(N, Sq, 8, D)
        cos, sin = ops.build_rope_cache(p + Sq, D, 10000.0, dev)
        call = lambda c, **t: lambda: ops.extend_attention(
            q, k, v, c[0], c[1], cos, sin, p, max_len=p + Sq, **kw(c), **t)
        _row(f"  extend     {N:>3} {Sq:>4} {p:>5}",
             dict(slot=call(slot), paged=call(pool, block_table=table)), max(args.reps // 4, 10))
        # (extend stays on the ops call: at 35 us and more the wrapper does not show)


if __name__ == "__main__":
    main()
