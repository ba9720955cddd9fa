#!/usr/bin/env python
"""Real (non-padding) tokens per second of one training stage with
pack_sequences on and off, on one GPU.

The corpus is generated here: --examples prompt/response pairs whose total
length in words is log-normal (median ~180, sigma 0.9, clipped to 8..seq_len-2),
one third of it prompt.  Both runs train the same 65B-shaped stage (--layers
decoder layers, hidden 8192, 64 heads) on it through the jsonl path; the result
depends on that length distribution: the shorter the examples against seq_len,
the more padding the unpacked run pays for.

    python scripts/packed_e2e_bench.py [--seq 4096 --layers 2 --steps 6 --warmup 2]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def write_corpus(path, n, seq_len, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    with open(path, "w") as f:
        for i in range(n):
            total = int(torch.exp(torch.randn((), generator=g) * 0.9 + 5.2).clamp(8, seq_len - 2))
            a = max(1, total // 3)
            f.write(json.dumps({"inputs": " ".join(f"w{(i * 7 + j) % 5000}" for j in range(a)),
                                "targets": " ".join(f"w{(i * 11 + j) % 5000}"
                                                    for j in range(total - a))}) + "\n")


def run(train_file, pack, a):
    import torch

    from lpp_amd.config import TrainConfig, model_config, torch_dtype
    from lpp_amd.data import RepeatingLoader, build_loader
    from lpp_amd.engine import PipelineEngine
    from lpp_amd.models import get_layers_from_config, loss_fn
    from lpp_amd.pipeline_module import PipelineModule
    from lpp_amd.topology import ProcessGrid
    from lpp_amd.trainer import build_dataset

    mcfg = model_config("llama-65b", num_layers=a.layers, max_seq_len=a.seq)
    cfg = TrainConfig(model=mcfg, num_stages=1, micro_batch_size=1,
                      gradient_accumulation_steps=a.gas, seq_len=a.seq, dtype="bf16",
                      data_kind="jsonl", train_file=train_file, tokenizer_path="simple",
                      pack_sequences=pack)
    device = torch.device("cuda", 0)
    grid = ProcessGrid(1, 0, 1)
    torch.manual_seed(0)
    module = PipelineModule(get_layers_from_config(mcfg), grid, loss_fn=loss_fn,
                            activation_checkpoint_interval=1, device=device,
                            dtype=torch_dtype("bf16"))
    with torch.no_grad():
        for p in module.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    engine = PipelineEngine(module, cfg, grid, device=device)
    ds, collate = build_dataset(cfg)
    pad = 3  # SimpleTokenizer's [PAD]
    real = [0]

    def counted(it):
        for batch in it:
            real[0] += int((batch["input_ids"] != pad).sum())
            yield batch

    loader = build_loader(ds, 1, 1, 0, seed=0, num_workers=0, collator=collate)
    it = counted(iter(RepeatingLoader(loader)))
    for _ in range(a.warmup):
        engine.train_batch(it)
    torch.cuda.synchronize()
    real[0] = 0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = engine.train_batch(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rows = a.steps * a.gas
    return {"pack_sequences": pack, "rows_in_dataset": len(ds), "rows_run": rows,
            "real_tokens": real[0], "fill": real[0] / (rows * a.seq), "seconds": dt,
            "real_tokens_per_s": real[0] / dt, "row_tokens_per_s": rows * a.seq / dt,
            "loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--gas", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--examples", type=int, default=2000)
    ap.add_argument("--only", choices=["on", "off"], default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "corpus.jsonl")
        write_corpus(path, a.examples, a.seq, seed=5)
        for pack in (False, True):
            if a.only and (a.only == "on") != pack:
                continue
            r = run(path, pack, a)
            r.update(seq=a.seq, layers=a.layers, gas=a.gas, examples=a.examples)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
