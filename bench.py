#!/usr/bin/env python
"""Flagship benchmark: LLaMA-65B pipeline-parallel training throughput on
MI355X (BASELINE.json metric: "tokens/sec (whole node), LLaMA-65B PP=8
seq4096 at 1/2/4/8 MI355X").

Weak scaling over pipeline depth: each GPU holds one 65B-shaped stage
(hidden 8192, heads 64, intermediate 22016 — 10 of the 80 decoder layers
per stage).  At --gpus 8 this is the full LLaMA-65B with PP=8; at smaller N
the model is the first N/8 slice of it, so per-GPU work is fixed as N grows
and the ideal scaling curve is FLAT tokens/s (the model grows with N; any
drop measures pipeline bubble + p2p cost).

Synthetic data (random tokens of the BASELINE shape), random-init weights,
bf16 compute, fp32 grad accumulation + master AdamW.  Activation
checkpointing is SELECTIVE: the auto policy recomputes only as many layers
per stage as the 288 GB memory budget demands (usually zero).  Nothing is
skipped inside the timed region: each step runs `gas` microbatches
forward+backward plus the full optimizer step.

Launch (the driver's contract):
  python bench.py --gpus 1 --steps 3 --warmup 1
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line.
--dump-outputs DIR also writes what the last timed step computed (its loss
and a seeded sample of the updated parameters and Adam first moments) as
DIR/<name>.npy, identical inputs for identical arguments, so two builds can
be compared output for output.  --full is where secondary measurements go;
the benchmark has none of its own today (per-op and serving figures live in
scripts/), so the flag changes nothing yet.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

from lpp_amd.config import TrainConfig, model_config
from lpp_amd.data import CausalLMCollator, RepeatingLoader, SyntheticCausalLMDataset
from lpp_amd.engine import PipelineEngine
from lpp_amd.models import RMSNorm, get_layers_from_config, loss_fn
from lpp_amd.pipeline_module import PipelineModule
from lpp_amd.topology import ProcessGrid
from lpp_amd.utils import init_distributed, set_seed


@torch.no_grad()
def fast_random_init(module: PipelineModule, std: float, seed: int) -> None:
    """On-device random init (normal(0, std) matrices, ones for norms).
    Per-param generator seeding keeps it deterministic per rank."""
    dev = next(module.parameters()).device
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 1000 * module.grid.rank)
    for m in module.modules():
        if isinstance(m, RMSNorm):
            m.weight.fill_(1.0)
        elif isinstance(m, (torch.nn.Linear, torch.nn.Embedding)):
            m.weight.normal_(0.0, std, generator=g)


DUMP_SAMPLE_PER_PARAM = 4096  # elements sampled from each parameter tensor


@torch.no_grad()
def dump_outputs(out_dir: str, module: PipelineModule, optimizer, losses,
                 rank: int, world: int) -> None:
    """Write what the last timed train_batch() handed its caller as .npy:
    the returned loss (plus the loss of every timed step) and the model and
    optimizer state it updated in place.  Those are far above the 64 MB
    cap, so a fixed seeded sample of DUMP_SAMPLE_PER_PARAM elements per
    tensor is written instead (same indices every run: comparable build to
    build)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    prefix = f"rank{rank}_" if world > 1 else ""
    if rank == 0:  # the loss is identical on every rank
        np.save(os.path.join(out_dir, "loss.npy"),
                np.asarray(losses[-1:], dtype=np.float64))
        np.save(os.path.join(out_dir, "step_losses.npy"),
                np.asarray(losses, dtype=np.float64))

    def save_sample(name: str, tensors) -> None:
        g = torch.Generator(device="cpu")
        g.manual_seed(4321)
        chunks = []
        for t in tensors:
            flat = t.detach().reshape(-1)
            n = flat.numel()
            if n > DUMP_SAMPLE_PER_PARAM:
                idx = torch.randint(0, n, (DUMP_SAMPLE_PER_PARAM,), generator=g)
                flat = flat[idx.to(flat.device)]
            chunks.append(flat.float().cpu())
        if chunks:
            np.save(os.path.join(out_dir, f"{prefix}{name}.npy"),
                    torch.cat(chunks).numpy())

    save_sample("params_sample", module.parameters())
    # Adam first moment = running mean of the accumulated gradients: the
    # part of the updated state most sensitive to the backward kernels
    save_sample("grad_moment_sample", optimizer.exp_avg)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gas", type=int, default=0,
                    help="microbatches per step (0 = auto: 64 // micro_batch_size)")
    ap.add_argument("--micro-batch-size", type=int, default=0,
                    help="0 = auto by pipeline depth: bigger microbatches where "
                         "activations fit and the bubble stays small")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--model", type=str, default="llama-65b")
    ap.add_argument("--layers-per-stage", type=int, default=10,
                    help="decoder layers per GPU (65B/8 = 10)")
    ap.add_argument("--dp", type=int, default=1, help="data-parallel degree")
    ap.add_argument("--dtype", type=str, default="bf16")
    ap.add_argument("--act-ckpt", type=str, default="auto", choices=("auto", "0", "1"),
                    help="activation checkpointing: auto = only when the full "
                         "activations would not fit in 288 GB HBM")
    ap.add_argument("--p2p-overlap", type=int, default=1,
                    help="1 = pre-posted p2p on dedicated channels (default), "
                         "0 = serial blocking exchanges (A/B baseline)")
    ap.add_argument("--overlap-allreduce", type=int, default=1,
                    help="1 = DP bucket all-reduce launched during the final "
                         "backward (default), 0 = boundary all-reduce")
    ap.add_argument("--watchdog", type=float, default=900.0,
                    help="seconds before the deadlock watchdog dumps per-rank "
                         "schedule position (0 = off)")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps write the last step's loss and a "
                         "seeded sample of the updated state as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement; a plain run does "
                         "only what the headline figure needs (there is none "
                         "today: the flag is accepted and changes nothing)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    n_gpus = max(world, 1)
    if world > 1:
        init_distributed()

    on_gpu = torch.cuda.is_available()
    if on_gpu:
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    else:
        device = torch.device("cpu")

    num_stages = world // args.dp if world > 1 else 1
    dp = args.dp if world > 1 else 1
    # weak scaling: model depth grows with pipeline depth
    num_layers = args.layers_per_stage * num_stages
    mcfg = model_config(args.model, num_layers=num_layers, max_seq_len=args.seq_len)

    # MI355X-first schedule/memory policy (lpp_amd.utils.schedule)
    from lpp_amd.utils.schedule import choose_schedule

    sched = choose_schedule(mcfg, num_stages, args.layers_per_stage, args.seq_len,
                            args.micro_batch_size, args.gas)
    args.micro_batch_size = sched.micro_batch_size
    args.gas = sched.gas
    if args.act_ckpt == "auto":
        ckpt_per_stage = sched.ckpt_layers_per_stage
    elif args.act_ckpt == "1":
        ckpt_per_stage = args.layers_per_stage
    else:
        ckpt_per_stage = 0
    lps = args.layers_per_stage

    def _ckpt_fn(i: int) -> bool:
        return (i % lps) < ckpt_per_stage  # each stage checkpoints its first k

    cfg = TrainConfig(
        model=mcfg,
        num_stages=num_stages,
        micro_batch_size=args.micro_batch_size,
        gradient_accumulation_steps=args.gas,
        seq_len=args.seq_len,
        dtype=args.dtype if on_gpu else "fp32",
        activation_checkpoint_interval=0,  # per-layer selective instead
        p2p_overlap=bool(args.p2p_overlap),
        overlap_allreduce=bool(args.overlap_allreduce),
        watchdog_timeout_s=args.watchdog,  # armed by default: the first
        # multi-GPU deadlock dumps per-rank schedule positions
    )
    cfg.optimizer.lr = 1e-5
    cfg.optimizer.total_num_steps = 1000

    set_seed(1234, rank)
    grid = ProcessGrid(max(world, 1), rank, num_stages)
    grid.build_groups()

    from lpp_amd.config import torch_dtype

    module = PipelineModule(
        get_layers_from_config(mcfg, checkpoint_fn=_ckpt_fn),
        grid,
        loss_fn=loss_fn,
        activation_checkpoint_interval=0,
        device=device,
        dtype=torch_dtype(cfg.dtype),
    )
    fast_random_init(module, mcfg.initializer_range, seed=1234)
    engine = PipelineEngine(module, cfg, grid, device=device)

    # data: only first/last stage iterate
    n_examples = args.gas * args.micro_batch_size * (args.steps + args.warmup + 1)
    ds = SyntheticCausalLMDataset(n_examples, args.seq_len, mcfg.vocab_size, seed=7)
    loader = torch.utils.data.DataLoader(
        ds, batch_size=args.micro_batch_size, shuffle=False,
        collate_fn=CausalLMCollator(args.seq_len), drop_last=True,
    )
    it = iter(RepeatingLoader(loader))

    def sync():
        if dist.is_initialized():
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        engine.train_batch(it)
    engine.timer_summary(reset=True)  # timers cover only the timed steps

    sync()
    t0 = time.time()
    step_losses = []
    for _ in range(args.steps):
        step_losses.append(float(engine.train_batch(it)))
    last_loss = step_losses[-1]
    sync()
    elapsed = time.time() - t0

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, module, engine.optimizer, step_losses, rank, world)

    # MAX elapsed over ranks (ranks are barrier-synced; take max anyway)
    t = torch.tensor([elapsed], dtype=torch.float64)
    if dist.is_initialized():
        t_dev = t.to(device) if on_gpu else t
        dist.all_reduce(t_dev, op=dist.ReduceOp.MAX)
        elapsed = float(t_dev.item())

    tokens_per_step = args.gas * args.micro_batch_size * args.seq_len * dp
    tokens_per_sec = tokens_per_step * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    # per-rank section timers (DEVICE-measured hipEvent pairs, seconds over
    # the timed steps) so a multi-GPU run's bubble/p2p/compute split is
    # diagnosable from the JSON: fwd/bwd are compute-stream kernel time,
    # p2p/allreduce are comm-wait stalls suffered by the compute stream
    tsum = engine.timer_summary()
    tvec = torch.tensor([tsum["forward"], tsum["backward"], tsum["p2p"],
                         tsum["allreduce"], tsum["optimizer"]], dtype=torch.float64)
    if dist.is_initialized():
        gathered = [torch.zeros_like(tvec) for _ in range(world)]
        dist.all_gather(gathered, tvec)
    else:
        gathered = [tvec]
    stage_timers = [
        {"rank": i, "fwd_s": round(float(g[0]), 2), "bwd_s": round(float(g[1]), 2),
         "p2p_s": round(float(g[2]), 2), "allreduce_s": round(float(g[3]), 2),
         "optim_s": round(float(g[4]), 2)}
        for i, g in enumerate(gathered)
    ]

    if rank == 0:
        par = f"pp{num_stages}" + (f"_dp{dp}" if dp > 1 else "")
        result = {
            "metric": "tokens/sec (whole node), LLaMA-65B PP=8 seq4096 at 1/2/4/8 MI355X",
            "value": round(tokens_per_sec, 2),
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": cfg.dtype,
            "data": "synthetic",
            "config": {
                "model": args.model,
                # honest shape label: below 8 GPUs this measures the first
                # num_layers-layer slice of the 65B model (weak scaling per
                # stage); only n_gpus=8/pp8 runs the full headline model
                "measured_model": (
                    args.model if num_layers >= model_config(args.model).num_layers
                    else f"{args.model}-shaped {num_layers}-layer slice "
                         f"({num_layers}/{model_config(args.model).num_layers} layers)"),
                "global_batch": args.gas * args.micro_batch_size * dp,
                "seq_len": args.seq_len,
                "parallelism": par,
                "layers_per_stage": args.layers_per_stage,
                "num_layers": num_layers,
                "micro_batch_size": args.micro_batch_size,
                "grad_accum_steps": args.gas,
                "ckpt_layers_per_stage": ckpt_per_stage,
                "last_loss": round(last_loss, 4),
                "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 2)
                if on_gpu
                else None,
                "stage_timers": stage_timers,
            },
        }
        print(json.dumps(result), flush=True)

    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
