#!/usr/bin/env python3
"""Benchmark: the BASELINE.json headline metric.

metric: images/sec (whole node), SD1.5 txt2img 512x512 20-step batch=64,
at 1/2/4/8 GPUs (strong scaling: the 64-image batch is sharded across N
ranks by the benchmark-weighted scheduler). Synthetic prompts, random-init
weights (no network for datasets/checkpoints), bf16 on GPU.

Run:  python bench.py --gpus N --steps K --warmup W
N>1 is launched by the driver as
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N ...
(one rank per GPU over RCCL; RANK/WORLD_SIZE read from the env).
One bench "step" = one full generation of the global batch (plan ->
CLIP encode -> 20-step denoise -> VAE decode -> image gather).

A plain run sets up, warms up, times the K steps and prints one JSON result
line. --dump-outputs DIR additionally writes the last timed step's gallery
(images.npy, seeds.npy) so two builds can be compared output for output;
the request and its seeds are fixed, so inputs are identical run to run.
--full is where secondary measurements live (none today).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch


# --dump-outputs budget: the gallery is written whole when it fits, else as
# a fixed, seeded sample of its elements (same indices on every run, so two
# builds compare element for element)
DUMP_MAX_ELEMS = 4 * 1024 * 1024  # float32 -> 16 MiB
DUMP_SAMPLE_SEED = 0


def dump_outputs(out_dir: str, res) -> None:
    """Write the GalleryResult of the last timed step as .npy files:
    images.npy (float32; the uint8 gallery [N,H,W,3] flattened, or a seeded
    sample of it) and seeds.npy (float64, one per gallery image)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    flat = res.images.reshape(-1).numpy()
    if flat.size > DUMP_MAX_ELEMS:
        rng = np.random.default_rng(DUMP_SAMPLE_SEED)
        idx = rng.integers(0, flat.size, size=DUMP_MAX_ELEMS)
        flat = flat[idx]
        images = flat.astype(np.float32)
    else:
        images = res.images.numpy().astype(np.float32)
    np.save(os.path.join(out_dir, "images.npy"), images)
    np.save(os.path.join(out_dir, "seeds.npy"),
            np.asarray(res.seeds, dtype=np.float64))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed bench steps")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", type=str, default="sd15")
    ap.add_argument("--global-batch", type=int, default=64)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--denoise-steps", type=int, default=20)
    ap.add_argument("--sampler", type=str, default="Euler a")
    ap.add_argument("--cfg", type=float, default=7.0)
    ap.add_argument("--task", choices=["txt2img", "img2img"], default="txt2img",
                    help="img2img adds VAE encode + strength-limited denoise")
    ap.add_argument("--strength", type=float, default=0.75)
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed "
                         "step returned to DIR/<name>.npy (float32/float64)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements; a plain run "
                         "does only what the headline figure needs (today "
                         "the benchmark has none, so this adds nothing)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.warmup < 0:
        ap.error("--warmup must be >= 0")

    from sdwd_amd.config import add_flags  # noqa: F401  (flag surface)
    from sdwd_amd.parallel import DistributedEngine, GenerationRequest, barrier

    have_gpu = torch.cuda.is_available()
    engine = DistributedEngine(model=args.model)
    rank = engine.rank
    world = engine.world_size
    dev = engine.device

    # homogeneous node: seed equal speeds so the weighted planner runs its
    # real path (it reduces to equal split + remainder round-robin)
    for w in engine.world.workers:
        w.eta.avg_ipm = 60.0

    init_images = None
    if args.task == "img2img":
        g = torch.Generator().manual_seed(7)
        init_images = torch.randint(
            0, 255, (args.global_batch, args.height, args.width, 3),
            generator=g, dtype=torch.uint8,
        )
    req = GenerationRequest(
        prompt="A herd of cows grazing at the bottom of a sunny valley",
        negative_prompt="blurry, low quality",
        batch_size=args.global_batch,
        width=args.width,
        height=args.height,
        steps=args.denoise_steps,
        cfg_scale=args.cfg,
        sampler_name=args.sampler,
        seed=1234,
        init_images=init_images,
        denoising_strength=args.strength,
    )

    def sync():
        if have_gpu:
            torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        engine.generate(req)
    sync()
    barrier()
    sync()

    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = engine.generate(req)
    sync()
    barrier()
    sync()
    elapsed = time.perf_counter() - t0

    # MAX over ranks (the slowest rank defines the job)
    from sdwd_amd.parallel import allgather_floats

    all_elapsed = allgather_floats([elapsed], dev if have_gpu else "cpu")
    elapsed = max(v[0] for v in all_elapsed)

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, res)

    if rank == 0:
        total_images = args.global_batch * args.steps
        value = total_images / elapsed
        out = {
            "metric": "images/sec (whole node) SD1.5 txt2img 512x512 "
                      "20-step batch=64 at 1/2/4/8 GPU",
            "value": round(value, 4),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1000.0 / args.steps, 2),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "bf16" if have_gpu else "fp32",
            "data": "synthetic prompts, random-init weights",
            "config": {
                "task": args.task,
                "model": args.model,
                "global_batch": args.global_batch,
                "seq_len": args.width,
                "resolution": f"{args.width}x{args.height}",
                "denoise_steps": args.denoise_steps,
                "sampler": args.sampler,
                "cfg_scale": args.cfg,
                "parallelism": f"dp{world} (benchmark-weighted batch shard)",
            },
        }
        print(json.dumps(out))
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
