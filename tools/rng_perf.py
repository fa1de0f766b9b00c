#!/usr/bin/env python3
"""What does the per-step sampler noise cost, drawn on the host ("CPU") and
on the device ("NV", the fused Philox kernel)?

(a) per noisy step at latents [B,4,64,64] bf16: the device time of the
    kernel alone (events around back-to-back launches) and the wall time of
    the whole step as the sampler runs it (noise_fn() + add_noise for
    CpuNoise, PhiloxNoise.add_to for NV), which is where the host path pays.
(b) the headline generation (SD1.5 512x512, 20 steps, batch 64, "Euler a")
    end to end through StableDiffusionPipeline.generate with randn_source CPU
    and NV, alternating in one process after warming both; the spread of the
    CPU runs among themselves is the same-box noise band.

Needs a GPU (no fallback). Results of record: profiles/r08_device_rng.md.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sdwd_amd import ops  # noqa: E402
from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline  # noqa: E402
from sdwd_amd.pipeline.noise import CpuNoise, PhiloxNoise  # noqa: E402


def _events_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def _wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def per_step(batch, iters, dev):
    shape = (4, 64, 64)
    seeds = list(range(1000, 1000 + batch))
    x = torch.randn(batch, *shape, device=dev, dtype=torch.bfloat16)
    cpu = CpuNoise(seeds, [-1] * batch, 0.0, 0, dev, torch.bfloat16)
    nv = PhiloxNoise(seeds, [-1] * batch, 0.0, 0, dev, torch.bfloat16)
    cpu.shape = nv.shape = shape
    noise = cpu()
    table = nv._main.table
    for _ in range(3):  # warm both routes
        cpu.add_to(x, 1.0, 0.5)
        nv.add_to(x, 1.0, 0.5)
    return {
        "batch": batch,
        "kernel_us_axpby": 1e3 * _events_ms(
            lambda: ops.add_noise(x, noise, 1.0, 0.5), 200),
        "kernel_us_axpby_philox": 1e3 * _events_ms(
            lambda: ops.add_philox_noise(x, table, 7, 1.0, 0.5), 200),
        "wall_us_cpu_step": 1e3 * _wall_ms(
            lambda: cpu.add_to(x, 1.0, 0.5), iters),
        "wall_us_nv_step": 1e3 * _wall_ms(
            lambda: nv.add_to(x, 1.0, 0.5), iters),
    }


def end_to_end(batch, reps, dev):
    pipe = StableDiffusionPipeline("sd15", device=dev, dtype=torch.bfloat16)
    base = dict(
        prompt="A herd of cows grazing at the bottom of a sunny valley",
        negative_prompt="blurry, low quality", steps=20, width=512,
        height=512, cfg_scale=7.0, sampler_name="Euler a",
        seeds=list(range(1234, 1234 + batch)),
    )

    def run(source):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pipe.generate(PipelineRequest(**base, randn_source=source))
        torch.cuda.synchronize()
        assert torch.isfinite(res.images.float()).all()
        return time.perf_counter() - t0

    for source in ("CPU", "NV"):  # graphs, code objects, library choices
        run(source)
    times = {"CPU": [], "NV": []}
    for _ in range(reps):
        for source in ("CPU", "NV"):
            times[source].append(run(source))
    out = {"batch": batch, "reps": reps}
    for source, ts in times.items():
        out[source] = {
            "seconds": [round(t, 4) for t in ts],
            "median_s": round(statistics.median(ts), 4),
            "min_s": round(min(ts), 4),
            "max_s": round(max(ts), 4),
            "images_per_s_median": round(batch / statistics.median(ts), 3),
        }
    med_c, med_n = out["CPU"]["median_s"], out["NV"]["median_s"]
    out["band_pct_cpu_runs"] = round(
        100.0 * (out["CPU"]["max_s"] - out["CPU"]["min_s"]) / med_c, 3)
    out["nv_vs_cpu_pct"] = round(100.0 * (med_c - med_n) / med_c, 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5,
                    help="end-to-end generations per source")
    ap.add_argument("--iters", type=int, default=30,
                    help="noisy steps per wall-time measurement")
    ap.add_argument("--e2e-batch", type=int, default=64)
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rng_perf needs a GPU; nothing is measured without one")
    assert ops.have_ext(), "HIP extension not built"
    dev = torch.device("cuda", 0)
    result = {"per_step": [per_step(b, args.iters, dev) for b in (64, 8)]}
    if not args.skip_e2e:
        result["end_to_end"] = end_to_end(args.e2e_batch, args.reps, dev)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
