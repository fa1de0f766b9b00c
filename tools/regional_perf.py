#!/usr/bin/env python3
"""Regional cross-attention: the fused route (one multi-context blend
kernel) against the per-region loop, per layer and per generation.

Per layer: CrossAttention.forward on a RegionalContext at the SD1.5 / SDXL
cross-attention shapes (8 cond + 8 uncond rows, Sk=77), R in {2, 3}, columns
and rows masks. Both routes run in this process, alternating, after a
warm-up; one sample is at least --sample-seconds of work between two device
events. Reported: the median per-call time of each route and the spread
((max - min) / median over the samples).

Per generation: one regional txt2img at 512x512, 20 steps, batch 8, both
ways, alternating, --gen-repeats times each after a warm-up generation.

Prints a table per part and one JSON line at the end. No GPU: fails.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sdwd_amd.models.unet import CrossAttention, RegionalContext  # noqa: E402
from sdwd_amd.pipeline.pipeline import _region_masks  # noqa: E402

NR = 8  # cond rows; the batch is 2 * NR (cfg-doubled)
# (tag, S, heads, D, context dim)
SHAPES = [
    ("sd15-320", 4096, 8, 40, 768),
    ("sd15-640", 1024, 8, 80, 768),
    ("sd15-1280", 256, 8, 160, 768),
    ("sd15-mid", 64, 8, 160, 768),
    ("sdxl-640", 4096, 10, 64, 2048),
    ("sdxl-1280", 1024, 20, 64, 2048),
]


def _sample(fn, iters):
    """ms per call over `iters` calls between two device events."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def _stats(xs):
    med = statistics.median(xs)
    return med, (max(xs) - min(xs)) / med


def layer_case(tag, s, heads, dh, cdim, r, mode, args):
    d = heads * dh
    side = int(round(s ** 0.5))
    torch.manual_seed(s + dh + r)
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    attn = CrossAttention(d, cdim, heads).eval().to(dev, bf)
    x = torch.randn(2 * NR, s, d, device=dev, dtype=bf)
    rc = RegionalContext(
        torch.randn(2 * NR, 77, cdim, device=dev, dtype=bf),
        torch.randn(r, 77, cdim, device=dev, dtype=bf),
        _region_masks(mode, [1.0] * r, side, side).to(dev), rows=NR,
        base_ratio=0.2, lat_hw=(side, side))

    def call(fused):
        CrossAttention.fused_regional = fused
        with torch.no_grad():
            return attn(x, rc)

    for fused in (True, False):  # warm-up: caches, kernel load, GEMM tuning
        for _ in range(3):
            call(fused)
    torch.cuda.synchronize()
    iters = {}
    for fused in (True, False):
        ms = _sample(lambda: call(fused), 5)
        iters[fused] = max(5, int(args.sample_seconds * 1e3 / ms) + 1)
    times = {True: [], False: []}
    for _ in range(args.samples):
        for fused in (True, False):  # alternating
            times[fused].append(_sample(lambda: call(fused), iters[fused]))
    fm, fs = _stats(times[True])
    lm, ls = _stats(times[False])
    row = {"shape": tag, "S": s, "D": dh, "R": r, "mode": mode,
           "fused_ms": round(fm, 4), "fused_spread": round(fs, 4),
           "loop_ms": round(lm, 4), "loop_spread": round(ls, 4),
           "loop_over_fused": round(lm / fm, 3)}
    print(f"{tag:10s} S={s:<5d} D={dh:<4d} R={r} {mode:8s} "
          f"fused {fm:8.4f} ms (+-{fs:6.2%})  loop {lm:8.4f} ms "
          f"(+-{ls:6.2%})  loop/fused {lm / fm:5.2f}x", flush=True)
    return row


def generation(args):
    from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

    pipe = StableDiffusionPipeline("sd15", device="cuda:0",
                                   dtype=torch.bfloat16)
    req = PipelineRequest(
        prompt="a valley BREAK a red barn BREAK a blue lake", steps=20,
        width=512, height=512, seeds=list(range(100, 108)),
        regional_mode="columns", regional_ratios="1,1",
        regional_base_ratio=0.2)

    def gen(fused):
        CrossAttention.fused_regional = fused
        torch.cuda.synchronize()
        res = pipe.generate(req)
        torch.cuda.synchronize()
        assert "RP Active: True" in res.infotexts[0]
        return res.elapsed

    for fused in (True, False):
        gen(fused)
    times = {True: [], False: []}
    for _ in range(args.gen_repeats):
        for fused in (True, False):
            times[fused].append(gen(fused))
    fm, fs = _stats(times[True])
    lm, ls = _stats(times[False])
    print(f"generation 512x512 20 steps batch 8 columns R=2: fused {fm:.3f} s "
          f"(+-{fs:.2%})  loop {lm:.3f} s (+-{ls:.2%})  "
          f"loop/fused {lm / fm:.3f}x", flush=True)
    return {"fused_s": round(fm, 4), "fused_spread": round(fs, 4),
            "loop_s": round(lm, 4), "loop_spread": round(ls, 4),
            "samples": {"fused": times[True], "loop": times[False]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--sample-seconds", type=float, default=0.5)
    ap.add_argument("--gen-repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="substring filter on shape")
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--skip-generation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regional_perf: a GPU is required")
    default = CrossAttention.fused_regional
    out = {"layers": [], "generation": None}
    try:
        if not args.skip_layers:
            for tag, s, heads, dh, cdim in SHAPES:
                if args.only and args.only not in tag:
                    continue
                for r in (2, 3):
                    for mode in ("columns", "rows"):
                        out["layers"].append(
                            layer_case(tag, s, heads, dh, cdim, r, mode, args))
        if not args.skip_generation:
            out["generation"] = generation(args)
    finally:
        CrossAttention.fused_regional = default
    print(json.dumps(out))


if __name__ == "__main__":
    main()
