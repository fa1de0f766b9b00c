#!/usr/bin/env python3
"""Token merging: one level-0 transformer block and one generation, timed.

Per block: BasicTransformerBlock at C=320, H=8 heads, batch 16, N=4096
(64x64) and N=16384 (128x128), ratio 0 / 0.3 / 0.5 / 0.75. The whole block
is timed native (tome.hip kernels) and composed (torch route), alternating,
after a warm-up; one sample is at least --sample-seconds of work between two
device events. The native route is also split into match / plan / merge /
attn1 / add+LN, each stage timed alone on the tensors of a real forward.
"overhead" is match + plan + merge plus what the gathered add+LN costs over
the plain one at ratio 0: everything token merging adds around attn1.

Per generation: one txt2img at the headline configuration (sd15, 512x512,
20 steps, --gen-batch images) at ratio 0 and 0.5, alternating, --gen-repeats
times each after a warm-up generation of each.

Prints a table per part and one JSON line at the end. No GPU: fails.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sdwd_amd import ops  # noqa: E402
from sdwd_amd.models.layers import _fp32_cached  # noqa: E402
from sdwd_amd.models.unet import BasicTransformerBlock  # noqa: E402

B, C, HEADS, CTX = 16, 320, 8, 768
SIDES = [64, 128]
RATIOS = [0.0, 0.3, 0.5, 0.75]


def _sample(fn, iters):
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


def _timed(fns, args):
    """{name: (median ms, spread)} of the callables, alternating."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    iters = {}
    for name, fn in fns.items():
        ms = _sample(fn, 3)
        iters[name] = max(3, int(args.sample_seconds * 1e3 / ms) + 1)
    times = {name: [] for name in fns}
    for _ in range(args.samples):
        for name, fn in fns.items():
            times[name].append(_sample(fn, iters[name]))
    return {name: _stats(xs) for name, xs in times.items()}


def block_case(side, ratio, args):
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(side)
    blk = BasicTransformerBlock(C, CTX, HEADS).eval().to(dev, bf)
    blk.tome_ratio = ratio
    n = side * side
    x = torch.randn(B, n, C, device=dev, dtype=bf)
    ctx = torch.randn(B, 77, CTX, device=dev, dtype=bf)
    hw = (side, side)

    def whole(native):
        blk.tome_native = native
        with torch.no_grad():
            return blk(x, ctx, hw)

    fns = {"native": lambda: whole(True)}
    if ratio > 0:
        fns["composed"] = lambda: whole(False)
    row = {"N": n, "ratio": ratio}
    for name, (med, spread) in _timed(fns, args).items():
        row[f"{name}_ms"] = round(med, 4)
        row[f"{name}_spread"] = round(spread, 4)

    # the native route's stages, each alone on the tensors of one forward
    blk.tome_native = True
    w2, b2 = _fp32_cached(blk.norm2)
    with torch.no_grad():
        n1 = blk.norm1(x)
        if ratio > 0:
            r = ops.tome_merge_count(side, side, ratio)
            node_max, node_idx = ops.tome_match(x, side, side)
            plan = ops.tome_plan(node_max, node_idx, side, side, r)
            merged = ops.tome_merge(n1, plan)
            h = blk.attn1(merged)
            stages = {
                "match": lambda: ops.tome_match(x, side, side),
                "plan": lambda: ops.tome_plan(node_max, node_idx, side,
                                              side, r),
                "merge": lambda: ops.tome_merge(n1, plan),
                "attn1": lambda: blk.attn1(merged),
                "add_ln": lambda: ops.add_layer_norm(
                    x, h, w2, b2, 1e-5, gather=plan.slot),
            }
        else:
            h = blk.attn1(n1)
            stages = {
                "attn1": lambda: blk.attn1(n1),
                "add_ln": lambda: ops.add_layer_norm(x, h, w2, b2, 1e-5),
            }

        def run(fn):
            def call():
                with torch.no_grad():
                    fn()
            return call

        split = _timed({k: run(v) for k, v in stages.items()}, args)
    for name, (med, _) in split.items():
        row[f"{name}_ms"] = round(med, 4)
    line = "  ".join(f"{k} {row[f'{k}_ms']:8.4f}" for k in split)
    comp = f"  composed {row['composed_ms']:8.4f}" if ratio > 0 else ""
    print(f"N={n:<6d} ratio {ratio:<5} block {row['native_ms']:8.4f} ms "
          f"(+-{row['native_spread']:6.2%}){comp}  |  {line}", flush=True)
    return row


def generation(args):
    from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

    pipe = StableDiffusionPipeline("sd15", device="cuda:0",
                                   dtype=torch.bfloat16)
    base = dict(
        prompt="A herd of cows grazing at the bottom of a sunny valley",
        steps=20, width=512, height=512,
        seeds=list(range(100, 100 + args.gen_batch)))

    def gen(ratio):
        torch.cuda.synchronize()
        res = pipe.generate(PipelineRequest(**base,
                                            token_merging_ratio=ratio))
        torch.cuda.synchronize()
        assert ("Token merging ratio" in res.infotexts[0]) == (ratio > 0)
        return res.elapsed

    ratios = (0.0, 0.5)
    # every switch of the ratio drops the captured graphs, so a generation
    # includes its capture; the second of two equal-ratio runs does not
    times = {r: [] for r in ratios}
    for _ in range(args.gen_repeats):
        for r in ratios:
            gen(r)  # re-capture after the switch
            times[r].append(gen(r))
    out = {"batch": args.gen_batch}
    for r in ratios:
        med, spread = _stats(times[r])
        out[f"ratio_{r}_s"] = round(med, 4)
        out[f"ratio_{r}_spread"] = round(spread, 4)
        out[f"ratio_{r}_samples"] = [round(t, 4) for t in times[r]]
        print(f"generation 512x512 20 steps batch {args.gen_batch} ratio {r}: "
              f"{med:.3f} s (+-{spread:.2%})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--sample-seconds", type=float, default=0.3)
    ap.add_argument("--gen-repeats", type=int, default=3)
    ap.add_argument("--gen-batch", type=int, default=64)
    ap.add_argument("--skip-blocks", action="store_true")
    ap.add_argument("--skip-generation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tome_perf: a GPU is required")
    default = BasicTransformerBlock.tome_native
    out = {"blocks": [], "generation": None}
    try:
        if not args.skip_blocks:
            for side in SIDES:
                for ratio in RATIOS:
                    out["blocks"].append(block_case(side, ratio, args))
        if not args.skip_generation:
            out["generation"] = generation(args)
    finally:
        BasicTransformerBlock.tome_native = default
    print(json.dumps(out))


if __name__ == "__main__":
    main()
