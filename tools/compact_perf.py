#!/usr/bin/env python3
"""Compact (SRVGG) upscalers: ops.conv_compact against the closest existing
kernel, and the whole model native against native=False, alternating in one
process.

Per input size (512x512 and 1024x1024 by default): the 64 -> 64 PRELU layer
against ops.conv3x3_dense(..., lrelu=0.2) on the same tensors (not a
functional substitute: a scalar slope), the 64 -> 48 SHUFFLE tail, then the
32-conv model. Each figure is the median of --rounds alternating rounds with
the min and max beside it; TF/s is on 2 * H * W * 9 * 64 * Cout.
One JSON object on stdout.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sdwd_amd import ops
from sdwd_amd.models.esrgan import SRVGGNetCompact

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--model-iters", type=int, default=3)
ap.add_argument("--num-conv", type=int, default=32)
ap.add_argument("--skip-model", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "compact_perf needs a GPU"
DEV = "cuda"


def step(fn, warm, it):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(it):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / it


def alternate(runs, it):
    ts = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ts[k].append(step(fn, 2, it))
    out = {}
    for k, v in ts.items():
        v = sorted(v)
        out[k] = {"med": v[len(v) // 2], "min": v[0], "max": v[-1]}
    return out


def row(r, flops=None):
    d = {"ms": round(r["med"] * 1e3, 3),
         "min_max_ms": [round(r["min"] * 1e3, 3), round(r["max"] * 1e3, 3)]}
    if flops:
        d["tf"] = round(flops / r["med"] / 1e12, 1)
    return d


def layer_rows(size):
    g = torch.Generator(device=DEV).manual_seed(size)

    def bf(*shape, s=1.0):
        return (torch.randn(*shape, device=DEV, generator=g) * s).bfloat16()

    x = bf(1, 64, size, size).contiguous(memory_format=torch.channels_last)
    out = torch.empty_like(x)
    w64 = bf(64, 3, 3, 64, s=0.02)
    w48 = bf(48, 3, 3, 64, s=0.02)
    b64, b48, slope = bf(64), bf(48), bf(64, s=0.3)
    base = torch.rand(1, 3, size, size, device=DEV, generator=g).bfloat16()
    r = alternate({
        "compact": lambda: ops.conv_compact(x, w64, b64, slope=slope),
        "dense": lambda: ops.conv3x3_dense(x, w64, b64, out, lrelu=0.2),
        "shuffle": lambda: ops.conv_compact(x, w48, b48, shuffle_base=base),
    }, args.iters)
    px = 2 * size * size * 9 * 64
    return {
        "64->64 compact PRELU": row(r["compact"], px * 64),
        "64->64 conv3x3_dense lrelu": row(r["dense"], px * 64),
        "dense / compact": round(r["dense"]["med"] / r["compact"]["med"], 3),
        "64->48 compact SHUFFLE": row(r["shuffle"], px * 48),
    }


def model_row(size):
    torch.manual_seed(0)
    net = SRVGGNetCompact(64, args.num_conv).eval().to(DEV, torch.bfloat16)
    x = torch.rand(1, 3, size, size, device=DEV, dtype=torch.bfloat16)
    assert net.native_supported(x)
    with torch.no_grad():
        r = alternate({
            "native": lambda: net(x),
            "composed": lambda: net(x, native=False),
        }, args.model_iters)
    flops = 2 * size * size * 9 * (3 * 64 + args.num_conv * 64 * 64 + 64 * 48)
    return {
        "native": row(r["native"], flops),
        "composed": row(r["composed"], flops),
        "speedup": round(r["composed"]["med"] / r["native"]["med"], 3),
        "speedup_worst": round(r["composed"]["min"] / r["native"]["max"], 3),
    }


out = {}
for size in args.sizes:
    out[f"{size}x{size}"] = {"layers": layer_rows(size)}
    if not args.skip_model:
        out[f"{size}x{size}"]["model"] = model_row(size)
print(json.dumps(out, indent=1))
