#!/usr/bin/env python3
"""SwinIR window attention and the whole 4x model: ops.attention_swin
(swin_attn_bf16_kernel) against the torch route (roll, partition, score
tensor, mask, softmax, reverse, roll back; what SwinIR.forward(native=False)
runs), alternating in one process.

Per token grid (64x64 and 128x128 by default) and head count (6, 8): one
block's attention, shift 4, on the [B, H, W, 3, heads, 32] view of a QKV GEMM
output. GB/s is on the kernel's compulsory traffic: qkv in, the output out,
the bias once; the two routes' outputs are compared at every timed size
before timing. Then SwinIR-L (embed 240, 9 x 6 blocks, 3conv) on a
--image x --image input. Each figure is the median of --rounds alternating
rounds. One JSON object on stdout.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sdwd_amd import ops
from sdwd_amd.models.swinir import SwinIR

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--grids", type=int, nargs="+", default=[64, 128])
ap.add_argument("--heads", type=int, nargs="+", default=[6, 8])
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--image", type=int, default=512)
ap.add_argument("--model-iters", type=int, default=2)
ap.add_argument("--limit", type=float, default=20.0,
                help="seconds a single timing step may take")
ap.add_argument("--skip-model", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "swinir_perf needs a GPU"
DEV = "cuda"


def step(fn, warm, it):
    """Mean seconds per call: `it` calls enqueued, one synchronise."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < it:
        for _ in range(min(10, it - done)):
            fn()
        torch.cuda.synchronize()
        done += min(10, it - done)
        if time.perf_counter() - t0 > args.limit:
            break
    return (time.perf_counter() - t0) / done


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


def attention_row(grid, heads):
    g = torch.Generator(device=DEV).manual_seed(grid + heads)
    b = args.batch
    qkv = torch.randn(b, grid, grid, 3, heads, 32, device=DEV, generator=g,
                      dtype=torch.bfloat16)
    bias = torch.randn(heads, 64, 64, device=DEV, generator=g)
    scale = 30 ** -0.5
    # the outputs at the size that is timed: the kernel is within 3 * 2^-8 *
    # max|v| of the exact result (the tests' bound, p @ |v| <= max|v|), the
    # fp32 torch route within one bf16 rounding, 2^-9 * max|v|
    diff = (ops.attention_swin(qkv, bias, scale, 4).float()
            - ops.attention_swin(qkv, bias, scale, 4, native=False).float()
            ).abs().max().item()
    vmax = qkv[:, :, :, 2].float().abs().max().item()
    assert diff <= 2.0 ** -6 * vmax, (grid, heads, diff, vmax)
    r = alternate({
        "native": lambda: ops.attention_swin(qkv, bias, scale, 4),
        "torch": lambda: ops.attention_swin(qkv, bias, scale, 4, native=False),
    }, args.iters)
    nbytes = qkv.numel() * 2 + qkv.numel() // 3 * 2 + bias.numel() * 4
    us = {k: [round(v[s] * 1e6, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {
        "native_us_med_min_max": us["native"],
        "torch_us_med_min_max": us["torch"],
        "native_gb_s": round(nbytes / r["native"]["med"] / 1e9, 1),
        "compulsory_bytes": nbytes,
        "plan_walk_blocks": list(ops.ext().attention_swin_plan(
            b * (grid // 8) ** 2, heads)),
        "speedup": round(r["torch"]["med"] / r["native"]["med"], 2),
        "max_abs_diff_native_torch": diff,
        "diff_limit": 2.0 ** -6 * vmax,
    }


def model_row(size):
    torch.manual_seed(0)
    net = SwinIR(240, (6,) * 9, 8, 2.0, "3conv").eval().to(DEV, torch.bfloat16)
    x = torch.rand(1, 3, size, size, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        a, b = net(x).float(), net(x, native=False).float()
        diff, amp = (a - b).abs().max().item(), b.abs().max().item()
        del a, b
        r = alternate({
            "native": lambda: net(x),
            "plain": lambda: net(x, native=False),
        }, args.model_iters)
    ms = {k: [round(v[s] * 1e3, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {"native_ms_med_min_max": ms["native"],
            "plain_ms_med_min_max": ms["plain"],
            "speedup": round(r["plain"]["med"] / r["native"]["med"], 3),
            "max_abs_diff_native_plain": diff, "max_abs_plain": amp}


out = {"attention": {}}
for grid in args.grids:
    for heads in args.heads:
        out["attention"][f"{grid}x{grid} heads={heads} B={args.batch}"] = \
            attention_row(grid, heads)
if not args.skip_model:
    out[f"SwinIR-L {args.image}x{args.image}"] = model_row(args.image)
print(json.dumps(out, indent=1))
