#!/usr/bin/env python3
"""HAT attention and the whole 4x model: ops.attention_hat
(hat_attn_bf16_kernel, kw 16 with shift 8 and kw 24) against its native=False
torch route (roll, partition, mask or unfold, score tensor, softmax, reverse;
what HAT.forward(native=False) runs), alternating in one process.

Per token grid (256x256 and 512x512 by default) at 6 heads: one block's
attention on the [B, H, W, 3, heads, 32] view of a QKV GEMM output. GB/s is on
the kernel's compulsory traffic (qkv in, the output out, the offsets once),
TFLOP/s on 4 * queries * keys * 32 a head; the two routes' outputs are
compared at every timed size before timing. Then HAT (embed 180, 6 x 6
blocks) on a --image x --image input. Each figure is the median of --rounds
alternating rounds. One JSON object on stdout.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sdwd_amd import ops
from sdwd_amd.models.hat import HAT

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
ap.add_argument("--heads", type=int, default=6)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--image", type=int, default=256)
ap.add_argument("--model-iters", type=int, default=2)
ap.add_argument("--limit", type=float, default=10.0,
                help="seconds a single timing step may take")
ap.add_argument("--skip-model", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "hat_perf needs a GPU"
DEV = "cuda"


def step(fn, warm, it):
    """Mean seconds per call: `it` calls enqueued, one synchronise per 10."""
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


def attention_row(grid, kw, shift):
    heads = args.heads
    g = torch.Generator(device=DEV).manual_seed(grid + kw)
    qkv = torch.randn(1, grid, grid, 3, heads, 32, device=DEV, generator=g,
                      dtype=torch.bfloat16)
    off = torch.randn(heads, kw + 15, kw + 15, device=DEV, generator=g)
    scale = 30 ** -0.5

    def native():
        return ops.attention_hat(qkv, off, scale, shift, kw)

    def plain():
        return ops.attention_hat(qkv, off, scale, shift, kw, native=False)

    # the kernel is within 3 * 2^-8 * max|v| of the exact result (the tests'
    # bound, p @ |v| <= max|v|), the fp32 torch route within one bf16 rounding
    diff = (native().float() - plain().float()).abs().max().item()
    vmax = qkv[:, :, :, 2].float().abs().max().item()
    assert diff <= 2.0 ** -6 * vmax, (grid, kw, diff, vmax)
    r = alternate({"native": native, "torch": plain}, args.iters)
    nbytes = qkv.numel() * 2 + qkv.numel() // 3 * 2 + off.numel() * 4
    flop = 4 * grid * grid * kw * kw * 32 * heads
    us = {k: [round(v[s] * 1e6, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {
        "native_us_med_min_max": us["native"],
        "torch_us_med_min_max": us["torch"],
        "native_gb_s": round(nbytes / r["native"]["med"] / 1e9, 1),
        "native_tflop_s": round(flop / r["native"]["med"] / 1e12, 1),
        "compulsory_bytes": nbytes,
        "flop": flop,
        "speedup": round(r["torch"]["med"] / r["native"]["med"], 2),
        "max_abs_diff_native_torch": diff,
        "diff_limit": 2.0 ** -6 * vmax,
    }


def model_row(size):
    torch.manual_seed(0)
    net = HAT(180, (6,) * 6, 6).eval().to(DEV, torch.bfloat16)
    x = torch.rand(1, 3, size, size, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        a, b = net(x).float(), net(x, native=False).float()
        diff, amp = (a - b).abs().max().item(), b.abs().max().item()
        del a, b
        r = alternate({"native": lambda: net(x),
                       "plain": lambda: net(x, native=False)},
                      args.model_iters)
    ms = {k: [round(v[s] * 1e3, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {"native_ms_med_min_max": ms["native"],
            "plain_ms_med_min_max": ms["plain"],
            "speedup": round(r["plain"]["med"] / r["native"]["med"], 3),
            "max_abs_diff_native_plain": diff, "max_abs_plain": amp}


out = {"attention": {}}
for grid in args.grids:
    for kw, shift in ((16, 8), (24, 0)):
        out["attention"][f"{grid}x{grid} kw={kw} shift={shift} "
                         f"heads={args.heads}"] = attention_row(grid, kw, shift)
if not args.skip_model:
    out[f"HAT {args.image}x{args.image}"] = model_row(args.image)
print(json.dumps(out, indent=1))
