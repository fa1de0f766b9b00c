#!/usr/bin/env python3
"""SCUNet's attention half and the whole model: ops.window_attn_block
(window_block_attn_bf16_kernel) against the composed five-launch route
(ops.layer_norm, the QKV GEMM, ops.attention_swin, the proj GEMM,
ops.add_layer_norm: what SCUNet runs with fused_attention off), alternating
in one process.

Per branch width (32, 64) and token grid (512x512, 1024x1024 by default), on
the trans half of a [1, H, W, 2C] NHWC buffer as the model passes it. GB/s is
on the kernel's compulsory traffic (x in, y and n2 out), TFLOP/s on
2 * (4 C^2 + 2 * 64 * C) FLOP a token (QKV and proj, QK^T and PV); the two
routes' outputs are compared at every timed size before timing. Then SCUNet
(config [4]*7, dim 64) on an --image x --image input with the fused kernel
on, off, and native=False. Each figure is the median of --rounds alternating
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
from sdwd_amd.models.scunet import Block, SCUNet

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--grids", type=int, nargs="+", default=[512, 1024])
ap.add_argument("--widths", type=int, nargs="+", default=[32, 64])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--image", type=int, default=512)
ap.add_argument("--model-iters", type=int, default=3)
ap.add_argument("--limit", type=float, default=10.0,
                help="seconds a single timing step may take")
ap.add_argument("--skip-model", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "scunet_perf needs a GPU"
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


def attention_row(c, grid, shift):
    torch.manual_seed(c + grid)
    blk = Block(c, shift).eval()
    with torch.no_grad():
        for p in blk.parameters():
            p.normal_(std=c ** -0.5)
        blk.ln1.weight.add_(1.0)
        blk.ln2.weight.add_(1.0)
    blk = blk.to(DEV, torch.bfloat16)
    buf = torch.randn(1, grid, grid, 2 * c, device=DEV, dtype=torch.bfloat16)
    x = buf[..., c:]

    def fused():
        return blk.attention_native(x, True)

    def composed():
        return blk.attention_native(x, False)

    with torch.no_grad():
        a, b = fused(), composed()
        # both routes are bf16 roundings of the same fp32 math at different
        # points; the kernel tests bound each against fp64
        diff = max((p.float() - q.float()).abs().max().item()
                   for p, q in zip(a, b))
        amp = max(q.float().abs().max().item() for q in b)
        assert diff <= 2.0 ** -5 * (1 + amp), (c, grid, diff, amp)
        del a, b
        r = alternate({"fused": fused, "composed": composed}, args.iters)
    tokens = grid * grid
    nbytes = tokens * c * 2 * 3
    flop = 2 * tokens * (4 * c * c + 2 * 64 * c)
    us = {k: [round(v[s] * 1e6, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    walk, blocks = ops.ext().window_block_attn_plan(tokens // 64, c)
    return {
        "fused_us_med_min_max": us["fused"],
        "composed_us_med_min_max": us["composed"],
        "fused_gb_s": round(nbytes / r["fused"]["med"] / 1e9, 1),
        "fused_tflop_s": round(flop / r["fused"]["med"] / 1e12, 2),
        "compulsory_bytes": nbytes,
        "flop": flop,
        "walk_blocks": [walk, blocks],
        "speedup": round(r["composed"]["med"] / r["fused"]["med"], 2),
        "max_abs_diff_fused_composed": diff,
        "max_abs_composed": amp,
    }


def model_row(size):
    torch.manual_seed(0)
    net = SCUNet().eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                p.normal_(std=p[0].numel() ** -0.5)
    net = net.to(DEV, torch.bfloat16)
    x = torch.rand(1, 3, size, size, device=DEV, dtype=torch.bfloat16)

    def fused():
        net.fused_attention = True
        return net(x)

    def composed():
        net.fused_attention = False
        return net(x)

    with torch.no_grad():
        a, b = fused().float(), net(x, native=False).float()
        diff, amp = (a - b).abs().max().item(), b.abs().max().item()
        del a, b
        r = alternate({"fused": fused, "composed": composed,
                       "plain": lambda: net(x, native=False)},
                      args.model_iters)
    ms = {k: [round(v[s] * 1e3, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {"fused_ms_med_min_max": ms["fused"],
            "composed_ms_med_min_max": ms["composed"],
            "plain_ms_med_min_max": ms["plain"],
            "fused_over_composed": round(
                r["composed"]["med"] / r["fused"]["med"], 3),
            "fused_over_plain": round(r["plain"]["med"] / r["fused"]["med"],
                                      3),
            "max_abs_diff_fused_plain": diff, "max_abs_plain": amp}


out = {"attention_half": {}}
for c in args.widths:
    for grid in args.grids:
        out["attention_half"][f"c={c} {grid}x{grid} shift=4"] = \
            attention_row(c, grid, 4)
if not args.skip_model:
    out[f"SCUNet {args.image}x{args.image}"] = model_row(args.image)
print(json.dumps(out, indent=1))
