#!/usr/bin/env python3
"""The elementwise tail of a HAT block: ops.channel_gate +
ops.gated_add_layer_norm (hab_tail.hip: pool, gate, row kernel) against the
composed torch route HAT runs with fused_tail off (ChannelAttention.forward,
the two adds, the scale, norm2), alternating in one process on the same
tensors.

Per token grid (256x256 and 512x512 by default) at C = 180, B = 1: time per
tail, and the fused route's GB/s over its six compulsory passes (c for the
mean; x, attn, c in; sum and norm out). Then HAT (embed 180, 6 x 6 blocks) on
an --image x --image input with HAT.fused_tail on and off, and SwinIR (embed
180, 6 x 6 blocks) with ops.add_layer_norm as it is against the composed
route it took at embed 180 before (fp32 add, one rounding, ops.layer_norm).
Each figure is the median [min, max] of --rounds alternating rounds. One JSON
object on stdout.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sdwd_amd import ops
from sdwd_amd.models import swinir as swinir_mod
from sdwd_amd.models.hat import CONV_SCALE, HAB, HAT, _nchw, _tokens
from sdwd_amd.models.layers import _fp32_cached
from sdwd_amd.models.swinir import SwinIR

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
ap.add_argument("--width", type=int, default=180)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--image", type=int, default=256)
ap.add_argument("--model-iters", type=int, default=2)
ap.add_argument("--limit", type=float, default=10.0,
                help="seconds a single timing step may take")
ap.add_argument("--skip-models", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "hab_tail_perf needs a GPU"
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


def tail_row(grid):
    c_ = args.width
    torch.manual_seed(grid)
    blk = HAB(c_, 6, 2 * c_, 0, 3, 30).eval().to(DEV, torch.bfloat16)
    for p in blk.parameters():
        torch.nn.init.normal_(p, std=0.1)
    ca, norm2 = blk.conv_block.cab[3], blk.norm2
    t, attn, c = (torch.randn(1, grid, grid, c_, device=DEV,
                              dtype=torch.bfloat16) for _ in range(3))
    cn = _nchw(c)           # what the CAB's second conv hands over

    def fused():
        gate = ops.channel_gate(_tokens(cn), *ca.prepared(), scale=CONV_SCALE)
        return ops.gated_add_layer_norm(t, attn, _tokens(cn), gate,
                                        *_fp32_cached(norm2), norm2.eps)

    def composed():
        s = t + attn + CONV_SCALE * _tokens(ca(cn))
        return s, norm2(s)

    with torch.no_grad():
        assert ops.hab_tail_supported(t, attn, _tokens(cn))
        (fs, fn), (cs, cn_) = fused(), composed()
        # the composed route rounds to bf16 four times on the way to s
        d_sum = (fs.float() - cs.float()).abs().max().item()
        d_ln = (fn.float() - cn_.float()).abs().max().item()
        amp = cs.float().abs().max().item()
        assert d_sum <= 2.0 ** -6 * amp, (grid, d_sum, amp)
        del fs, fn, cs, cn_
        r = alternate({"fused": fused, "composed": composed}, args.iters)
    nbytes = 6 * t.numel() * 2
    us = {k: [round(v[s] * 1e6, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {
        "fused_us_med_min_max": us["fused"],
        "composed_us_med_min_max": us["composed"],
        "fused_gb_s_over_6_passes": round(nbytes / r["fused"]["med"] / 1e9, 1),
        "compulsory_bytes": nbytes,
        "speedup": round(r["composed"]["med"] / r["fused"]["med"], 2),
        "composed_min_above_fused_max":
            r["composed"]["min"] > r["fused"]["max"],
        "max_abs_diff_sum": d_sum, "max_abs_diff_ln": d_ln,
        "max_abs_sum": amp,
    }


def model_row(net, x, routes):
    """routes: name -> a callable that sets the route; alternating."""
    def run(select):
        def fn():
            select()
            return net(x)
        return fn

    names = list(routes)
    with torch.no_grad():
        a, b = (run(routes[k])().float() for k in names)
        diff, amp = (a - b).abs().max().item(), b.abs().max().item()
        del a, b
        r = alternate({k: run(routes[k]) for k in names}, args.model_iters)
    routes[names[0]]()
    out = {f"{k}_ms_med_min_max": [round(v[s] * 1e3, 2)
                                   for s in ("med", "min", "max")]
           for k, v in r.items()}
    out["speedup"] = round(r[names[1]]["med"] / r[names[0]]["med"], 3)
    out["max_abs_diff"], out["max_abs"] = diff, amp
    return out


def composed_add_layer_norm(x, res, weight, bias, eps=1e-5, gather=None):
    """What ops.add_layer_norm ran at a width that is no multiple of 8."""
    s = (x.float() + res.float()).to(x.dtype)
    return s, ops.layer_norm(s, weight, bias, eps)


class _SwinOps:
    """sdwd_amd.ops with another add_layer_norm, for models/swinir.py."""

    def __init__(self, add_layer_norm):
        self.add_layer_norm = add_layer_norm

    def __getattr__(self, name):
        return getattr(ops, name)


out = {"tail": {}}
for grid in args.grids:
    out["tail"][f"{grid}x{grid} C={args.width}"] = tail_row(grid)
if not args.skip_models:
    size = args.image
    x = torch.rand(1, 3, size, size, device=DEV, dtype=torch.bfloat16)
    torch.manual_seed(0)
    hat = HAT(180, (6,) * 6, 6).eval().to(DEV, torch.bfloat16)

    def hat_route(flag):
        return lambda: setattr(HAT, "fused_tail", flag)

    out[f"HAT {size}x{size}"] = model_row(
        hat, x, {"fused_tail": hat_route(True), "composed": hat_route(False)})
    del hat
    torch.manual_seed(0)
    swin = SwinIR(180, (6,) * 6, 6, 2.0, "1conv").eval().to(DEV,
                                                             torch.bfloat16)

    def swin_route(fn):
        return lambda: setattr(swinir_mod, "ops", _SwinOps(fn))

    out[f"SwinIR {size}x{size}"] = model_row(
        swin, x, {"kernel": swin_route(ops.add_layer_norm),
                  "composed": swin_route(composed_add_layer_norm)})
    swinir_mod.ops = ops
print(json.dumps(out, indent=1))
