#!/usr/bin/env python3
"""ESRGAN trunk convs and the whole 4x RRDBNet: ops.conv3x3_dense (native)
against the composed route (torch.cat + F.conv2d + leaky_relu, what
RRDBNet.forward(native=False) runs), alternating in one process.

Per input size (512x512 and 1024x1024 by default): the five dense-block conv
shapes (Cin 64..192 -> 32 with LeakyReLU, 192 -> 64 with the residual), then
the 23-block model. Each figure is the median of --rounds alternating rounds;
TF/s is on the FLOPs each route executes. A step that exceeds --limit seconds
stops iterating early (its mean is over the calls it completed).
One JSON object on stdout.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from sdwd_amd import ops
from sdwd_amd.models.esrgan import RRDBNet

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--model-iters", type=int, default=2)
ap.add_argument("--nb", type=int, default=23)
ap.add_argument("--limit", type=float, default=20.0,
                help="seconds a single timing step may take")
ap.add_argument("--skip-model", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "esrgan_perf needs a GPU"
DEV = "cuda"
NF, GC = 64, 32


def step(fn, warm, it):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < it:
        fn()
        torch.cuda.synchronize()
        done += 1
        if time.perf_counter() - t0 > args.limit:
            break
    return (time.perf_counter() - t0) / done


def alternate(runs, it):
    ts = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ts[k].append(step(fn, 1, it))
    out = {}
    for k, v in ts.items():
        v = sorted(v)
        out[k] = {"med": v[len(v) // 2], "min": v[0], "max": v[-1]}
    return out


def conv_rows(size):
    g = torch.Generator(device=DEV).manual_seed(size)
    ws = torch.randn(1, NF + 4 * GC, size, size, device=DEV, generator=g,
                     dtype=torch.bfloat16)
    ws = ws.contiguous(memory_format=torch.channels_last)
    dst = torch.empty_like(ws)
    rows = {}
    for j in range(5):
        cin = NF + j * GC
        cout = GC if j < 4 else NF
        w = (torch.randn(cout, cin, 3, 3, device=DEV, generator=g) * 0.02
             ).bfloat16()
        wcl = w.contiguous(memory_format=torch.channels_last)
        wp = w.permute(0, 2, 3, 1).contiguous()
        b = torch.randn(cout, device=DEV, generator=g).bfloat16()
        parts = [ws[:, :NF]] + [ws[:, NF + k * GC:NF + (k + 1) * GC]
                                for k in range(j)]
        if j < 4:
            def native(cin=cin, wp=wp, b=b):
                ops.conv3x3_dense(ws[:, :cin], wp, b, ws[:, cin:cin + GC],
                                  lrelu=0.2)

            def composed(parts=parts, wcl=wcl, b=b):
                return F.leaky_relu(
                    F.conv2d(torch.cat(parts, 1), wcl, b, padding=1), 0.2)
        else:
            def native(wp=wp, b=b):
                ops.conv3x3_dense(ws, wp, b, dst[:, :NF], alpha=0.2,
                                  res2=ws[:, :NF])

            def composed(parts=parts, wcl=wcl, b=b):
                return F.conv2d(torch.cat(parts, 1), wcl, b,
                                padding=1) * 0.2 + parts[0]
        r = alternate({"native": native, "composed": composed}, args.iters)
        flops = 2 * size * size * 9 * cin * cout
        rows[f"{cin}->{cout}"] = {
            "native_ms": round(r["native"]["med"] * 1e3, 3),
            "native_min_max_ms": [round(r["native"]["min"] * 1e3, 3),
                                  round(r["native"]["max"] * 1e3, 3)],
            "native_tf": round(flops / r["native"]["med"] / 1e12, 1),
            "composed_ms": round(r["composed"]["med"] * 1e3, 3),
            "composed_min_max_ms": [round(r["composed"]["min"] * 1e3, 3),
                                    round(r["composed"]["max"] * 1e3, 3)],
            "composed_tf": round(flops / r["composed"]["med"] / 1e12, 1),
            "speedup": round(r["composed"]["med"] / r["native"]["med"], 3),
        }
    return rows


def model_flops(size, nb, fold):
    px = size * size
    trunk = sum(9 * (NF + j * GC) * (GC if j < 4 else NF) for j in range(5))
    up_taps = 4 if fold else 9     # the folded upsample executes 4 taps
    macs = px * (9 * 3 * NF + nb * 3 * trunk + 9 * NF * NF)
    macs += 4 * px * up_taps * NF * NF + 16 * px * up_taps * NF * NF
    macs += 16 * px * (9 * NF * NF + 9 * NF * 3)
    return 2 * macs


def model_row(size):
    torch.manual_seed(0)
    net = RRDBNet(NF, GC, args.nb).eval().to(DEV, torch.bfloat16)
    x = torch.rand(1, 3, size, size, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        r = alternate({
            "native": lambda: net(x),
            "composed": lambda: net(x, native=False),
        }, args.model_iters)
    fn, fc = model_flops(size, args.nb, True), model_flops(size, args.nb, False)
    return {
        "native_ms": round(r["native"]["med"] * 1e3, 2),
        "native_min_max_ms": [round(r["native"]["min"] * 1e3, 2),
                              round(r["native"]["max"] * 1e3, 2)],
        "native_tf": round(fn / r["native"]["med"] / 1e12, 1),
        "composed_ms": round(r["composed"]["med"] * 1e3, 2),
        "composed_min_max_ms": [round(r["composed"]["min"] * 1e3, 2),
                                round(r["composed"]["max"] * 1e3, 2)],
        "composed_tf": round(fc / r["composed"]["med"] / 1e12, 1),
        "speedup": round(r["composed"]["med"] / r["native"]["med"], 3),
    }


out = {}
for size in args.sizes:
    out[f"{size}x{size}"] = {"convs": conv_rows(size)}
    if not args.skip_model:
        out[f"{size}x{size}"]["model"] = model_row(size)
print(json.dumps(out, indent=1))
