#!/usr/bin/env python3
"""Our conv3x3 vs MIOpen F.conv2d on the SD hot shapes (channels_last).

--wrap adds, per shape, the wrapped (seamless-tiling) native time next to
the plain native time, and the time of the library route a tiled conv took
before the kernels could wrap: F.pad(mode="circular") + F.conv2d.

--ups times only the six fused upsample convs of the headline workload:
the folded 2x2 sub-pixel kernel against the 9-tap kernel, alternating in
one process, in ms and in TF/s on the FLOPs each kernel executes.

--extras times each shape the three ways the UNet calls it (plain, with the
residual, with the time-embedding bias and the GroupNorm partials), at Cin
and 2 Cin, and fits time = a * K tiles + b. --dump DIR writes the outputs
and partials of seeded inputs, to compare two builds bit for bit.
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

SHAPES = [
    (128, 320, 64, 64, 320, 1),
    (128, 640, 32, 32, 640, 1),
    (128, 1280, 16, 16, 1280, 1),
    (128, 1280, 8, 8, 1280, 1),
    (128, 2560, 8, 8, 1280, 1),
    (128, 1920, 16, 16, 1280, 1),
    (128, 960, 32, 32, 640, 1),
    (128, 640, 64, 64, 320, 1),
    (128, 320, 64, 64, 320, 2),
    (16, 512, 64, 64, 512, 1),    # VAE mid
    (16, 512, 128, 128, 512, 1),
    (16, 256, 256, 256, 256, 1),
    (16, 128, 512, 512, 128, 1),
]


ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--wrap", action="store_true",
                help="also time wrap=(True, True) and F.pad(circular)+conv2d")
ap.add_argument("--ups", action="store_true",
                help="only the fused upsample convs: folded 2x2 sub-pixel "
                     "kernel vs the 9-tap kernel, alternating in this process")
ap.add_argument("--rounds", type=int, default=7,
                help="--ups / --extras: alternating rounds per shape")
ap.add_argument("--extras", action="store_true",
                help="each of SHAPES plain, with residual, and with channel "
                     "bias + collect_gn, at Cin and 2 Cin, with the "
                     "time = a * K tiles + b fit")
ap.add_argument("--dump", metavar="DIR",
                help="write outputs and GroupNorm partials of seeded inputs "
                     "(every SHAPES row and mode, every upsample conv) as "
                     ".npy into DIR")
args = ap.parse_args()


def t(fn, warm=2, it=6):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(it):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / it


# (N, Cin, H, W, Cout) of the source image: the three UNet Upsample convs at
# batch 64 (cond + uncond rows) and the three VAE-decoder ones
UPS_SHAPES = [
    (128, 1280, 8, 8, 1280),
    (128, 1280, 16, 16, 1280),
    (128, 640, 32, 32, 640),
    (16, 512, 64, 64, 512),
    (16, 512, 128, 128, 512),
    (16, 256, 256, 256, 256),
]


def ups_perf():
    """Per shape: `rounds` alternating (folded, 9-tap) timings, each of 20
    calls after 2 warm-up calls. Reports the median, the spread (min..max
    over the rounds) and the rate on EXECUTED FLOPs: 4 taps x Cin per
    output for the folded kernel, 9 for the other."""
    res = {}
    for (N, Ci, H, W, Co) in UPS_SHAPES:
        x = torch.randn(N, Ci, H, W, device="cuda", dtype=torch.bfloat16)
        xc = x.contiguous(memory_format=torch.channels_last)
        w = torch.randn(Co, Ci, 3, 3, device="cuda",
                        dtype=torch.bfloat16) * 0.02
        b = torch.randn(Co, device="cuda", dtype=torch.bfloat16)
        wp = w.permute(0, 2, 3, 1).contiguous()
        wf = ops.fold_ups2x_weight(wp)
        runs = {
            "fold": lambda: ops.ups2x_conv3x3(xc, wp, b, collect_gn=True,
                                              w_fold=wf),
            "tap9": lambda: ops.ups2x_conv3x3(xc, wp, b, collect_gn=True,
                                              fold=False),
        }
        taps = {"fold": 4, "tap9": 9}
        ts = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                ts[k].append(t(fn, warm=2, it=20))
        row = {}
        for k, v in ts.items():
            v = sorted(v)
            med = v[len(v) // 2]
            flops = 2 * N * Co * Ci * taps[k] * 4 * H * W
            row.update({
                f"{k}_ms": round(med * 1e3, 3),
                f"{k}_min_ms": round(v[0] * 1e3, 3),
                f"{k}_max_ms": round(v[-1] * 1e3, 3),
                f"{k}_tf": round(flops / med / 1e12, 1),
            })
        row["speedup"] = round(row["tap9_ms"] / row["fold_ms"], 3)
        # a gain only if the slowest folded round beats the fastest 9-tap
        row["clear"] = row["fold_max_ms"] < row["tap9_min_ms"]
        res[f"{N}x{Ci}x{H}x{W}->{Co}/ups2x"] = row
    print(json.dumps(res, indent=1))


def extras_inputs(N, Ci, H, W, Co, s, seed):
    """Seeded operands of one SHAPES row as the UNet passes them: bf16
    bias, channels_last residual, bf16 [N, Cout] time-embedding bias."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    x = rnd(N, Ci, H, W).bfloat16()
    xc = x.contiguous(memory_format=torch.channels_last)
    w = (rnd(Co, Ci, 3, 3) * 0.02).bfloat16()
    wp = w.permute(0, 2, 3, 1).contiguous()
    b = rnd(Co).bfloat16()
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    res = rnd(N, Co, Ho, Wo).bfloat16().contiguous(
        memory_format=torch.channels_last)
    cb = rnd(N, Co).bfloat16()
    return xc, wp, b, res, cb


def extras_modes(xc, wp, b, res, cb, s):
    """plain: conv + bias (+ partials for the next GroupNorm); res: the
    ResBlock's conv2 with its skip; cb: conv1 with the time embedding."""
    return {
        "plain": lambda: ops.conv3x3(xc, wp, b, None, s),
        "res": lambda: ops.conv3x3(xc, wp, b, res, s),
        "cb": lambda: ops.conv3x3(xc, wp, b, None, s, chan_bias=cb,
                                  collect_gn=True),
    }


def extras_perf():
    """Per SHAPES row and mode: `rounds` timings (20 calls after 2 warm-up
    calls each, modes alternating) at Cin and at 2 Cin, and the r07 fit
    time = a * K tiles + b from the two medians (K tiles = 9 Cin / 64).
    One JSON object; compare two builds by running this once per build in
    alternating processes."""
    res_all = {}
    for (N, Ci, H, W, Co, s) in SHAPES:
        row = {}
        for mult in (1, 2):
            ops_in = extras_inputs(N, Ci * mult, H, W, Co, s, 11)
            modes = extras_modes(*ops_in, s)
            ts = {k: [] for k in modes}
            for _ in range(args.rounds):
                for k, fn in modes.items():
                    ts[k].append(t(fn, warm=2, it=20))
            for k, v in ts.items():
                v = sorted(v)
                row.setdefault(k, {})[f"ms_x{mult}"] = {
                    "med": round(v[len(v) // 2] * 1e3, 4),
                    "min": round(v[0] * 1e3, 4),
                    "max": round(v[-1] * 1e3, 4),
                }
            del ops_in, modes
        for k, d in row.items():
            k1 = 9 * Ci // 64
            t1, t2 = d["ms_x1"]["med"], d["ms_x2"]["med"]
            a = (t2 - t1) / k1
            d["a_ms_per_ktile"] = round(a, 5)
            d["b_fixed_ms"] = round(t1 - a * k1, 4)
        res_all[f"{N}x{Ci}x{H}x{W}->{Co}/s{s}"] = row
    print(json.dumps(res_all))


def extras_dump(out_dir):
    """Outputs and GroupNorm partials of seeded inputs as .npy (bf16 as its
    int16 bit pattern), per SHAPES row, mode and upsample shape: two builds
    compute the same iff the files are byte-equal. conv3x3_plan depends on
    the row count, so each conv is dumped twice: whole at a small batch
    (which the plan sends to the v2 kernel, mostly at BN = 64), and at the
    timed batch, the kernels the timings run (v4, v2 at BN = 128), as every
    1021st element of y plus all partials."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)

    def save(name, y, step=1):
        flat = y.permute(0, 2, 3, 1).reshape(-1).view(torch.int16)
        np.save(os.path.join(out_dir, name + "_y.npy"),
                flat[::step].cpu().numpy())
        gnp = getattr(y, "_sdwd_gnp", None)
        if gnp is not None:
            np.save(os.path.join(out_dir, name + "_gnp.npy"),
                    gnp[0].cpu().numpy())

    def all_modes(name, ops_in, s, step):
        for k, fn in extras_modes(*ops_in, s).items():
            save(f"{name}_{k}", fn(), step)
        xc, wp, b, res, cb = ops_in
        save(f"{name}_all", ops.conv3x3(xc, wp, b, res, s, chan_bias=cb,
                                        collect_gn=True), step)

    for i, (N, Ci, H, W, Co, s) in enumerate(SHAPES):
        n = max(1, min(N, 4, 65536 // (H * W)))
        all_modes(f"conv{i}_n{n}", extras_inputs(n, Ci, H, W, Co, s, 100 + i),
                  s, 1)
        all_modes(f"conv{i}_n{N}", extras_inputs(N, Ci, H, W, Co, s, 300 + i),
                  s, 1021)
    for i, (N, Ci, H, W, Co) in enumerate(UPS_SHAPES):
        n = max(1, min(N, 2, 16384 // (H * W)))
        xc, wp, b, _, _ = extras_inputs(n, Ci, H, W, Co, 1, 200 + i)
        save(f"ups{i}_fold", ops.ups2x_conv3x3(xc, wp, b, collect_gn=True))
        save(f"ups{i}_tap9", ops.ups2x_conv3x3(xc, wp, b, collect_gn=True,
                                               fold=False))
    torch.cuda.synchronize()
    print(json.dumps({"dumped": len(os.listdir(out_dir)), "dir": out_dir}))


if args.ups:
    ups_perf()
    sys.exit(0)
if args.dump:
    extras_dump(args.dump)
    sys.exit(0)
if args.extras:
    extras_perf()
    sys.exit(0)

out = {}
tot_ours = tot_miopen = tot_wrap = tot_padlib = 0.0
for (N, Ci, H, W, Co, s) in SHAPES:
    x = torch.randn(N, Ci, H, W, device="cuda", dtype=torch.bfloat16)
    xc = x.contiguous(memory_format=torch.channels_last)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", dtype=torch.bfloat16) * 0.02
    b = torch.randn(Co, device="cuda", dtype=torch.bfloat16)
    wp = w.permute(0, 2, 3, 1).contiguous()
    wcl = w.contiguous(memory_format=torch.channels_last)
    t_ours = t(lambda: ops.conv3x3(xc, wp, b, None, s))
    t_mi = t(lambda: F.conv2d(xc, wcl, b, stride=s, padding=1))
    flops = 2 * N * Co * Ci * 9 * (H // s) * (W // s)
    key = f"{N}x{Ci}x{H}x{W}->{Co}/s{s}"
    out[key] = {
        "ours_ms": round(t_ours * 1e3, 3),
        "ours_tf": round(flops / t_ours / 1e12, 1),
        "miopen_ms": round(t_mi * 1e3, 3),
        "miopen_tf": round(flops / t_mi / 1e12, 1),
    }
    tot_ours += t_ours
    tot_miopen += t_mi
    if args.wrap:
        t_wrap = t(lambda: ops.conv3x3(xc, wp, b, None, s,
                                       wrap=(True, True)))
        t_pad = t(lambda: F.conv2d(F.pad(xc, (1, 1, 1, 1), mode="circular"),
                                   wcl, b, stride=s))
        out[key].update({
            "wrap_ms": round(t_wrap * 1e3, 3),
            "wrap_tf": round(flops / t_wrap / 1e12, 1),
            "wrap_vs_plain": round(t_wrap / t_ours, 3),
            "padlib_ms": round(t_pad * 1e3, 3),
            "padlib_tf": round(flops / t_pad / 1e12, 1),
        })
        tot_wrap += t_wrap
        tot_padlib += t_pad
out["_total"] = {"ours_ms": round(tot_ours * 1e3, 2),
                 "miopen_ms": round(tot_miopen * 1e3, 2)}
if args.wrap:
    out["_total"].update({"wrap_ms": round(tot_wrap * 1e3, 2),
                          "padlib_ms": round(tot_padlib * 1e3, 2)})
print(json.dumps(out, indent=1))
