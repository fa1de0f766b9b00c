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

--mlp runs the MLP section instead: per grid, ops.swin_mlp
(swin_mlp_bf16_kernel) against F.linear, F.gelu, F.linear, ops.add_layer_norm
at (C, hidden) = (180, 360) and (240, 480), with per-call time and the
compulsory bytes of either route, then SwinIR-M and SwinIR-L with Mlp.fused on
against off.

--conv runs the conv section instead: per grid, ops.conv_ragged
(conv_ragged_bf16_kernel) against the route it replaces, SDConv2d on the
library plus the add or LeakyReLU pass that conv needs, at 180 -> 180 with a
residual, 240 -> 60 with LeakyReLU, 60 -> 60 1x1 with LeakyReLU, 60 -> 240 with
a residual and 240 -> 64 with LeakyReLU; then SwinIR-M and SwinIR-L with
SwinIR.native_convs on against off.
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
ap.add_argument("--mlp", action="store_true",
                help="instead: ops.swin_mlp against the composed route per "
                     "grid at (180, 360) and (240, 480), then SwinIR-M and "
                     "SwinIR-L with Mlp.fused on against off")
ap.add_argument("--conv", action="store_true",
                help="instead: ops.conv_ragged against the library conv plus "
                     "its elementwise pass per grid and shape, then SwinIR-M "
                     "and SwinIR-L with SwinIR.native_convs on against off")
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


def mlp_row(grid, c, hidden):
    """One block's MLP half with the next norm: ops.swin_mlp against
    F.linear, F.gelu, F.linear, ops.add_layer_norm on the same tensors."""
    g = torch.Generator(device=DEV).manual_seed(grid + c)

    def n(*s, dt=torch.bfloat16):
        return torch.randn(*s, device=DEV, generator=g).to(dt)

    shape = (args.batch, grid, grid, c)
    x, res = n(*shape), 2 * n(*shape)
    w1, b1 = n(hidden, c) / c ** 0.5, 0.5 * n(hidden)
    w2, b2 = n(c, hidden) / hidden ** 0.5, 0.5 * n(c)
    gm, bt = 1 + 0.5 * n(c, dt=torch.float32), 0.5 * n(c, dt=torch.float32)
    prep = ops.swin_mlp_prepare(w1, b1, w2, b2)

    def fused():
        return ops.swin_mlp(x, res, *prep, gm, bt)

    def composed():
        h = F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)
        return ops.add_layer_norm(h, res, gm, bt)

    # both routes round the sum to bf16 once (the composed one h and fc2's
    # output as well): they agree within a few bf16 steps of the largest sum
    (s0, l0), (s1, l1) = fused(), composed()
    diff = max((s0.float() - s1.float()).abs().max().item(),
               (l0.float() - l1.float()).abs().max().item())
    amp = s1.float().abs().max().item()
    assert diff <= 2.0 ** -6 * amp, (grid, c, diff, amp)
    r = alternate({"fused": fused, "composed": composed}, args.iters)
    rows = x.numel() // c
    nbytes = 4 * rows * c * 2                      # x, res in; sum, ln out
    comp = 14 * rows * c * 2                       # the four passes, hidden 2C
    cpad, hp = prep[0].shape[1], prep[0].shape[0]
    us = {k: [round(v[s] * 1e6, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {
        "fused_us_med_min_max": us["fused"],
        "composed_us_med_min_max": us["composed"],
        "fused_compulsory_bytes": nbytes,
        "composed_compulsory_bytes": comp,
        "fused_gb_s": round(nbytes / r["fused"]["med"] / 1e9, 1),
        "composed_gb_s": round(comp / r["composed"]["med"] / 1e9, 1),
        "flop": 4 * rows * c * hidden,
        "padded_flop": 4 * rows * cpad * hp,
        "speedup": round(r["composed"]["med"] / r["fused"]["med"], 3),
        "fused_below_composed_min": r["fused"]["med"] < r["composed"]["min"],
        "max_abs_diff_fused_composed": diff,
    }


def mlp_model_row(size, *cfg):
    """The whole model with Mlp.fused on against off, alternating."""
    from sdwd_amd.models.swinir import Mlp

    torch.manual_seed(0)
    net = SwinIR(*cfg).eval().to(DEV, torch.bfloat16)
    x = torch.rand(1, 3, size, size, device=DEV, dtype=torch.bfloat16)

    def run(flag):
        def fn():
            Mlp.fused = flag
            return net(x)
        return fn

    default = Mlp.fused
    with torch.no_grad():
        a, b = run(True)().float(), run(False)().float()
        diff, amp = (a - b).abs().max().item(), b.abs().max().item()
        del a, b
        r = alternate({"fused": run(True), "composed": run(False)},
                      args.model_iters)
    Mlp.fused = default
    ms = {k: [round(v[s] * 1e3, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {"fused_ms_med_min_max": ms["fused"],
            "composed_ms_med_min_max": ms["composed"],
            "speedup": round(r["composed"]["med"] / r["fused"]["med"], 3),
            "fused_below_composed_min": r["fused"]["med"] < r["composed"]["min"],
            "max_abs_diff_fused_composed": diff, "max_abs_composed": amp}


# (Cin, Cout, ksize, LeakyReLU slope or None, residual)
CONV_SHAPES = [(180, 180, 3, None, True), (240, 60, 3, 0.2, False),
               (60, 60, 1, 0.2, False), (60, 240, 3, None, True),
               (240, 64, 3, 0.01, False)]


def conv_row(grid, cin, cout, ks, slope, with_res):
    """One conv with its epilogue: ops.conv_ragged against SDConv2d on the
    library, then what SwinIR's route without the kernel does to its output
    (.contiguous() + t on the tokens, or the LeakyReLU module)."""
    from sdwd_amd.models.layers import SDConv2d

    torch.manual_seed(grid + cin + cout)
    conv = SDConv2d(cin, cout, ks, padding=ks // 2).to(DEV, torch.bfloat16)
    act = torch.nn.LeakyReLU(slope) if slope is not None else None
    b = args.batch
    t_in = torch.randn(b, grid, grid, cin, device=DEV, dtype=torch.bfloat16)
    t_res = (torch.randn(b, grid, grid, cout, device=DEV,
                         dtype=torch.bfloat16) if with_res else None)
    x = t_in.permute(0, 3, 1, 2)
    out = torch.empty(b, cout, grid, grid, device=DEV, dtype=torch.bfloat16,
                      memory_format=torch.channels_last)
    assert ops.conv_ragged_supported(x, conv.weight, out)
    wp = ops.conv_ragged_prepare(conv.weight)
    res = None if t_res is None else t_res.permute(0, 3, 1, 2)

    def native():
        return ops.conv_ragged(x, wp, conv.bias, out, ksize=ks, lrelu=slope,
                               res=res)

    def composed():
        y = conv(x)
        if act is not None:
            y = act(y)
        if t_res is not None:
            return (y.permute(0, 2, 3, 1).contiguous() + t_res
                    ).permute(0, 3, 1, 2)
        return y

    with torch.no_grad():
        # the kernel rounds once, the composed route after the conv and again
        # after the pass: a few bf16 steps of the largest output
        y0, y1 = native().float(), composed().float()
        diff, amp = (y0 - y1).abs().max().item(), y1.abs().max().item()
        assert diff <= 2.0 ** -6 * amp, (grid, cin, cout, diff, amp)
        del y0, y1
        r = alternate({"native": native, "composed": composed}, args.iters)
    flop = 2 * b * grid * grid * cin * cout * ks * ks
    us = {k: [round(v[s] * 1e6, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {
        "native_us_med_min_max": us["native"],
        "composed_us_med_min_max": us["composed"],
        "flop": flop,
        "native_tflop_s": round(flop / r["native"]["med"] / 1e12, 1),
        "composed_tflop_s": round(flop / r["composed"]["med"] / 1e12, 1),
        "speedup": round(r["composed"]["med"] / r["native"]["med"], 3),
        "native_below_composed_min": r["native"]["med"] < r["composed"]["min"],
        "max_abs_diff_native_composed": diff,
    }


def conv_model_row(size, *cfg):
    """The whole model with SwinIR.native_convs on against off, alternating."""
    torch.manual_seed(0)
    net = SwinIR(*cfg).eval().to(DEV, torch.bfloat16)
    x = torch.rand(1, 3, size, size, device=DEV, dtype=torch.bfloat16)

    def run(flag):
        def fn():
            net.native_convs = flag
            return net(x)
        return fn

    with torch.no_grad():
        a, b = run(True)().float(), run(False)().float()
        diff, amp = (a - b).abs().max().item(), b.abs().max().item()
        del a, b
        r = alternate({"native": run(True), "library": run(False)},
                      args.model_iters)
    ms = {k: [round(v[s] * 1e3, 2) for s in ("med", "min", "max")]
          for k, v in r.items()}
    return {"native_convs_ms_med_min_max": ms["native"],
            "library_convs_ms_med_min_max": ms["library"],
            "speedup": round(r["library"]["med"] / r["native"]["med"], 3),
            "native_below_library_min": r["native"]["med"] < r["library"]["min"],
            "max_abs_diff_native_library": diff, "max_abs_library": amp}


if args.conv:
    out = {"conv": {}}
    for grid in args.grids:
        for cin, cout, ks, slope, with_res in CONV_SHAPES:
            key = (f"{grid}x{grid} {cin}->{cout} ks={ks} lrelu={slope} "
                   f"res={with_res} B={args.batch}")
            out["conv"][key] = conv_row(grid, cin, cout, ks, slope, with_res)
    if not args.skip_model:
        size = args.image
        out[f"SwinIR-M {size}x{size}"] = conv_model_row(
            size, 180, (6,) * 6, 6, 2.0, "1conv")
        out[f"SwinIR-L {size}x{size}"] = conv_model_row(
            size, 240, (6,) * 9, 8, 2.0, "3conv")
    print(json.dumps(out, indent=1))
    sys.exit(0)

if args.mlp:
    out = {"mlp": {}}
    for grid in args.grids:
        for c, hidden in ((180, 360), (240, 480)):
            out["mlp"][f"{grid}x{grid} C={c} hidden={hidden} B={args.batch}"] = \
                mlp_row(grid, c, hidden)
    if not args.skip_model:
        size = args.image
        out[f"SwinIR-M {size}x{size}"] = mlp_model_row(
            size, 180, (6,) * 6, 6, 2.0, "1conv")
        out[f"SwinIR-L {size}x{size}"] = mlp_model_row(
            size, 240, (6,) * 9, 8, 2.0, "3conv")
    print(json.dumps(out, indent=1))
    sys.exit(0)

out = {"attention": {}}
for grid in args.grids:
    for heads in args.heads:
        out["attention"][f"{grid}x{grid} heads={heads} B={args.batch}"] = \
            attention_row(grid, heads)
if not args.skip_model:
    out[f"SwinIR-L {args.image}x{args.image}"] = model_row(args.image)
print(json.dumps(out, indent=1))
