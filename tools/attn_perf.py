#!/usr/bin/env python3
"""Attention kernel microbench at the SD UNet shapes.

Reports per-shape ms and TF/s (useful FLOPs, true head dim D, not the
padded kernel extent) for the in-tree flash kernel. --check compares
against a fp32 eager reference first. Shapes follow the batch-64
CFG-doubled 512x512 SD1.5 step (B=128) plus SDXL/cross-attn variants.

--window times Hypertile's windowed self-attention at the shapes that occur
(WINDOW_SHAPES), each on strided q/k/v views of one fused QKV tensor, five
ways: (1) the windowed kernel, (2) the plain kernel on pre-rearranged
contiguous window copies, copies excluded, (3) the same with the copies of
q, k, v and the output included, (4) the plain full-sequence call, (5) token
merging at ratio 0.5 at the same shape (match, plan, merge, attention on the
merged length), for orientation. The variants alternate inside each of
--rounds rounds; the report is the median round and the min..max band.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sdwd_amd import ops  # noqa: E402

# (tag, B, H, Sq, Sk, D)
SHAPES = [
    ("sd15-self-320", 128, 8, 4096, 4096, 40),
    ("sd15-self-640", 128, 8, 1024, 1024, 80),
    ("sd15-self-1280", 128, 8, 256, 256, 160),
    ("sd15-cross-320", 128, 8, 4096, 77, 40),
    ("sd15-cross-640", 128, 8, 1024, 77, 80),
    ("sdxl-self-640", 64, 10, 4096, 4096, 64),
    ("sdxl-self-1280", 64, 20, 1024, 1024, 64),
]


def flops(B, H, Sq, Sk, D):
    return 2 * B * H * Sq * Sk * D * 2  # QK^T + PV


# (tag, grid, window, heads, D): the level-0 self-attention of 512x512 at
# SD1.x (D=40) and SDXL-like D=64, of the 1024x1024 hires pass, of 768x512
WINDOW_SHAPES = [
    ("512x512-d40", (64, 64), (32, 32), 8, 40),
    ("512x512-d64", (64, 64), (32, 32), 5, 64),
    ("1024x1024-d40", (128, 128), (32, 32), 8, 40),
    ("768x512-d40", (64, 96), (32, 32), 8, 40),
]


def _band(times):
    ts = sorted(times)
    return {"median_ms": round(ts[len(ts) // 2] * 1e3, 3),
            "min_ms": round(ts[0] * 1e3, 3), "max_ms": round(ts[-1] * 1e3, 3)}


def window_main(args):
    """The five routes of --window; prints one JSON line per shape."""
    B = args.batch
    out = {}
    for tag, grid, window, H, D in WINDOW_SHAPES:
        if args.only and args.only not in tag:
            continue
        gh, gw = grid
        S, C = gh * gw, H * D
        g = torch.Generator(device="cuda").manual_seed(len(tag) + S + D)
        qkv = torch.randn(B, S, 3 * C, device="cuda", dtype=torch.bfloat16,
                          generator=g) * 0.5
        q, k, v = (qkv[..., i * C:(i + 1) * C].unflatten(-1, (H, D))
                   for i in range(3))
        x = torch.randn(B, S, C, device="cuda", dtype=torch.bfloat16,
                        generator=g)
        assert ops.attention_window_supported(q, k, v)
        split, merge = ops.window_split, ops.window_merge
        qw, kw, vw = (split(t, grid, window).contiguous() for t in (q, k, v))
        ref = merge(ops.attention_bshd(qw, kw, vw), grid, window)
        got = ops.attention_window_bshd(q, k, v, grid=grid, window=window)
        assert torch.equal(got, ref), f"{tag}: windowed kernel != copies"
        del ref, got

        def copies():
            a, b, c = (split(t, grid, window).contiguous() for t in (q, k, v))
            return merge(ops.attention_bshd(a, b, c), grid, window)

        routes = {
            "windowed": lambda: ops.attention_window_bshd(
                q, k, v, grid=grid, window=window),
            "prearranged": lambda: ops.attention_bshd(qw, kw, vw),
            "copies": copies,
            "full": lambda: ops.attention_bshd(q, k, v),
        }
        r = ops.tome_merge_count(gh, gw, 0.5)
        if ops.tome_match_supported(x):
            qm, km, vm = (t[:, :S - r] for t in (q, k, v))

            def tome():
                node_max, node_idx = ops.tome_match(x, gh, gw)
                plan = ops.tome_plan(node_max, node_idx, gh, gw, r)
                ops.tome_merge(x, plan)
                return ops.attention_bshd(qm, km, vm)

            routes["tome_0.5"] = tome
        times = {name: [] for name in routes}
        for fn in routes.values():  # every shape and route warmed first
            bench(fn, warm=2, it=1)
        for _ in range(args.rounds):
            for name, fn in routes.items():
                times[name].append(bench(fn, warm=1, it=args.iters))
        res = {name: _band(ts) for name, ts in times.items()}
        res["shape"] = {"B": B, "grid": grid, "window": window, "H": H, "D": D}
        out[tag] = res
        print(json.dumps({tag: res}), flush=True)
        del qkv, q, k, v, x, qw, kw, vw
        torch.cuda.empty_cache()
    return out


def bench(fn, warm=3, it=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(it):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only", default=None, help="substring filter on tag")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--variant", default=None, choices=["auto", "v2", "v3"],
                    help="flash kernel to time (default: follow SDWD_ATTN)")
    ap.add_argument("--window", action="store_true",
                    help="time Hypertile's windowed attention (five routes)")
    ap.add_argument("--batch", type=int, default=128,
                    help="--window: batch rows (headline: 64 images x CFG)")
    ap.add_argument("--rounds", type=int, default=5,
                    help="--window: alternating rounds per shape")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "GPU required"
    if args.window:
        window_main(args)
        return
    results = {}
    for tag, B, H, Sq, Sk, D in SHAPES:
        if args.only and args.only not in tag:
            continue
        g = torch.Generator(device="cuda").manual_seed(hash(tag) % 2**31)
        q = torch.randn(B, H, Sq, D, device="cuda", dtype=torch.bfloat16,
                        generator=g) * 0.5
        k = torch.randn(B, H, Sk, D, device="cuda", dtype=torch.bfloat16,
                        generator=g) * 0.5
        v = torch.randn(B, H, Sk, D, device="cuda", dtype=torch.bfloat16,
                        generator=g)
        scale = D ** -0.5
        if args.check:
            # reference on a 2-batch slice: the eager fp32 score matrix at
            # full B would need tens of GB
            with torch.no_grad():
                qs, ks, vs = q[:2], k[:2], v[:2]
                ref = torch.softmax(
                    (qs.float() @ ks.float().transpose(-1, -2)) * scale,
                    dim=-1,
                ) @ vs.float()
                got = ops.attention(qs, ks, vs, scale, args.variant).float()
                err = (got - ref).abs().max().item()
                rel = err / ref.abs().max().item()
            print(f"{tag}: max abs err {err:.4e} (rel {rel:.3e})")
            assert rel < 2e-2, f"{tag} numerics off"
            del ref, got, qs, ks, vs
        ms = bench(lambda: ops.attention(q, k, v, scale, args.variant),
                   it=args.iters) * 1e3
        tf = flops(B, H, Sq, Sk, D) / (ms * 1e-3) / 1e12
        results[tag] = {"ms": round(ms, 3), "tf": round(tf, 1)}
        print(f"{tag}: {ms:.3f} ms  {tf:.1f} TF/s (useful, D={D})")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
