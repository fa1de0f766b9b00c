"""window_block_attn_bf16_kernel (ops.window_attn_block) against an fp64
reference of its definition written the literal way here: LN1, roll by -shift,
partition, QKV, rel[:, relation], an -inf mask filled by slices, softmax,
proj, reverse, roll back, residual, LN2, on the same bf16 x and weights.

Tolerance: the kernel rounds to bf16 at n1, q/k/v, P, o and the outputs. The
"rounding model" is the same fp64 definition with bf16 rounding at exactly
those points. Asserted: RMS(kernel - ref) <= 2 * RMS(model - ref) for y and
n2 (room for accumulation order only), and max |kernel - model| <=
2^-6 * (1 + |ref|) (four bf16 ulps of the output). Each case prints
"WBLK ..." with the measured ratios.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 32 ** -0.5
EPS = 1e-5


def bf16_round(t):
    return t.bfloat16().double()


def definition(x, p, shift, rd):
    """fp64 (y, n2); rd rounds at the kernel's five points (identity: the
    reference)."""
    b, h, w, c = x.shape
    heads, nw = c // 32, (h // 8) * (w // 8)
    xd = x.double()
    n1 = rd(F.layer_norm(xd, (c,), p["g1"].double(), p["b1"].double(), EPS))
    t = torch.roll(n1, (-shift, -shift), (1, 2))
    t = t.view(b, h // 8, 8, w // 8, 8, c).permute(0, 1, 3, 2, 4, 5)
    qkv = rd(t.reshape(b, nw, 64, c) @ p["wqkv"].double().T
             + p["bqkv"].double())
    q, k, v = qkv.view(b, nw, 64, 3, heads, 32).permute(3, 0, 1, 4, 2, 5)
    coord = torch.tensor([[i, j] for i in range(8) for j in range(8)])
    relation = coord[:, None] - coord[None, :] + 7
    s = SCALE * q @ k.transpose(-2, -1) \
        + p["rel"].double()[:, relation[..., 0], relation[..., 1]]
    if shift:
        mask = torch.zeros(h // 8, w // 8, 8, 8, 8, 8, dtype=torch.bool,
                           device=x.device)
        mask[-1, :, :4, :, 4:, :] = True
        mask[-1, :, 4:, :, :4, :] = True
        mask[:, -1, :, :4, :, 4:] = True
        mask[:, -1, :, 4:, :, :4] = True
        s = s.masked_fill(mask.view(1, nw, 1, 64, 64), float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    o = rd(rd(e) @ v / e.sum(-1, keepdim=True))          # [b, nw, heads, 64, 32]
    o = o.transpose(2, 3).reshape(b, nw, 64, c) @ p["wp"].double().T
    o = o.view(b, h // 8, w // 8, 8, 8, c).permute(0, 1, 3, 2, 4, 5)
    y = xd + torch.roll(o.reshape(b, h, w, c), (shift, shift), (1, 2)) \
        + p["bp"].double()
    n2 = F.layer_norm(y, (c,), p["g2"].double(), p["b2"].double(), EPS)
    return rd(y), rd(n2)


@functools.lru_cache(maxsize=None)
def params(c):
    g = torch.Generator().manual_seed(c)

    def rn(*shape, s=1.0):
        return (torch.randn(*shape, generator=g) * s).to(DEV)

    p = dict(wqkv=rn(3 * c, c, s=c ** -0.5).bfloat16(),
             wp=rn(c, c, s=c ** -0.5).bfloat16(), bqkv=rn(3 * c, s=0.5),
             bp=rn(c, s=0.5), rel=rn(c // 32, 15, 15), g1=1 + rn(c, s=0.3),
             b1=rn(c, s=0.3), g2=1 + rn(c, s=0.3), b2=rn(c, s=0.3))
    p["prep"] = ops.window_attn_block_prepare(p["wqkv"], p["wp"])
    return p


@functools.lru_cache(maxsize=None)
def case(c, h, w, shift, b):
    g = torch.Generator().manual_seed(1000 * h + 10 * w + shift + c)
    x = torch.randn(b, h, w, c, generator=g).bfloat16().to(DEV)
    p = params(c)
    return x, definition(x, p, shift, lambda t: t), \
        definition(x, p, shift, bf16_round)


def run(x, c, shift, out=None):
    p = params(c)
    return ops.window_attn_block(
        x, p["g1"], p["b1"], p["prep"][0], p["bqkv"], p["rel"], p["prep"][1],
        p["bp"], p["g2"], p["b2"], SCALE, shift, EPS, out=out)


def check(tag, got, ref, model):
    for name, o, r, m in zip(("y", "n2"), got, ref, model):
        rms = (o.double() - r).square().mean().sqrt().item()
        base = (m - r).square().mean().sqrt().item()
        worst = ((o.double() - m).abs() / (1 + r.abs())).max().item()
        print(f"WBLK {tag} {name}: rms/model {rms / base:.3f} "
              f"max|k-model|/(1+|ref|) {worst:.2e}")
        assert rms <= 2 * base
        assert worst <= 2.0 ** -6


# one wave a window, then (160 x 160, B 6: 2400 windows) past the 2048
# resident waves, so a wave walks two windows
CASES = [(c, h, w, shift, b) for c in (32, 64)
         for (h, w) in ((8, 8), (16, 24), (24, 16)) for shift in (0, 4)
         for b in (1, 3)]
WALK = [(32, 160, 160, 4, 6), (64, 160, 160, 4, 6)]


@pytest.mark.parametrize("c,h,w,shift,b", CASES + WALK)
def test_kernel_matches_definition(c, h, w, shift, b):
    x, ref, model = case(c, h, w, shift, b)
    walk, _ = ops.ext().window_block_attn_plan(b * (h // 8) * (w // 8), c)
    assert (walk > 1) == ((c, h, w, shift, b) in WALK)
    check(f"c{c} {h}x{w} s{shift} b{b}", run(x, c, shift), ref, model)


@pytest.mark.parametrize("c", [32, 64])
def test_strided_views(c):
    """x and y are channel slices of NaN-filled NHWC buffers: the kernel reads
    and writes through the strides and touches nothing else."""
    h, w, shift, b = 16, 24, 4, 1
    x, ref, model = case(c, h, w, shift, b)
    nan = float("nan")
    xbuf = torch.full((b + 1, h, w + 2, 2 * c + 8), nan, device=DEV,
                      dtype=torch.bfloat16)
    xs = xbuf[:b, :, :w, c:2 * c]
    xs.copy_(x)
    assert ops.window_attn_block_supported(xs, torch.empty_like(x),
                                           torch.empty_like(x))
    outs = []
    for _ in range(2):
        ybuf = torch.full_like(xbuf, nan)
        n2 = torch.empty_like(x)
        run(xs, c, shift, out=(ybuf[:b, :, :w, c:2 * c], n2))
        outs.append((ybuf, n2))
    (ybuf, n2), (ybuf2, n2b) = outs
    check(f"strided c{c}", (ybuf[:b, :, :w, c:2 * c], n2), ref, model)
    assert torch.equal(n2, n2b)
    assert torch.equal(ybuf.nan_to_num(7.0), ybuf2.nan_to_num(7.0))
    keep = torch.ones_like(ybuf, dtype=torch.bool)
    keep[:b, :, :w, c:2 * c] = False
    assert ybuf[keep].isnan().all() and not ybuf[~keep].isnan().any()


@pytest.mark.parametrize("what", ["c48", "odd_stride", "fp16_out", "h12",
                                  "rel_shape"])
def test_refusals(what):
    c = 48 if what == "c48" else 32
    h = 12 if what == "h12" else 16
    x = torch.zeros(1, h, 16, c, device=DEV, dtype=torch.bfloat16)
    if what == "odd_stride":
        x = torch.zeros(1, h, 16, c + 4, device=DEV,
                        dtype=torch.bfloat16)[..., :c]
    p = dict(params(32))
    out = None
    if what == "fp16_out":
        out = (torch.empty_like(x, dtype=torch.float16), torch.empty_like(x))
    if what == "rel_shape":
        p["rel"] = torch.zeros(1, 225, device=DEV)
    with pytest.raises(ValueError):
        ops.window_attn_block(
            x, p["g1"], p["b1"], p["prep"][0], p["bqkv"], p["rel"],
            p["prep"][1], p["bp"], p["g2"], p["b2"], SCALE, 0, EPS, out=out)
