"""hat_attn_bf16_kernel (ops.attention_hat) against an fp64 reference written
the literal way here, on the same bf16 qkv: kw 16 rolls by -shift, partitions
and adds the slice-built -100 mask; kw 24 takes F.unfold(kernel 24, stride 16,
padding 4) of K and V. The bias is a random table gathered through the model's
index buffers.

Bound (derived, the exact=True bound of tests/attention_oracle.py: scale, bias
and mask are applied to fp32 scores, so no score-side term):
|out - ref| <= 2^-7 * (p @ |v|) + 2^-8 * |ref| per element. Each case prints
its worst err/bound as "ATTN hat ...".
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops
from sdwd_amd.models.hat import (relative_position_index_oca,
                                 relative_position_index_sa)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 30 ** -0.5
INDEX = {16: relative_position_index_sa(), 24: relative_position_index_oca()}


def reference(qkv, bias, shift, kw):
    """fp64 -> (out, p @ |v|), both [B, H, W, heads * 32]; bias is the
    gathered [heads, 256, kw*kw]."""
    b, h, w, _, heads, d = qkv.shape
    nw = (h // 16) * (w // 16)
    x = torch.roll(qkv.double(), (-shift, -shift), (1, 2))

    def windows(t):                 # [b, h, w, heads, d] -> [b, nw, heads, 256, d]
        t = t.view(b, h // 16, 16, w // 16, 16, heads, d)
        return t.permute(0, 1, 3, 5, 2, 4, 6).reshape(b, nw, heads, 256, d)

    def patches(t):
        t = t.permute(0, 3, 4, 1, 2).reshape(b, heads * d, h, w)
        t = F.unfold(t, kernel_size=24, stride=16, padding=4)
        return t.view(b, heads, d, 576, nw).permute(0, 4, 1, 3, 2)

    part = windows if kw == 16 else patches
    q, k, v = windows(x[:, :, :, 0]), part(x[:, :, :, 1]), part(x[:, :, :, 2])
    s = SCALE * q @ k.transpose(-2, -1) + bias.double()
    if shift:
        img, cnt = torch.zeros(h, w), 0
        for hs in (slice(0, -16), slice(-16, -shift), slice(-shift, None)):
            for ws in (slice(0, -16), slice(-16, -shift), slice(-shift, None)):
                img[hs, ws] = cnt
                cnt += 1
        win = img.view(h // 16, 16, w // 16, 16).transpose(1, 2).reshape(-1, 256)
        differ = win[:, None, :] != win[:, :, None]
        s = s + (-100.0 * differ)[None, :, None]
    p = torch.softmax(s, -1)

    def back(t):
        t = t.view(b, h // 16, w // 16, heads, 16, 16, d)
        t = t.permute(0, 1, 4, 2, 5, 3, 6).reshape(b, h, w, heads * d)
        return torch.roll(t, (shift, shift), (1, 2))

    return back(p @ v), back(p @ v.abs())


@functools.lru_cache(maxsize=None)
def case(h, w, shift, kw, b, heads):
    g = torch.Generator().manual_seed(1000 * h + 10 * w + shift + kw + heads)
    qkv = torch.randn(b, h, w, 3, heads, 32, generator=g)
    qkv[..., 30:] = 0
    qkv = qkv.bfloat16()
    table = torch.randn((kw + 15) ** 2, heads, generator=g)
    off = ops.window_bias_offsets(table, INDEX[kw], kw)
    bias = table[INDEX[kw]].permute(2, 0, 1)
    return qkv, off, reference(qkv, bias, shift, kw)


def worst(out, ref, pav):
    bound = 2.0 ** -7 * pav + 2.0 ** -8 * ref.abs()
    return ((out.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


# one block per (window, head) and no launch walk: 16x16 is one window (every
# overlap border out of the grid), 48x32 has a middle window with neighbours
# on both sides
CASES = [(h, w, shift, kw, b, heads)
         for h, w in [(16, 16), (32, 32), (16, 48), (48, 32)]
         for shift, kw in [(0, 16), (8, 16), (0, 24)]
         for b, heads in [(1, 6), (2, 8)]]


@pytest.mark.parametrize("h,w,shift,kw,b,heads", CASES)
def test_against_fp64(h, w, shift, kw, b, heads):
    qkv, off, (ref, pav) = case(h, w, shift, kw, b, heads)
    assert ops.attention_hat_supported(qkv.to(DEV), off.to(DEV), kw)
    out = ops.attention_hat(qkv.to(DEV), off.to(DEV), SCALE, shift, kw).cpu()
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    ratio = worst(out, ref, pav)
    print(f"ATTN hat grid={h}x{w} kw={kw} shift={shift} B={b} heads={heads} "
          f"err/bound={ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("shift,kw", [(8, 16), (0, 24)])
def test_strided_view_padding_and_determinism(shift, kw):
    """qkv as a view inside a NaN-filled buffer (a NaN batch row, NaN token
    columns and NaN channels around it); the pad channels come out exactly 0
    and two runs are equal."""
    h, w, b, heads = 48, 32, 2, 8
    qkv, off, (ref, pav) = case(h, w, shift, kw, b, heads)
    buf = torch.full((b + 1, h, w + 2, 3 * heads * 32 + 8), float("nan"),
                     dtype=torch.bfloat16, device=DEV)
    view = buf[:b, :, 1:w + 1, 8:].view(b, h, w, 3, heads, 32)
    view.copy_(qkv)
    assert not view.is_contiguous()
    assert ops.attention_hat_supported(view, off.to(DEV), kw)
    out = ops.attention_hat(view, off.to(DEV), SCALE, shift, kw)
    again = ops.attention_hat(view, off.to(DEV), SCALE, shift, kw)
    assert torch.equal(out, again)
    ratio = worst(out.cpu(), ref, pav)
    print(f"ATTN hat strided grid={h}x{w} kw={kw} shift={shift} "
          f"err/bound={ratio:.3f}")
    assert ratio <= 1.0
    assert (out.view(b, h, w, heads, 32)[..., 30:] == 0).all()


def test_contract():
    qkv, off, _ = case(16, 16, 0, 16, 1, 6)
    off24 = case(16, 16, 0, 24, 1, 6)[1].to(DEV)
    qkv, off = qkv.to(DEV), off.to(DEV)
    bad = {
        "grid": (qkv[:, :8], off, 0, 16),
        "head dim": (qkv[..., :24], off, 0, 16),
        "bias dtype": (qkv, off.bfloat16(), 0, 16),
        "bias shape": (qkv, off24, 0, 16),
        "bias view": (qkv, off.transpose(1, 2), 0, 16),
        "shift 4": (qkv, off, 4, 16),
        "shift 8 at kw 24": (qkv, off24, 8, 24),
        "stride": (qkv.repeat_interleave(2, -1)[..., ::2], off, 0, 16),
    }
    for what, (a, b, shift, kw) in bad.items():
        if not what.startswith("shift"):
            assert not ops.attention_hat_supported(a, b, kw), what
        with pytest.raises(ValueError):
            ops.attention_hat(a, b, SCALE, shift, kw)
