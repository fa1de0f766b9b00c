"""swin_attn_bf16_kernel (ops.attention_swin) against an fp64 reference
written the literal way here: roll by -shift, partition, the slice-built -100
mask, softmax, reverse, roll back, on the same bf16 qkv and fp32 bias.

Bound (derived, the exact=True bound of tests/attention_oracle.py: scale, bias
and mask are applied to fp32 scores, so no score-side term):
|out - ref| <= 2^-7 * (p @ |v|) + 2^-8 * |ref| per element. Each case prints
its worst err/bound as "ATTN swin ...".
"""
import functools

import pytest
import torch

from sdwd_amd import ops
from sdwd_amd.models.swinir import relative_position_index

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 30 ** -0.5


def reference(qkv, bias, shift):
    """fp64 -> (out, p @ |v|), both [B, H, W, heads * 32]."""
    b, h, w, _, heads, d = qkv.shape
    x = torch.roll(qkv.double(), (-shift, -shift), (1, 2))
    x = x.view(b, h // 8, 8, w // 8, 8, 3, heads, d).permute(5, 0, 1, 3, 6, 2,
                                                             4, 7)
    q, k, v = x.reshape(3, b, h // 8 * (w // 8), heads, 64, d)
    s = SCALE * q @ k.transpose(-2, -1) + bias.double()
    if shift:
        img, cnt = torch.zeros(h, w), 0
        for hs in (slice(0, -8), slice(-8, -shift), slice(-shift, None)):
            for ws in (slice(0, -8), slice(-8, -shift), slice(-shift, None)):
                img[hs, ws] = cnt
                cnt += 1
        win = img.view(h // 8, 8, w // 8, 8).transpose(1, 2).reshape(-1, 64)
        differ = win[:, None, :] != win[:, :, None]
        s = s + (-100.0 * differ)[None, :, None]
    p = torch.softmax(s, -1)

    def back(t):
        t = t.view(b, h // 8, w // 8, heads, 8, 8, d).permute(0, 1, 4, 2, 5,
                                                              3, 6)
        return torch.roll(t.reshape(b, h, w, heads * d), (shift, shift), (1, 2))

    return back(p @ v), back(p @ v.abs())


@functools.lru_cache(maxsize=None)
def case(h, w, shift, b, heads):
    g = torch.Generator().manual_seed(1000 * h + 10 * w + shift + heads)
    qkv = torch.randn(b, h, w, 3, heads, 32, generator=g)
    qkv[..., 30:] = 0
    qkv = qkv.bfloat16()
    table = torch.randn(15 * 15, heads, generator=g)
    bias = table[relative_position_index().view(-1)].view(64, 64, heads)
    bias = bias.permute(2, 0, 1).contiguous()
    return qkv, bias, reference(qkv, bias, shift)


def worst(out, ref, pav):
    bound = 2.0 ** -7 * pav + 2.0 ** -8 * ref.abs()
    return ((out.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


# the small grids give every wave one window; the last two cases pass the
# 2048 resident waves, so a wave walks 2 (2 or 3) windows with the bias kept
# in registers and its V tile overwritten without a barrier
CASES = [(h, w, shift, b, heads)
         for h, w in [(8, 8), (16, 16), (8, 24), (24, 16)]
         for shift in (0, 4) for b, heads in [(1, 6), (2, 8)]]
CASES += [(64, 64, 4, 6, 8), (40, 80, 4, 14, 6)]


@pytest.mark.parametrize("h,w,shift,b,heads", CASES)
def test_against_fp64(h, w, shift, b, heads):
    qkv, bias, (ref, pav) = case(h, w, shift, b, heads)
    assert ops.attention_swin_supported(qkv.to(DEV), bias.to(DEV))
    walk = ops.ext().attention_swin_plan(b * (h // 8) * (w // 8), heads)[0]
    assert (walk > 1) == (b > 2)
    out = ops.attention_swin(qkv.to(DEV), bias.to(DEV), SCALE, shift).cpu()
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    ratio = worst(out, ref, pav)
    print(f"ATTN swin grid={h}x{w} shift={shift} B={b} heads={heads} "
          f"walk={walk} err/bound={ratio:.3f}")
    assert ratio <= 1.0


def test_strided_view_padding_and_determinism():
    """qkv as a view inside a NaN-filled buffer (a NaN batch row, NaN token
    columns and NaN channels around it); the pad channels come out exactly 0
    and two runs are equal."""
    h, w, shift, b, heads = 24, 16, 4, 2, 6
    qkv, bias, (ref, pav) = case(h, w, shift, b, heads)
    buf = torch.full((b + 1, h, w + 2, 3 * heads * 32 + 8), float("nan"),
                     dtype=torch.bfloat16, device=DEV)
    view = buf[:b, :, 1:w + 1, 8:].view(b, h, w, 3, heads, 32)
    view.copy_(qkv)
    assert not view.is_contiguous()
    assert ops.attention_swin_supported(view, bias.to(DEV))
    out = ops.attention_swin(view, bias.to(DEV), SCALE, shift)
    again = ops.attention_swin(view, bias.to(DEV), SCALE, shift)
    assert torch.equal(out, again)
    ratio = worst(out.cpu(), ref, pav)
    print(f"ATTN swin strided grid={h}x{w} shift={shift} err/bound={ratio:.3f}")
    assert ratio <= 1.0
    assert (out.view(b, h, w, heads, 32)[..., 30:] == 0).all()


def test_contract():
    qkv, bias, _ = case(8, 8, 0, 1, 6)
    qkv, bias = qkv.to(DEV), bias.to(DEV)
    bad = {
        "grid": (qkv[:, :4], bias, 0),
        "head dim": (qkv[..., :24], bias, 0),
        "bias dtype": (qkv, bias.bfloat16(), 0),
        "bias shape": (qkv, bias[:, :49, :49], 0),
        "bias view": (qkv, bias.transpose(1, 2), 0),
        "shift": (qkv, bias, 2),
        "stride": (qkv.repeat_interleave(2, -1)[..., ::2], bias, 0),
    }
    for what, (a, b, shift) in bad.items():
        if what != "shift":
            assert not ops.attention_swin_supported(a, b), what
        with pytest.raises(ValueError):
            ops.attention_swin(a, b, SCALE, shift)
