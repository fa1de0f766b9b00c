"""The folded upsample conv: ops.ups2x_conv3x3 as four 2x2 sub-pixel convs
with fold_ups2x_weight's weights (the default route), against the fp64 conv
of the nearest-upsampled input with the ORIGINAL 3x3 weights.

Per-element bound, from the arithmetic and not from the kernel's results:

    |out - ref| <= 2^-9 |ref| + (2^-9 + 4 Cin 2^-24) conv2d(|up(x)|, |w|)

(the output's bf16 rounding; the single bf16 rounding of each folded weight,
|w_fold - exact| <= 2^-9 * sum|w| of the taps it sums; the fp32 accumulation
over K = 4 Cin products). Every test asserts max(err / bound) <= 1 over all
elements. Worst ratios measured on an MI355X are in
profiles/r07_upsample_fold.md.

Exact checks on top: the wrapped result is bit-equal to the unwrapped run on
the input padded by one source pixel and cropped by two output pixels (same
per-pixel arithmetic, different tile structure), routes are bit-equal, and
the GroupNorm partials equal fp64 sums of the stored output within the fp32
summation bound.
"""
import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops

pytestmark = pytest.mark.gpu

# (N, Cin, H, W, Cout): the smallest shapes that reach each path
SHAPES = [
    (1, 64, 4, 4, 64),       # whole phase smaller than one tile
    (1, 64, 3, 5, 128),      # odd dims, row clamp
    (1, 64, 1, 9, 64),       # H = 1: both row taps alias or leave the image
    (2, 64, 8, 8, 64),       # H*W = 64: a tile spans two images
    (1, 128, 16, 8, 64),     # H*W = 128, Cin/64 = 2: (plane, kc) decode
    (2, 64, 16, 16, 192),    # n > 0 and t > 0 in the slot; column tail
    (1, 256, 33, 17, 128),   # ragged last tile
]
WRAPS = [(True, True), (True, False), (False, True)]
GN_SHAPES = [SHAPES[3], SHAPES[4], SHAPES[5]]  # H*W = 64, 128, 256
NOWRAP = (False, False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def pad_axes(x, wrap, p=1):
    """Pad H and W by p: circularly on the wrapped axes, zeros elsewhere."""
    x = F.pad(x, (0, 0, p, p), mode="circular" if wrap[0] else "constant")
    return F.pad(x, (p, p, 0, 0), mode="circular" if wrap[1] else "constant")


_INPUTS = {}


def make(dev, shape):
    """bf16 (x channels_last, w, w_prep, bias) of a shape, made once."""
    if shape not in _INPUTS:
        N, Cin, H, W, Cout = shape
        g = torch.Generator(device="cpu").manual_seed(29 + H * 131 + W)
        x = torch.randn(N, Cin, H, W, generator=g).to(dev, torch.bfloat16)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
        w = w.to(dev, torch.bfloat16)
        b = torch.randn(Cout, generator=g).to(dev, torch.bfloat16)
        _INPUTS[shape] = (cl(x), w, w.permute(0, 2, 3, 1).contiguous(), b)
    return _INPUTS[shape]


def reference(x, w, b, wrap):
    """(ref, bound) in fp64 on the CPU from the bf16 values of x, w, b."""
    xd, wd, bd = x.double().cpu(), w.double().cpu(), b.double().cpu()
    up = F.interpolate(xd, scale_factor=2, mode="nearest")
    ref = F.conv2d(pad_axes(up, wrap), wd, bd)
    mag = F.conv2d(pad_axes(up.abs(), wrap), wd.abs())
    cin = x.shape[1]
    bound = 2.0 ** -9 * ref.abs() + (2.0 ** -9 + 4 * cin * 2.0 ** -24) * mag
    return ref, bound


_REFS = {}


def shared_reference(dev, shape, wrap):
    """reference() of make(shape), computed once per (shape, wrap)."""
    key = (shape, wrap)
    if key not in _REFS:
        x, w, _, b = make(dev, shape)
        _REFS[key] = reference(x, w, b, wrap)
    return _REFS[key]


def worst_ratio(out, ref, bound):
    assert out.shape == ref.shape
    assert (bound > 0).all()
    return ((out.double().cpu() - ref).abs() / bound).max().item()


@pytest.mark.parametrize("shape", SHAPES)
def test_vs_fp64_reference(dev, shape):
    x, w, wp, b = make(dev, shape)
    out = ops.ups2x_conv3x3(x, wp, b)
    ratio = worst_ratio(out, *shared_reference(dev, shape, NOWRAP))
    print(f"fold {shape}: max err/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_wrap(dev, shape, wrap):
    x, w, wp, b = make(dev, shape)
    out = ops.ups2x_conv3x3(x, wp, b, wrap=wrap)
    ratio = worst_ratio(out, *shared_reference(dev, shape, wrap))
    print(f"fold {shape} wrap {wrap}: max err/bound {ratio:.3f}")
    assert ratio <= 1.0
    # pad the REAL input by 1, run unwrapped, crop 2 from each side
    big = ops.ups2x_conv3x3(cl(pad_axes(x, wrap, 1)), wp, b)
    assert torch.equal(big[:, :, 2:-2, 2:-2], out)


def test_tiling_independence(dev):
    """16x8 wrapped (1 tile per phase) vs 18x10 unwrapped (2 ragged tiles
    per phase): different tiles, the same per-pixel arithmetic."""
    shape = (1, 64, 16, 8, 64)
    x, w, wp, b = make(dev, shape)
    out = ops.ups2x_conv3x3(x, wp, b, wrap=(True, True))
    xp = cl(pad_axes(x, (True, True), 1))
    assert xp.shape[2:] == (18, 10)
    big = ops.ups2x_conv3x3(xp, wp, b)
    assert torch.equal(big[:, :, 2:-2, 2:-2], out)
    assert worst_ratio(out, *shared_reference(dev, shape, (True, True))) <= 1


@pytest.mark.parametrize("shape", GN_SHAPES)
def test_partials(dev, shape):
    """Tile partials vs fp64 sums over the stored y: an fp32 sum of n terms
    in any order is within n 2^-24 sum|v| of the exact sum (n = Ho Wo per
    image and channel).

    GroupNorm from them vs GroupNorm of a copy that takes its own stats
    pass: both sets of group statistics lie within that bound (n = the G
    elements of a group) of the exact ones, so they differ by at most twice
    it. With d1 = 2 G 2^-24 mean|v| and d2 = 2 G 2^-24 mean(v^2) the bounds
    on the mean and on E[v^2], var moves by dv <= d2 + 2 |mean| d1 + d1^2
    and z = (v - mean) rstd gamma + beta by
        dz <= |gamma| rstd (d1 + |v - mean| rstd^2 dv / 2),
    to which the kernel's own fp32 arithmetic on different statistics adds
    at most 2^-20 (|z| + |beta|). SiLU is 1.1-Lipschitz, and two values dz
    apart round to bf16 values at most dz + 2^-8 |out| apart."""
    N, Cin, H, W, Cout = shape
    Ho, Wo = 2 * H, 2 * W
    x, w, wp, b = make(dev, shape)
    y = ops.ups2x_conv3x3(x, wp, b, collect_gn=True)
    assert hasattr(y, "_sdwd_gnp"), "partials not attached"
    gnp, tpi, _ = y._sdwd_gnp
    assert tpi == Ho * Wo // 128
    assert gnp.shape == (N * tpi, 2, Cout)
    assert worst_ratio(y, *shared_reference(dev, shape, NOWRAP)) <= 1.0

    yd = y.double()
    got = gnp.double().view(N, tpi, 2, Cout).sum(1)       # [N,2,C]
    s1, s2 = yd.sum((2, 3)), (yd * yd).sum((2, 3))        # [N,C]
    eps32 = Ho * Wo * 2.0 ** -24
    assert ((got[:, 0] - s1).abs() <= eps32 * yd.abs().sum((2, 3))).all()
    assert ((got[:, 1] - s2).abs() <= eps32 * s2).all()

    groups, eps = 8, 1e-5
    g = torch.Generator(device="cpu").manual_seed(5)
    gw = torch.randn(Cout, generator=g).to(dev)
    gb = torch.randn(Cout, generator=g).to(dev)
    fused = ops.group_norm_silu(y, gw, gb, groups, eps, True)
    copy = y.detach().clone()
    assert not hasattr(copy, "_sdwd_gnp")
    std = ops.group_norm_silu(copy, gw, gb, groups, eps, True)

    cg = Cout // groups
    G = cg * Ho * Wo
    v = yd.view(N, groups, cg, Ho, Wo)
    mean = v.mean((2, 3, 4), keepdim=True)
    var = v.var((2, 3, 4), unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    d1 = 2 * G * 2.0 ** -24 * v.abs().mean((2, 3, 4), keepdim=True)
    d2 = 2 * G * 2.0 ** -24 * (v * v).mean((2, 3, 4), keepdim=True)
    dv = d2 + 2 * mean.abs() * d1 + d1 * d1
    gam = gw.double().view(1, groups, cg, 1, 1)
    bet = gb.double().view(1, groups, cg, 1, 1)
    z = (v - mean) * rstd * gam + bet
    dz = gam.abs() * rstd * (d1 + (v - mean).abs() * rstd * rstd * dv / 2)
    dz = dz + 2.0 ** -20 * (z.abs() + bet.abs())
    tol = ((1.1 * dz).reshape(N, Cout, Ho, Wo)
           + 2.0 ** -8 * std.double().abs())
    diff = (fused.double() - std.double()).abs()
    print(f"gn {shape}: max diff/tol {(diff / tol).max().item():.3f}")
    assert (diff <= tol).all()


class TestRoutes:
    shape = (2, 64, 16, 16, 192)

    def _conv(self, dev):
        from sdwd_amd.models.layers import SDConv2d

        N, Cin, H, W, Cout = self.shape
        x, w, wp, b = make(dev, self.shape)
        conv = SDConv2d(Cin, Cout, 3, padding=1).to(dev, torch.bfloat16)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        return conv, x

    def test_module_equals_op_without_w_fold(self, dev):
        conv, x = self._conv(dev)
        out = conv.forward_upsampled2x(x)
        direct = ops.ups2x_conv3x3(cl(x), conv._wprep(), conv.bias,
                                   collect_gn=True)
        assert torch.equal(out, direct)
        assert torch.equal(out._sdwd_gnp[0], direct._sdwd_gnp[0])
        assert torch.equal(conv.forward_upsampled2x(x), out)
        assert torch.equal(
            ops.ups2x_conv3x3(cl(x), conv._wprep(), conv.bias,
                              collect_gn=True), direct)

    def test_nine_tap_route(self, dev, monkeypatch):
        """fold=False needs no folded weights, so it can only be the 9-tap
        kernel; the extension refuses fold=True without them."""
        from sdwd_amd.models.layers import SDConv2d

        conv, x = self._conv(dev)
        wp = conv._wprep()
        nine = ops.ups2x_conv3x3(x, wp, conv.bias, fold=False)
        raw, _ = ops.ext().ups2x_conv3x3(x, wp, conv.bias, False, False,
                                         False, None, False)
        assert torch.equal(nine, raw)
        with pytest.raises(RuntimeError, match="w_fold"):
            ops.ext().ups2x_conv3x3(x, wp, conv.bias, False, False, False,
                                    None, True)
        ratio = worst_ratio(nine, *shared_reference(dev, self.shape, NOWRAP))
        print(f"9-tap {self.shape}: max err/bound {ratio:.3f}")
        assert ratio <= 1.0
        monkeypatch.setattr(SDConv2d, "fold_upsample", False)
        assert torch.equal(conv.forward_upsampled2x(x), nine)

    def test_cache_refresh(self, dev):
        conv, x = self._conv(dev)
        before = conv.forward_upsampled2x(x)
        g = torch.Generator(device="cpu").manual_seed(41)
        delta = (torch.randn(conv.weight.shape, generator=g) * 0.05)
        with torch.no_grad():
            conv.weight.add_(delta.to(dev, torch.bfloat16))
        conv._wprep_cache = None  # what models/lora.py does on a switch
        after = conv.forward_upsampled2x(x)
        assert not torch.equal(after, before)
        ref, bound = reference(x, conv.weight.detach(), conv.bias.detach(),
                               NOWRAP)
        assert worst_ratio(after, ref, bound) <= 1.0
        assert worst_ratio(before, ref, bound) > 1.0
