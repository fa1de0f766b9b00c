"""The conv epilogues: the vector path (operands fetched ahead of use, the
bf16 sub-tile transposed through wave-private LDS, 16-byte stores) and the
element-wise path that serves edge tiles and launches the vector path cannot
take, on both kernels (v2 128-row tiles, v4 256-row tiles).

Reference: the fp64 conv2d of the bf16 values (of the nearest-upsampled input
for the fused upsample convs) plus bias, channel bias and residual.
Per-element bound, from the arithmetic and not from the kernels' results, as
in test_ups_fold_gpu.py:

    |out - ref| <= 2^-9 |ref| + (2^-9 + 4 Cin 2^-24) mag,
    mag = conv2d(|x|, |w|) + |bias| + |cb| + |res|

Every case asserts max(err / bound) <= 1 over all elements. Worst ratios
measured on an MI355X are in profiles/r11_conv_epilogue.md.

Exact checks on top: the element-wise path is the arithmetic the kernels had
before the vector path, so the same problem through both paths must be
bit-equal; an fp32 and a bf16 bias must give bit-equal outputs; a captured
graph must replay what eager computes.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def pad_axes(x, wrap):
    """Pad H and W by 1: circularly on the wrapped axes, zeros elsewhere."""
    x = F.pad(x, (0, 0, 1, 1), mode="circular" if wrap[0] else "constant")
    return F.pad(x, (1, 1, 0, 0), mode="circular" if wrap[1] else "constant")


NOWRAP = (False, False)
_CASES = {}


def make(dev, shape, stride=1, ups=False, wrap=NOWRAP):
    """Seeded bf16 operands of a case and its fp64 conv, made once:
    x, w_prep, bias, cb, res on the GPU; conv (no bias) and the magnitude
    conv2d(|x|, |w|) in fp64 on the CPU."""
    key = (shape, stride, ups, wrap)
    if key in _CASES:
        return _CASES[key]
    N, Cin, H, W, Cout = shape
    g = torch.Generator(device="cpu").manual_seed(
        7 + 131 * H + 17 * W + Cout + 3 * N)
    x = torch.randn(N, Cin, H, W, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5)
    w = w.to(dev, torch.bfloat16)
    b = torch.randn(Cout, generator=g).to(dev, torch.bfloat16)
    cb = torch.randn(N, Cout, generator=g).to(dev, torch.bfloat16)
    xd, wd = x.double().cpu(), w.double().cpu()
    if ups:
        xd = F.interpolate(xd, scale_factor=2, mode="nearest")
    conv = F.conv2d(pad_axes(xd, wrap), wd, stride=stride)
    mag = F.conv2d(pad_axes(xd.abs(), wrap), wd.abs(), stride=stride)
    res = torch.randn(conv.shape, generator=g).to(dev, torch.bfloat16)
    c = dict(x=cl(x), wp=w.permute(0, 2, 3, 1).contiguous(), b=b, cb=cb,
             res=cl(res), conv=conv, mag=mag, cin=Cin)
    _CASES[key] = c
    return c


def worst_ratio(out, c, bias, cb, res):
    """max err / bound against the fp64 reference with the extras in use."""
    ref, mag = c["conv"].clone(), c["mag"].clone()
    if bias:
        t = c["b"].double().cpu().view(1, -1, 1, 1)
        ref, mag = ref + t, mag + t.abs()
    if cb:
        t = c["cb"].double().cpu()[:, :, None, None]
        ref, mag = ref + t, mag + t.abs()
    if res:
        t = c["res"].double().cpu()
        ref, mag = ref + t, mag + t.abs()
    k = 2.0 ** -9 + 4 * c["cin"] * 2.0 ** -24
    bound = 2.0 ** -9 * ref.abs() + k * mag
    assert out.shape == ref.shape
    assert (bound > 0).all()
    return ((out.double().cpu() - ref).abs() / bound).max().item()


def run(c, bias=True, cb=False, res=False, stride=1, gn=False, variant=None,
        wrap=NOWRAP):
    return ops.conv3x3(c["x"], c["wp"], c["b"] if bias else None,
                       c["res"] if res else None, stride,
                       chan_bias=c["cb"] if cb else None, collect_gn=gn,
                       variant=variant, wrap=wrap)


# (shape, variant): M tails (M = 81; M = 300 crosses a 128- and a 256-row
# boundary with a partial last tile), tiles spanning four images, and the
# column cases: Cout 64, 192, 72 (% 8 == 0, no tile multiple: vector tiles
# and an edge tile), 100 (% 8 != 0: element-wise), 320 on v4 (256 + 64 with
# ldY = 320; M = 384 is one full and one half 256-row tile). At these M the
# plan gives every v2 launch here BN = 64 (fewer than 512 blocks otherwise);
# the BN = 128 form of the v2 kernel is test_v2_bn128's.
SHAPE_CASES = [
    ((1, 64, 9, 9, 64), None),
    ((3, 64, 10, 10, 128), None),
    ((8, 64, 6, 6, 64), None),
    ((3, 64, 10, 10, 192), None),
    ((3, 64, 10, 10, 72), None),
    ((3, 64, 10, 10, 100), None),
    ((3, 64, 16, 8, 320), "v4"),
    ((2, 128, 16, 8, 128), None),
]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,variant", SHAPE_CASES)
def test_shapes(dev, shape, variant, stride):
    """Bias, channel bias and residual together, at stride 1 and 2."""
    c = make(dev, shape, stride)
    out = run(c, True, True, True, stride, variant=variant)
    ratio = worst_ratio(out, c, True, True, True)
    print(f"epi {shape} s{stride} {variant}: max err/bound {ratio:.3f}")
    assert ratio <= 1.0
    plain = run(c, False, False, False, stride, variant=variant)
    ratio = worst_ratio(plain, c, False, False, False)
    print(f"epi {shape} s{stride} {variant} plain: max err/bound {ratio:.3f}")
    assert ratio <= 1.0


EXTRA_SHAPES = {"v2": (2, 64, 16, 8, 128), "v4": (2, 64, 16, 8, 256)}


@pytest.mark.parametrize("gn", [False, True])
@pytest.mark.parametrize("variant", ["v2", "v4"])
def test_extras(dev, variant, gn):
    """Every combination of bias, residual and channel bias, with and
    without the GroupNorm partials (which must not change y)."""
    c = make(dev, EXTRA_SHAPES[variant])
    worst = 0.0
    for bias, res, cb in itertools.product([False, True], repeat=3):
        out = run(c, bias, cb, res, gn=gn, variant=variant)
        assert hasattr(out, "_sdwd_gnp") == gn
        worst = max(worst, worst_ratio(out, c, bias, cb, res))
        if gn:
            assert torch.equal(out, run(c, bias, cb, res, variant=variant))
    print(f"epi extras {variant} gn={gn}: max err/bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("variant", ["v2", "v4"])
def test_residual_batch_slice(dev, variant):
    """The residual as a batch slice of a larger tensor: an offset pointer."""
    c = make(dev, EXTRA_SHAPES[variant])
    res = c["res"]
    big = cl(torch.zeros(res.shape[0] + 2, *res.shape[1:], device=dev,
                         dtype=res.dtype))
    big[1:-1] = res
    view = big[1:-1]
    assert view.data_ptr() != big.data_ptr()
    out = ops.conv3x3(c["x"], c["wp"], c["b"], view, 1, chan_bias=c["cb"],
                      variant=variant)
    assert torch.equal(out, run(c, True, True, True, variant=variant))
    assert worst_ratio(out, c, True, True, True) <= 1.0


@pytest.mark.parametrize("variant,shape", [("v2", (2, 64, 16, 8, 64)),
                                           ("v4", (2, 64, 16, 8, 256))])
def test_gn_partials(dev, variant, shape):
    """Ho*Wo = 128: one partial slot per image. The partials against fp64
    sums over the stored y (an fp32 sum of n terms in any order is within
    n 2^-24 sum|v| of the exact one), and GroupNorm from them against
    GroupNorm's own stats pass to test_gn_partials_match_standard's 0.05."""
    N, _, H, W, Cout = shape
    c = make(dev, shape)
    for bias, res, cb in [(True, False, False), (True, True, True)]:
        y = run(c, bias, cb, res, gn=True, variant=variant)
        gnp, tpi, _ = y._sdwd_gnp
        assert tpi == H * W // 128 and gnp.shape == (N * tpi, 2, Cout)
        yd = y.double()
        got = gnp.double().view(N, tpi, 2, Cout).sum(1)
        s1, s2 = yd.sum((2, 3)), (yd * yd).sum((2, 3))
        eps32 = H * W * 2.0 ** -24
        assert ((got[:, 0] - s1).abs() <= eps32 * yd.abs().sum((2, 3))).all()
        assert ((got[:, 1] - s2).abs() <= eps32 * s2).all()
        g = torch.Generator(device="cpu").manual_seed(5)
        gw = torch.randn(Cout, generator=g).to(dev)
        gb = torch.randn(Cout, generator=g).to(dev)
        fused = ops.group_norm_silu(y, gw, gb, 8, 1e-5, True)
        copy = y.detach().clone()
        assert not hasattr(copy, "_sdwd_gnp")
        std = ops.group_norm_silu(copy, gw, gb, 8, 1e-5, True)
        assert (fused.float() - std.float()).abs().max() <= 0.05


@pytest.mark.parametrize("wrap", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("variant,shape", [("v2", (3, 64, 10, 10, 128)),
                                           ("v4", (2, 64, 16, 8, 256))])
def test_wrap(dev, variant, shape, wrap):
    c = make(dev, shape, wrap=wrap)
    out = run(c, True, True, True, variant=variant, wrap=wrap)
    ratio = worst_ratio(out, c, True, True, True)
    print(f"epi wrap {wrap} {variant}: max err/bound {ratio:.3f}")
    assert ratio <= 1.0


# The upsample kernels are BN = 128, so only Cout % 128 == 0 has full tiles.
# H*W = 9 and 15 are edge tiles only. 16x9 = 144 (odd width, Cout 128) puts a
# full 128-row tile of each phase, which ends mid image row, in front of the
# ragged one; 2 x 15x9 = 270 has a full tile that starts mid row and spans
# both images. 16x8 = 128 is the shape whose partials come from the epilogue.
UPS_SHAPES = [(1, 64, 1, 9, 64), (1, 64, 3, 5, 128), (1, 64, 16, 9, 128),
              (2, 64, 15, 9, 128), (2, 64, 16, 8, 128)]


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("shape", UPS_SHAPES)
def test_upsample(dev, shape, fold):
    """FOLD (four 2x2 sub-pixel convs) and UPS (fold=False, nine taps), with
    bias and collect_gn."""
    c = make(dev, shape, ups=True)
    out = ops.ups2x_conv3x3(c["x"], c["wp"], c["b"], collect_gn=True,
                            fold=fold)
    ratio = worst_ratio(out, c, True, False, False)
    print(f"epi ups fold={fold} {shape}: max err/bound {ratio:.3f}")
    assert ratio <= 1.0
    N, _, H, W, Cout = shape
    if (4 * H * W) % 128 == 0:
        gnp, tpi, _ = out._sdwd_gnp
        yd = out.double()
        got = gnp.double().view(N, tpi, 2, Cout).sum(1)
        eps32 = 4 * H * W * 2.0 ** -24
        s1, s2 = yd.sum((2, 3)), (yd * yd).sum((2, 3))
        assert ((got[:, 0] - s1).abs() <= eps32 * yd.abs().sum((2, 3))).all()
        assert ((got[:, 1] - s2).abs() <= eps32 * s2).all()
    bare = ops.ups2x_conv3x3(c["x"], c["wp"], None, fold=fold)
    assert worst_ratio(bare, c, False, False, False) <= 1.0


@pytest.mark.parametrize("variant", ["v2", "v4"])
def test_bias_dtypes(dev, variant):
    """bf16 -> fp32 is exact: an fp32 bias (read directly), a bf16 bias (read
    directly) and an fp64 one (converted on the host) are the same bias."""
    c = make(dev, EXTRA_SHAPES[variant])
    base = run(c, True, True, True, gn=True, variant=variant)
    for dt in (torch.float32, torch.float64):
        out = ops.conv3x3(c["x"], c["wp"], c["b"].to(dt), c["res"], 1,
                          chan_bias=c["cb"], collect_gn=True, variant=variant)
        assert torch.equal(out, base)
        assert torch.equal(out._sdwd_gnp[0], base._sdwd_gnp[0])
    up = make(dev, UPS_SHAPES[4], ups=True)
    a = ops.ups2x_conv3x3(up["x"], up["wp"], up["b"])
    assert torch.equal(a, ops.ups2x_conv3x3(up["x"], up["wp"],
                                            up["b"].float()))


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("variant,cout,shape", [
    ("v2", 128, (3, 64, 10, 10)), ("v2", 128, (2, 64, 16, 8)),
    ("v4", 256, (3, 64, 16, 8)), ("v4", 256, (2, 64, 16, 8)),
])
def test_vector_path_equals_elementwise(dev, variant, cout, shape, extras):
    """Cout columns take the vector path; the same weights as the first
    Cout channels of a Cout + 4 problem (% 8 != 0) take the element-wise
    path. Those columns must be bit-equal, GroupNorm partials included.
    (v2 runs BN = 64 at these sizes; BN = 128 is test_v2_bn128.)"""
    N, Cin, H, W = shape
    wide = make(dev, (N, Cin, H, W, cout + 4))
    gn = (H * W) % 128 == 0
    res_w = wide["res"] if extras else None
    cb_w = wide["cb"] if extras else None
    yw = ops.conv3x3(wide["x"], wide["wp"], wide["b"], res_w, 1,
                     chan_bias=cb_w, collect_gn=gn, variant=variant)
    res_n = cl(wide["res"][:, :cout].contiguous()) if extras else None
    cb_n = wide["cb"][:, :cout].contiguous() if extras else None
    yn = ops.conv3x3(wide["x"], wide["wp"][:cout].contiguous(),
                     wide["b"][:cout].contiguous(), res_n, 1, chan_bias=cb_n,
                     collect_gn=gn, variant=variant)
    assert torch.equal(yn, yw[:, :cout])
    if gn:
        assert torch.equal(yn._sdwd_gnp[0], yw._sdwd_gnp[0][..., :cout])


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("shape", [(1, 64, 16, 9), (2, 64, 15, 9)])
def test_upsample_vector_path_equals_elementwise(dev, shape, fold):
    """Odd width, full tiles that start or end mid image row: 128 columns
    (vector path, per-row output mapping) against the same weights as the
    first 128 channels of a 132-column problem (element-wise path)."""
    N, Cin, H, W = shape
    wide = make(dev, (N, Cin, H, W, 132), ups=True)
    yw = ops.ups2x_conv3x3(wide["x"], wide["wp"], wide["b"], fold=fold)
    yn = ops.ups2x_conv3x3(wide["x"], wide["wp"][:128].contiguous(),
                           wide["b"][:128].contiguous(), fold=fold)
    assert torch.equal(yn, yw[:, :128])
    assert worst_ratio(yw, wide, True, False, False) <= 1.0


def ref64_gpu(x, w):
    """(conv, magnitude) of the bf16 values in fp64 on the GPU, stride 1,
    as im2col + matmul (shapes too large for a quick CPU conv)."""
    cols = F.unfold(F.pad(x.double(), (1, 1, 1, 1)), 3)   # [N, Cin*9, H*W]
    wd = w.double().reshape(w.shape[0], -1)               # [Cout, Cin*9]
    out = (wd @ cols).view(x.shape[0], -1, *x.shape[2:])
    mag = (wd.abs() @ cols.abs()).view(out.shape)
    return out, mag


# M = 32768: 256 row tiles x 2 (or 3) column tiles >= 512 blocks, so the plan
# keeps BN = 128 on the v2 kernel. 64x64 images: every tile in one image,
# partials from the epilogue. 8x8 images: Ho*Wo = 64, every tile spans two
# images (one channel-bias image index per row).
@pytest.mark.parametrize("shape", [(8, 64, 64, 64), (512, 64, 8, 8)])
def test_v2_bn128(dev, shape):
    """The BN = 128 form of the v2 kernel with residual, channel bias and
    partials: 256 columns (vector path) against the fp64 bound and, bit for
    bit, against the same weights as the first 256 channels of a 260-column
    problem (element-wise path)."""
    N, Cin, H, W = shape
    for cout in (256, 260):
        nfull, rem, bn64 = ops.ext().conv3x3_plan(N, H, W, Cin, cout, 1, 2)
        assert (nfull, rem, bn64) == (0, cout, False)
    gn = (H * W) % 128 == 0
    g = torch.Generator(device="cpu").manual_seed(1000 + H)
    x = cl(torch.randn(N, Cin, H, W, generator=g).to(dev, torch.bfloat16))
    w = (torch.randn(260, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5)
    w = w.to(dev, torch.bfloat16)
    wp = w.permute(0, 2, 3, 1).contiguous()
    b = torch.randn(260, generator=g).to(dev, torch.bfloat16)
    cb = torch.randn(N, 260, generator=g).to(dev, torch.bfloat16)
    res = cl(torch.randn(N, 260, H, W, generator=g).to(dev, torch.bfloat16))
    yw = ops.conv3x3(x, wp, b, res, 1, chan_bias=cb, collect_gn=gn,
                     variant="v2")
    yn = ops.conv3x3(x, wp[:256].contiguous(), b[:256].contiguous(),
                     cl(res[:, :256].contiguous()), 1,
                     chan_bias=cb[:, :256].contiguous(), collect_gn=gn,
                     variant="v2")
    assert torch.equal(yn, yw[:, :256])
    assert hasattr(yn, "_sdwd_gnp") == gn
    if gn:
        assert torch.equal(yn._sdwd_gnp[0], yw._sdwd_gnp[0][..., :256])
    conv, mag = ref64_gpu(x, w[:256])
    extra = (b[:256].double().view(1, -1, 1, 1)
             .expand_as(conv), cb[:, :256].double()[:, :, None, None]
             .expand_as(conv), res[:, :256].double())
    ref = conv + extra[0] + extra[1] + extra[2]
    mag = mag + extra[0].abs() + extra[1].abs() + extra[2].abs()
    bound = 2.0 ** -9 * ref.abs() + (2.0 ** -9 + 4 * Cin * 2.0 ** -24) * mag
    assert (bound > 0).all()
    ratio = ((yn.double() - ref).abs() / bound).max().item()
    print(f"epi v2 BN=128 {shape}: max err/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("variant", ["v2", "v4"])
def test_graph_replay_equals_eager(dev, variant):
    """No per-call bias copy, so nothing of a capture is a dead temporary."""
    c = make(dev, EXTRA_SHAPES[variant])
    eager = run(c, True, True, True, gn=True, variant=variant)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(c, True, True, True, gn=True, variant=variant)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(c, True, True, True, gn=True, variant=variant)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, eager)
        assert torch.equal(out._sdwd_gnp[0], eager._sdwd_gnp[0])
