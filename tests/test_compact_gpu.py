"""ops.conv_compact (conv_compact_bf16_kernel) and SRVGGNetCompact on the GPU.

The op against the fp64 formula on the same bf16 operands. Tiles are 16 x 16,
so 19 x 37 is ragged in both directions and 2 x 3 tiles an image; N = 2 and
blocks = 2 make each block walk six tiles across the image boundary; 1 x 1 is
the all-halo patch. With pre_slope the operand of the conv is prelu(x, pre)
rounded to bf16 (the op's contract: what the separate activation pass stores),
and the reference forms it the same way: the product of two bf16 values is
exact in fp32 and fp64 alike, so that rounding is the same everywhere.

Tolerance |y - ref| <= 2^-8 |ref| + 2^-14 A, A the same conv on |x|, |w|,
|bias| (+ |base|): one bf16 rounding is at most 2^-9 relative, doubled; the
577-term fp32 accumulation errs by at most 577 * 2^-24 < 2^-14 of A. |slope|
<= 0.9, so the PReLU does not enlarge either term.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops
from sdwd_amd.models.esrgan import SRVGGNetCompact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 2


@functools.lru_cache(maxsize=None)
def case(variant, h, w):
    """bf16 operands and (ref, A) in fp64, computed once per variant/shape."""
    g = torch.Generator().manual_seed(h * 100 + w)
    cout = 48 if variant == "shuffle" else 64

    def bf(*shape, s=1.0):
        return (torch.randn(*shape, generator=g) * s).bfloat16()

    x, wt, b = bf(N, 64, h, w), bf(cout, 64, 3, 3, s=0.05), bf(cout)
    slope = bf(64, s=0.3).clamp(-0.9, 0.9)
    pre = bf(64, s=0.3).clamp(-0.9, 0.9)
    base = torch.rand(N, 3, h, w, generator=g).bfloat16()
    xin = x.double()
    if variant == "pre_act":
        xin = F.prelu(xin, pre.double()).bfloat16().double()
    ref = F.conv2d(xin, wt.double(), b.double(), padding=1)
    a = F.conv2d(xin.abs(), wt.double().abs(), b.double().abs(), padding=1)
    if variant == "shuffle":
        up = F.interpolate(base.double(), scale_factor=4)
        ref = F.pixel_shuffle(ref, 4) + up
        a = F.pixel_shuffle(a, 4) + up.abs()
    else:
        ref = F.prelu(ref, slope.double())
    return dict(x=x, w=wt, b=b, slope=slope, pre=pre, base=base), ref, a


@pytest.mark.parametrize("h,w,blocks", [(19, 37, None), (19, 37, 2),
                                        (1, 1, None)])
@pytest.mark.parametrize("variant", ["prelu", "pre_act", "shuffle"])
def test_op_against_fp64(variant, h, w, blocks):
    t, ref, a = case(variant, h, w)
    x = t["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    wp = t["w"].permute(0, 2, 3, 1).contiguous().to(DEV)
    assert ops.conv_compact_supported(x, wp)
    if variant == "shuffle":
        kw = dict(shuffle_base=t["base"].to(DEV))
    else:
        kw = dict(slope=t["slope"].to(DEV),
                  pre_slope=t["pre"].to(DEV) if variant == "pre_act" else None)
    y = ops.conv_compact(x, wp, t["b"].to(DEV), blocks=blocks, **kw)
    again = ops.conv_compact(x, wp, t["b"].to(DEV), blocks=blocks, **kw)
    assert y.dtype == torch.bfloat16
    if variant == "shuffle":
        assert y.shape == (N, 3, 4 * h, 4 * w) and y.is_contiguous()
    else:
        assert y.shape == (N, 64, h, w)
    assert torch.equal(y, again)                    # no atomics
    err = (y.cpu().double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -14 * a
    print(f"COMPACT {variant} {h}x{w} blocks={blocks} "
          f"max err/bound={(err / bound).max().item():.3f}")
    assert (err <= bound).all()


def test_native_against_fp64_and_composed():
    torch.manual_seed(5)
    net = SRVGGNetCompact(nf=64, num_conv=3).eval()
    with torch.no_grad():
        for m in net.body[1::2]:                    # mixed-sign slopes
            m.weight.copy_(torch.randn(64) * 0.3)
    net = net.to(torch.bfloat16)                    # the weights under test
    x = torch.rand(2, 3, 20, 24).bfloat16()
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(x.double())
        gpu = copy.deepcopy(net).to(DEV)
        assert gpu.native_supported(x.to(DEV))
        native = gpu(x.to(DEV)).cpu()
        again = gpu(x.to(DEV)).cpu()
        composed = gpu(x.to(DEV), native=False).cpu()
    assert native.shape == (2, 3, 80, 96) and native.dtype == torch.bfloat16
    assert torch.equal(native, again)
    err_native = (native.double() - ref).abs().max().item()
    err_composed = (composed.double() - ref).abs().max().item()
    print(f"COMPACT num_conv=3 2x3x20x24 max|ref|={ref.abs().max().item():.4f} "
          f"native_err={err_native:.3e} composed_err={err_composed:.3e}")
    assert err_native <= 2.0 * err_composed
