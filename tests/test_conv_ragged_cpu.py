"""ops.conv_ragged off the GPU: the padded weight layout, the CPU route of the
op, and SwinIR's native_convs switch (no effect on the CPU's plain route)."""
import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops
from sdwd_amd.models.swinir import SwinIR


@pytest.mark.parametrize("cout,cin,ks", [(180, 180, 3), (60, 240, 3),
                                         (60, 60, 1), (4, 4, 3), (64, 32, 1)])
def test_prepare_pads_with_zeros(cout, cin, ks):
    w = torch.randn(cout, cin, ks, ks)
    p = ops.conv_ragged_prepare(w)
    cp, kp = -(-cout // 64) * 64, -(-cin // 32) * 32
    assert p.shape == (cp, ks, ks, kp) and p.dtype == w.dtype
    assert torch.equal(p[:cout, :, :, :cin], w.permute(0, 2, 3, 1))
    # everything outside the real block: padded rows, padded channels
    assert (p[cout:] == 0).all() and (p[..., cin:] == 0).all()


@pytest.mark.parametrize("ks,lrelu,with_res", [(3, None, True), (3, 0.2, False),
                                               (1, 0.01, True)])
def test_cpu_route_is_conv2d(ks, lrelu, with_res):
    g = torch.Generator().manual_seed(ks)
    x = torch.randn(2, 20, 5, 6, generator=g).contiguous(
        memory_format=torch.channels_last)
    w = torch.randn(12, 20, ks, ks, generator=g)
    b = torch.randn(12, generator=g)
    res = torch.randn(2, 12, 5, 6, generator=g).contiguous(
        memory_format=torch.channels_last) if with_res else None
    out = torch.empty(2, 12, 5, 6).contiguous(
        memory_format=torch.channels_last)
    got = ops.conv_ragged(x, ops.conv_ragged_prepare(w), b, out, ksize=ks,
                          lrelu=lrelu, res=res)
    ref = F.conv2d(x, w, b, padding=ks // 2)
    if lrelu is not None:
        ref = F.leaky_relu(ref, lrelu)
    if with_res:
        ref = ref + res
    assert got is out
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)


def test_swinir_flag_has_no_effect_on_cpu():
    torch.manual_seed(0)
    net = SwinIR(180, (2,), 6, 2.0, "1conv").eval()
    x = torch.rand(1, 3, 8, 8)
    assert SwinIR.native_convs is True
    with torch.no_grad():
        on = net(x)
        net.native_convs = False
        off = net(x)
    assert on.shape == (1, 3, 32, 32)
    assert torch.equal(on, off)
