"""models/scunet.py on the GPU: the native bf16 route against the fp32 plain
route on the same bf16-rounded weights. The tolerance is measured: the bf16
plain route's RMS error against fp32 is what bf16 costs through this depth,
and the native route (fused attention on and off) may be at most 1.5x that
(different rounding points, not different math). Prints "SCUNET ...".
"""
import copy
import functools

import pytest
import torch

from sdwd_amd import ops
from sdwd_amd.models.scunet import SCUNet
from test_scunet_cpu import small_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def setup():
    net = small_model().to(DEV, torch.bfloat16)
    x = torch.rand(1, 3, 64, 128,
                   generator=torch.Generator().manual_seed(5)).to(DEV)
    x = x.bfloat16()
    with torch.no_grad():
        ref = copy.deepcopy(net).float()(x.float(), native=False)
        base = net(x, native=False).float()
    return net, x, ref, (base - ref).square().mean().sqrt().item()


@pytest.mark.parametrize("fused", [True, False])
def test_native_route_within_bf16_baseline(fused):
    net, x, ref, base = setup()
    net.fused_attention = fused
    try:
        with torch.no_grad():
            out = net(x).float()
    finally:
        net.fused_attention = SCUNet.fused_attention
    rms = (out - ref).square().mean().sqrt().item()
    print(f"SCUNET fused={fused}: native rms {rms:.3e} bf16-plain rms "
          f"{base:.3e} ratio {rms / base:.3f}")
    assert out.shape == x.shape and torch.isfinite(out).all()
    assert rms <= 1.5 * base


def test_fused_kernel_is_the_route_at_the_top_levels():
    """The views the model passes at c = 32 and 64 (the trans half of
    conv1_1's NHWC output) are ones the kernel takes; at 128 it is not."""
    for c, hw, takes in ((32, 64, True), (64, 32, True), (128, 16, False)):
        a = torch.empty(1, hw, 2 * hw, 2 * c, device=DEV, dtype=torch.bfloat16)
        x = a.permute(0, 3, 1, 2)[:, c:].permute(0, 2, 3, 1)
        y = torch.empty(x.shape, device=DEV, dtype=torch.bfloat16)
        assert ops.window_attn_block_supported(x, y, torch.empty_like(y)) \
            == takes
    assert SCUNet.fused_attention
