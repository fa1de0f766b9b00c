"""ops.fold_ups2x_weight on the CPU: a 3x3 conv over a nearest-2x upsample
equals, per output phase (a, b) = (oh & 1, ow & 1), a 2x2 conv on the source
image with the folded weights.

The reference is conv2d(interpolate(x, 2, "nearest"), w, padding=1) in fp64.
The fold is taken from fp32 weights (so it is the unrounded fp32 fold) and
the four phase convs run in fp64: what is left is the fp32 rounding of at
most three additions per folded weight, far inside the 1e-6 relative bound.
"""
import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops

# (N, Cin, H, W, Cout)
SHAPES = [(1, 8, 3, 5, 16), (2, 16, 1, 4, 8)]


def make(N, Cin, H, W, Cout):
    g = torch.Generator().manual_seed(17 + H * 131 + W)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    return x, w


def phase_convs(x, wf):
    """x [N,Cin,H,W], wf [4,Cout,2,2,Cin] -> [N,Cout,2H,2W]: phase (a, b)
    is a 2x2 correlation whose tap (r, s) reads source (i-1+a+r, j-1+b+s),
    zero outside the image."""
    N, _, H, W = x.shape
    out = x.new_zeros(N, wf.shape[1], 2 * H, 2 * W)
    xp = F.pad(x, (1, 1, 1, 1))
    for a in (0, 1):
        for b in (0, 1):
            k = wf[2 * a + b].permute(0, 3, 1, 2)  # [Cout,Cin,2,2]
            win = xp[:, :, a:a + H + 1, b:b + W + 1]
            out[:, :, a::2, b::2] = F.conv2d(win, k)
    return out


@pytest.mark.parametrize("N,Cin,H,W,Cout", SHAPES)
def test_fold_matches_upsampled_conv(N, Cin, H, W, Cout):
    x, w = make(N, Cin, H, W, Cout)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"),
                   w.double(), padding=1)
    wp = w.permute(0, 2, 3, 1).contiguous()  # fp32 [Cout,3,3,Cin]
    wf = ops.fold_ups2x_weight(wp)
    assert wf.shape == (4, Cout, 2, 2, Cin)
    assert wf.dtype == torch.float32 and wf.is_contiguous()
    out = phase_convs(x.double(), wf.double())
    rel = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"fold vs fp64 upsampled conv: rel {rel:.3e}")
    assert rel <= 1e-6


def test_fold_rounds_once_and_is_deterministic():
    """bf16 in -> bf16 out, equal to the fp32 fold of the same bf16 values
    rounded once; two calls and the out= form are bit-identical."""
    _, w = make(1, 8, 3, 5, 16)
    wp = w.permute(0, 2, 3, 1).contiguous().bfloat16()
    wf = ops.fold_ups2x_weight(wp)
    assert wf.dtype == torch.bfloat16
    assert torch.equal(wf, ops.fold_ups2x_weight(wp.float()).bfloat16())
    assert torch.equal(wf, ops.fold_ups2x_weight(wp))
    buf = torch.empty_like(wf)
    assert ops.fold_ups2x_weight(wp, out=buf) is buf
    assert torch.equal(buf, wf)


def test_fold_entries():
    """Spot values: phase (0,0) tap (1,1) sums the four weights ky,kx in
    {1,2}; phase (1,1) tap (0,0) those in {0,1}; corner taps are single."""
    _, w = make(1, 8, 3, 5, 16)
    wp = w.permute(0, 2, 3, 1).contiguous().double()
    wf = ops.fold_ups2x_weight(wp)
    assert torch.allclose(wf[0, :, 1, 1], wp[:, 1:, 1:].sum((1, 2)),
                          rtol=0, atol=1e-12)
    assert torch.allclose(wf[3, :, 0, 0], wp[:, :2, :2].sum((1, 2)),
                          rtol=0, atol=1e-12)
    assert torch.equal(wf[0, :, 0, 0], wp[:, 0, 0])
    assert torch.equal(wf[3, :, 1, 1], wp[:, 2, 2])
    assert torch.allclose(wf[1, :, 0, 1], wp[:, 0, 2], rtol=0, atol=0)
    assert torch.allclose(wf[2, :, 1, 0], wp[:, 2, 0], rtol=0, atol=0)


def test_module_switch_and_cache_slot():
    from sdwd_amd.models.layers import SDConv2d

    assert SDConv2d.fold_upsample is True
    conv = SDConv2d(8, 16, 3, padding=1)
    wf = conv._wfold()
    assert wf is conv._wfold()  # cached
    assert torch.equal(wf, ops.fold_ups2x_weight(conv._wprep()))
    with torch.no_grad():
        conv.weight.add_(0.5)
    assert torch.equal(conv._wfold(),
                       ops.fold_ups2x_weight(conv._wprep()))
    assert not torch.equal(conv._wfold(), wf)
    conv._wprep_cache = None  # what a LoRA switch does
    assert torch.equal(conv._wfold(),
                       ops.fold_ups2x_weight(conv._wprep()))
