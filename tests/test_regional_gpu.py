"""Regional cross-attention on the GPU: the fused route (one multi-context
blend kernel) against the per-region loop, both against the fp32 CPU module
on the same weights.

Both routes share the bf16 q/k/v projections and the to_out GEMM, which
dominate the error against fp32; the fused route rounds the blended row to
bf16 once where the loop rounds every per-context output first. The fused
route's max-abs error may exceed the loop's by FUSED_OVER_LOOP at the most.
"""
import pytest
import torch

from sdwd_amd import ops
from sdwd_amd.models.unet import CrossAttention, RegionalContext
from sdwd_amd.pipeline.pipeline import _region_masks

pytestmark = pytest.mark.gpu

# Measured on an MI355X over the cases below (profiles/
# r06_regional_attention.md): the fused/loop ratio of max-abs errors ran
# from 0.945 to 1.027. The worst case plus 50% (floor 1.0): two equally
# accurate roundings differ by that much in a max over ~10^5 elements.
FUSED_OVER_LOOP = 1.54

S, GRID, B, NR, R = 256, 16, 3, 2, 2

CASES = [
    # d, heads, mode, base_ratio, region tokens
    (320, 8, "columns", 0.25, 77),
    (320, 8, "columns", 0.0, 77),
    (320, 8, "rows", 0.25, 77),
    (320, 8, "rows", 0.0, 77),
    (640, 4, "columns", 0.25, 77),
    (640, 4, "columns", 0.0, 77),
    (640, 4, "rows", 0.25, 77),
    (640, 4, "rows", 0.0, 77),
    (320, 8, "columns", 0.25, 154),
    (640, 4, "rows", 0.25, 154),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _setup(d, heads, mode, base, rtok, dev):
    torch.manual_seed(d + rtok)
    attn = CrossAttention(d, d, heads).eval().to(dev, torch.bfloat16)
    ref = CrossAttention(d, d, heads).eval()
    ref.load_state_dict({k: v.float().cpu()
                         for k, v in attn.state_dict().items()})
    x = torch.randn(B, S, d).bfloat16()
    plain = torch.randn(B, 77, d).bfloat16()
    regions = torch.randn(R, rtok, d).bfloat16()
    masks = _region_masks(mode, [1.0, 2.0], GRID, GRID)

    def ctx(device, dtype):
        return RegionalContext(plain.to(device, dtype),
                               regions.to(device, dtype), masks, rows=NR,
                               base_ratio=base, lat_hw=(GRID, GRID))

    with torch.no_grad():
        want = ref(x.float(), ctx("cpu", torch.float32))
    return attn, x.to(dev), ctx, want


def _count(monkeypatch):
    calls = {"blend": 0, "plain": 0}
    blend, plain = ops.attention_blend_bshd, ops.attention_bshd

    def counted_blend(*a, **kw):
        calls["blend"] += 1
        return blend(*a, **kw)

    def counted_plain(*a, **kw):
        calls["plain"] += 1
        return plain(*a, **kw)

    monkeypatch.setattr(ops, "attention_blend_bshd", counted_blend)
    monkeypatch.setattr(ops, "attention_bshd", counted_plain)
    return calls


@pytest.mark.parametrize("d,heads,mode,base,rtok", CASES)
def test_fused_route_against_loop_and_fp32(dev, monkeypatch, d, heads, mode,
                                           base, rtok):
    attn, x, ctx, want = _setup(d, heads, mode, base, rtok, dev)
    calls = _count(monkeypatch)
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(CrossAttention, "fused_regional", fused)
        calls["blend"] = calls["plain"] = 0
        with torch.no_grad():
            outs[fused] = attn(x, ctx(dev, torch.bfloat16)).float().cpu()
        # route: one blend + the uncond rows' plain call, or 1 + R plain
        assert (calls["blend"], calls["plain"]) == (
            (1, 1) if fused else (0, 1 + R)), (fused, calls)
    err_fused = (outs[True] - want).abs().max().item()
    err_loop = (outs[False] - want).abs().max().item()
    print(f"REGIONAL d={d} D={d // heads} {mode} base={base} rtok={rtok} "
          f"err_fused={err_fused:.5f} err_loop={err_loop:.5f} "
          f"ratio={err_fused / err_loop:.3f}")
    assert torch.isfinite(outs[True]).all()
    assert err_loop > 0
    assert err_fused <= FUSED_OVER_LOOP * err_loop
    # the uncond rows never enter the blend
    assert torch.equal(outs[True][NR:], outs[False][NR:])


def test_all_rows_regional(dev, monkeypatch):
    """rows == batch (no uncond rows, the cfg-1 fast path): the fused route
    is one blend call and nothing else."""
    attn, x, ctx, want = _setup(320, 8, "columns", 0.25, 77, dev)
    calls = _count(monkeypatch)
    monkeypatch.setattr(CrossAttention, "fused_regional", True)
    rc = ctx(dev, torch.bfloat16)[:NR]
    assert rc.rows == NR
    with torch.no_grad():
        out = attn(x[:NR], rc).float().cpu()
    assert (calls["blend"], calls["plain"]) == (1, 0)
    monkeypatch.setattr(CrossAttention, "fused_regional", False)
    with torch.no_grad():
        loop = attn(x[:NR], rc).float().cpu()
    err_fused = (out - want[:NR]).abs().max().item()
    err_loop = (loop - want[:NR]).abs().max().item()
    assert err_fused <= FUSED_OVER_LOOP * err_loop


def test_unsupported_head_dim_keeps_the_loop(dev, monkeypatch):
    """D=16 has no flash kernel: the switch is on, the loop runs."""
    calls = _count(monkeypatch)
    monkeypatch.setattr(CrossAttention, "fused_regional", True)
    d, heads = 64, 4
    torch.manual_seed(0)
    attn = CrossAttention(d, d, heads).eval().to(dev, torch.bfloat16)
    x = torch.randn(B, S, d, device=dev, dtype=torch.bfloat16)
    rc = RegionalContext(
        torch.randn(B, 77, d, device=dev, dtype=torch.bfloat16),
        torch.randn(R, 77, d, device=dev, dtype=torch.bfloat16),
        _region_masks("columns", [1.0, 1.0], GRID, GRID), rows=NR,
        base_ratio=0.25, lat_hw=(GRID, GRID))
    with torch.no_grad():
        out = attn(x, rc)
    assert calls["blend"] == 0 and calls["plain"] == 1 + R
    assert torch.isfinite(out.float()).all()
