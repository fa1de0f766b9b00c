"""ops.channel_gate, ops.gated_add_layer_norm and ops.add_layer_norm at widths
that are no multiple of 8 (hab_tail.hip) against an fp64 evaluation of the
same bf16 inputs.

Bounds: one bf16 rounding is 2^-9 relative, taken with a factor 2; the
absolute terms (2^-14 of the summands, 2^-12 |w|, 2^-16 on the gate) are far
above fp32 rounding and below what a wrong gate, row or batch element moves.
"""
import functools

import pytest
import torch

from sdwd_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
# (1, 1, 1): one row, one partly filled wave. (2, 5, 7): 35 rows a batch
# element against 8 to 32 rows a wave, so waves straddle the batch boundary.
# (3, 67, 61): 4087 rows a batch element are 16 pool chunks of 256 rows, the
# last one of 247.
GRIDS = [(1, 1, 1), (2, 5, 7), (3, 67, 61)]
# 180: 8-byte rows; 144: 16-byte rows; 4: one piece a row (16-lane groups);
# 256: every lane of a 64-lane group
WIDTHS = [180, 144, 4, 256]


@functools.lru_cache(maxsize=None)
def _inputs(C, grid):
    g = torch.Generator(device=DEV).manual_seed(C * 1000 + grid[1])
    S = 1 if C == 4 else 6

    def r(*shape, dtype=torch.float32):
        return torch.randn(*shape, device=DEV, generator=g).to(dtype)

    bf = torch.bfloat16
    return dict(
        x=r(*grid, C, dtype=bf), a=r(*grid, C, dtype=bf),
        c=(r(*grid, C) + 1.5 * r(C)).to(bf),       # means differ by channel
        w1=r(S, C) / C ** 0.5, b1=r(S),
        w2=r(C, S) * 3.0 / S ** 0.5, b2=r(C),      # sigmoid arguments ~ +-3
        w=r(C), b=r(C))


def _reference(t, scale):
    """(gate, sum, ln) in fp64; gate None and sum = x + a without a scale."""
    d = {k: v.double() for k, v in t.items()}
    s, gate, gc = d["x"] + d["a"], None, 0.0
    if scale is not None:
        hidden = torch.relu(d["c"].mean((1, 2)) @ d["w1"].T + d["b1"])
        gate = scale * torch.sigmoid(hidden @ d["w2"].T + d["b2"])
        gc = gate[:, None, None, :] * d["c"]
        s = s + gc
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    ln = (s - mean) / (var + EPS).sqrt() * d["w"] + d["b"]
    mag = d["x"].abs() + d["a"].abs() + (gc.abs() if gate is not None else 0)
    return gate, s, ln, mag


@pytest.mark.parametrize("scale", [1.0, 0.01, None])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("C", WIDTHS)
def test_against_fp64(C, grid, scale):
    t = _inputs(C, grid)
    ref_gate, ref_s, ref_ln, mag = _reference(t, scale)

    def run():
        if scale is None:
            assert ops.hab_tail_supported(t["x"], t["a"])
            return (None,) + ops.gated_add_layer_norm(
                t["x"], t["a"], None, None, t["w"], t["b"], EPS)
        assert ops.hab_tail_supported(t["x"], t["a"], t["c"])
        gate = ops.channel_gate(t["c"], t["w1"], t["b1"], t["w2"], t["b2"],
                                scale)
        return (gate,) + ops.gated_add_layer_norm(
            t["x"], t["a"], t["c"], gate, t["w"], t["b"], EPS)

    gate, s, ln = run()
    r_s = ((s.double() - ref_s).abs()
           / (2.0 ** -8 * ref_s.abs() + 2.0 ** -14 * mag)).max().item()
    r_ln = ((ln.double() - ref_ln).abs()
            / (2.0 ** -8 * ref_ln.abs()
               + 2.0 ** -12 * t["w"].double().abs())).max().item()
    r_g = 0.0 if gate is None else \
        ((gate.double() - ref_gate).abs().max() / 2.0 ** -16).item()
    print(f"HABTAIL C={C} grid={grid} scale={scale} err/bound: "
          f"sum={r_s:.3f} ln={r_ln:.3f} gate={r_g:.3f}")
    assert r_s <= 1 and r_ln <= 1 and r_g <= 1
    if scale is None:
        assert torch.equal(
            s, (t["x"].float() + t["a"].float()).bfloat16())
    else:
        assert gate.dtype == torch.float32 and gate.shape == (grid[0], C)
        for first, again in zip((gate, s, ln), run()):
            assert torch.equal(first, again)


def test_add_layer_norm_takes_the_kernel_at_180():
    t = _inputs(180, (1, 1, 1))
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(5, 180, device=DEV, generator=g).bfloat16()
    r = torch.randn(5, 180, device=DEV, generator=g).bfloat16()
    assert ops.hab_tail_supported(x, r)
    s, ln = ops.add_layer_norm(x, r, t["w"], t["b"], EPS)
    ks, kln = ops.gated_add_layer_norm(x, r, None, None, t["w"], t["b"], EPS)
    assert torch.equal(s, ks) and torch.equal(ln, kln)
    assert torch.equal(s, (x.float() + r.float()).bfloat16())
