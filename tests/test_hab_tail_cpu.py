"""The torch routes of ops.channel_gate and ops.gated_add_layer_norm on fp32
CPU tensors against the written-out formula in fp64, and their ValueErrors.
"""
import pytest
import torch

from sdwd_amd import ops

B, H, W, C, S = 2, 3, 5, 12, 3


def _inputs():
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=r(B, H, W, C), a=r(B, H, W, C), c=r(B, H, W, C) + r(C),
                w1=r(S, C), b1=r(S), w2=r(C, S), b2=r(C), w=r(C), b=r(C))


def _gate64(t, scale):
    d = {k: v.double() for k, v in t.items()}
    hidden = torch.relu(d["c"].mean((1, 2)) @ d["w1"].T + d["b1"])
    return scale * torch.sigmoid(hidden @ d["w2"].T + d["b2"])


@pytest.mark.parametrize("scale", [1.0, 0.01])
def test_channel_gate_torch_route(scale):
    t = _inputs()
    gate = ops.channel_gate(t["c"], t["w1"], t["b1"], t["w2"], t["b2"], scale)
    assert gate.shape == (B, C) and gate.dtype == torch.float32
    torch.testing.assert_close(gate.double(), _gate64(t, scale), rtol=1e-5,
                               atol=0)


@pytest.mark.parametrize("gated", [True, False])
def test_gated_add_layer_norm_torch_route(gated):
    t = _inputs()
    gate = _gate64(t, 1.0).float() if gated else None
    s, ln = ops.gated_add_layer_norm(t["x"], t["a"], t["c"] if gated else None,
                                     gate, t["w"], t["b"], 1e-5)
    ref = t["x"].double() + t["a"].double()
    if gated:
        ref = ref + gate.double()[:, None, None, :] * t["c"].double()
    mean = ref.mean(-1, keepdim=True)
    var = ((ref - mean) ** 2).mean(-1, keepdim=True)
    ref_ln = (ref - mean) / (var + 1e-5).sqrt() * t["w"].double() \
        + t["b"].double()
    # relative to the tensor's scale: a single entry may cancel to near zero
    for out, want in ((s, ref), (ln, ref_ln)):
        assert (out.double() - want).abs().max() <= 1e-5 * want.abs().max()


def test_value_errors():
    t = _inputs()
    x, a, c, w, b = t["x"], t["a"], t["c"], t["w"], t["b"]
    gate = torch.ones(B, C)
    with pytest.raises(ValueError, match="both c and gate"):
        ops.gated_add_layer_norm(x, a, c, None, w, b)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.gated_add_layer_norm(x[..., :10], a[..., :10], None, None,
                                 w[:10], b[:10])
    with pytest.raises(ValueError, match="a .* must have x's shape"):
        ops.gated_add_layer_norm(x, a[:, :2], c, gate, w, b)
    with pytest.raises(ValueError, match="gate"):
        ops.gated_add_layer_norm(x, a, c, gate[:1], w, b)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.channel_gate(c[..., :10], t["w1"][:, :10], t["b1"],
                         t["w2"][:10], t["b2"][:10])
    with pytest.raises(ValueError, match="w2"):
        ops.channel_gate(c, t["w1"], t["b1"], t["w2"].T, t["b2"])
