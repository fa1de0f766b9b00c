"""ops.swin_mlp's torch route, swin_mlp_prepare's padding and the model's
prepared-weight cache (no GPU)."""
import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops
from sdwd_amd.models.swinir import Mlp


@pytest.mark.parametrize("ln", [False, True])
def test_torch_route_is_the_composition(ln):
    torch.manual_seed(0)
    c, hidden = 20, 44
    x, res = torch.randn(2, 3, 5, c), torch.randn(2, 3, 5, c)
    w1, b1 = torch.randn(hidden, c), torch.randn(hidden)
    w2, b2 = torch.randn(c, hidden), torch.randn(c)
    g, b = (torch.randn(c), torch.randn(c)) if ln else (None, None)
    s, n = ops.swin_mlp(x, res, w1, b1, w2, b2, g, b, eps=1e-6)
    want = res + F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)
    assert torch.equal(s, want)
    if ln:
        assert torch.equal(n, F.layer_norm(want, (c,), g, b, 1e-6))
    else:
        assert n is None


@pytest.mark.parametrize("c,hidden,cpad,hp", [(180, 360, 192, 384),
                                              (240, 480, 256, 480),
                                              (196, 32, 256, 32)])
def test_prepare_pads_with_zeros(c, hidden, cpad, hp):
    torch.manual_seed(1)
    w1, b1 = torch.randn(hidden, c).bfloat16(), torch.randn(hidden).bfloat16()
    w2, b2 = torch.randn(c, hidden).bfloat16(), torch.randn(c).bfloat16()
    w1p, b1p, w2p, b2p = ops.swin_mlp_prepare(w1, b1, w2, b2)
    assert w1p.shape == (hp, cpad) and w1p.dtype == torch.bfloat16
    assert w2p.shape == (hp // 32, cpad, 32) and w2p.dtype == torch.bfloat16
    assert b1p.shape == (hp,) and b1p.dtype == torch.float32
    assert b2p.shape == (c,) and b2p.dtype == torch.float32
    assert torch.equal(w1p[:hidden, :c], w1)
    w2full = w2p.permute(1, 0, 2).reshape(cpad, hp)   # [column, hidden]
    assert torch.equal(w2full[:c, :hidden], w2)
    assert torch.equal(b1p[:hidden], b1.float()) and torch.equal(b2p, b2.float())
    # everything outside the real block is zero
    assert w1p.count_nonzero() == w1.count_nonzero()
    assert w2p.count_nonzero() == w2.count_nonzero()
    assert b1p[hidden:].count_nonzero() == 0


def test_mlp_prepared_follows_the_weights():
    torch.manual_seed(2)
    mlp = Mlp(20, 40)
    first = mlp.prepared()
    assert all(a is b for a, b in zip(first, mlp.prepared()))
    with torch.no_grad():
        mlp.fc2.weight.mul_(2.0)
    again = mlp.prepared()
    assert again[2] is not first[2]
    want = ops.swin_mlp_prepare(mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight,
                                mlp.fc2.bias)
    assert all(torch.equal(a, b) for a, b in zip(again, want))
