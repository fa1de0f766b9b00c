"""swin_mlp_bf16_kernel against an fp64 reference on the same bf16 x / res /
weights and fp32 biases / gamma / beta.

The bound is derived, not tuned. The only rounding the reference lacks is the
bf16 hidden operand (relative 2^-9) plus fp32 accumulation. With h the fp64
hidden activation, E = 2^-8 (|h| |W2|^T) elementwise, and

  |sum - ref_sum| <= E + 2^-8 |ref_sum|
  |ln  - ref_ln | <= 2 |g|/sigma (E + mean_row(E) + |s^| rms_row(E))
                     + 2^-8 |ref_ln|

the second line being the first-order propagation of a perturbation e,
|e| <= E, through LayerNorm (g/sigma (e - mean e - s^ mean(s^ e)), with
|mean(s^ e)| <= rms(e)); the factor 2 covers higher order."""
import copy

import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops
from sdwd_amd.models.swinir import SwinIR

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _inputs(c, hidden, r, seed=0):
    g = torch.Generator().manual_seed(seed)

    def n(*s):
        return torch.randn(*s, generator=g)

    p = dict(x=n(r, c).bfloat16(), res=(2 * n(r, c)).bfloat16(),
             w1=(n(hidden, c) / c ** 0.5).bfloat16(), b1=0.5 * n(hidden),
             w2=(n(c, hidden) / hidden ** 0.5).bfloat16(), b2=0.5 * n(c),
             gamma=1 + 0.5 * n(c), beta=0.5 * n(c))
    return {k: v.cuda() for k, v in p.items()}


def _run(p, ln):
    prep = ops.swin_mlp_prepare(p["w1"], p["b1"], p["w2"], p["b2"])
    norm = (p["gamma"], p["beta"]) if ln else (None, None)
    return ops.swin_mlp(p["x"], p["res"], *prep, *norm, eps=EPS)


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("r", [1, 64, 200])
@pytest.mark.parametrize("c,hidden", [(180, 360), (240, 480), (172, 100),
                                      (196, 32)])
def test_swin_mlp_matches_fp64(c, hidden, r, ln):
    p = _inputs(c, hidden, r)
    d = {k: v.double() for k, v in p.items()}
    h = F.gelu(d["x"] @ d["w1"].T + d["b1"])
    ref = h @ d["w2"].T + d["b2"] + d["res"]
    e = 2.0 ** -8 * (h.abs() @ d["w2"].abs().T)
    got_sum, got_ln = _run(p, ln)
    worst = ((got_sum.double() - ref).abs()
             / (e + 2.0 ** -8 * ref.abs())).max().item()
    if ln:
        sigma = (ref.var(-1, unbiased=False, keepdim=True) + EPS).sqrt()
        shat = (ref - ref.mean(-1, keepdim=True)) / sigma
        ref_ln = shat * d["gamma"] + d["beta"]
        bound = 2 * d["gamma"].abs() / sigma * (
            e + e.mean(-1, keepdim=True)
            + shat.abs() * e.pow(2).mean(-1, keepdim=True).sqrt()
        ) + 2.0 ** -8 * ref_ln.abs()
        worst = max(worst,
                    ((got_ln.double() - ref_ln).abs() / bound).max().item())
    else:
        assert got_ln is None
    print(f"MLP swin C={c} hid={hidden} R={r} ln={ln} err/bound={worst:.3f}")
    assert worst <= 1.0


def test_swin_mlp_contract():
    p = _inputs(180, 360, 2 * 3 * 40)
    p["x"], p["res"] = p["x"].view(2, 3, 40, 180), p["res"].view(2, 3, 40, 180)
    a, b = _run(p, True), _run(p, True)
    for t, u in zip(a, b):
        assert torch.equal(t, u)
        assert t.shape == p["x"].shape and t.dtype == torch.bfloat16
        assert t.is_contiguous()

    prep = ops.swin_mlp_prepare(p["w1"], p["b1"], p["w2"], p["b2"])
    x, res = p["x"], p["res"]

    def wide(c):
        t = torch.zeros(8, c, device="cuda", dtype=torch.bfloat16)
        return (t, t) + prep

    bad = {
        "swin_mlp_prepare": (x, res, p["w1"], p["b1"], p["w2"], p["b2"]),
        "contiguous": (x.transpose(1, 2), res.transpose(1, 2)) + prep,
        "multiple of 4": wide(182),
        "at most 256": wide(260),
    }
    assert ops.swin_mlp_supported(x, res, prep[0], prep[2])
    for reason, args in bad.items():
        assert not ops.swin_mlp_supported(args[0], args[1], args[2], args[4])
        with pytest.raises(ValueError, match=reason):
            ops.swin_mlp(*args)
    # the fp32 vectors are no argument of the predicate, but are checked
    with pytest.raises(ValueError, match="ln_weight must be fp32"):
        ops.swin_mlp(x, res, *prep, p["gamma"].bfloat16(), p["beta"])
    with pytest.raises(ValueError, match=r"b2 must be \[180\]"):
        ops.swin_mlp(x, res, *prep[:3], prep[3][:176])


@pytest.mark.parametrize("c,hidden", [(180, 360), (240, 480)])
def test_swin_mlp_rows_at_an_8_byte_offset(c, hidden):
    """x and res are read in 8-byte pieces at every C, so a contiguous view 8
    bytes into a buffer is taken and gives the same bits."""
    p = _inputs(c, hidden, 40)
    want = _run(p, True)
    for k in ("x", "res"):
        buf = torch.empty(40 * c + 4, device="cuda", dtype=torch.bfloat16)
        p[k] = buf[4:].view(40, c).copy_(p[k])
        assert p[k].data_ptr() % 16 == 8
    for t, u in zip(_run(p, True), want):
        assert torch.equal(t, u)


@pytest.mark.parametrize("embed,heads", [(320, 10), (90, 3)])
def test_model_keeps_the_composed_mlp_at_other_widths(embed, heads):
    """An embed width the kernel has no instantiation for (above 256, no
    multiple of 4) still runs the native route, MLP composed, under the
    condition of tests/test_swinir_gpu.py: at most twice the error of the
    native=False bf16 route against the fp64 run of the same weights."""
    assert not ops.swin_mlp_width_supported(embed)
    torch.manual_seed(embed)
    net = SwinIR(embed, (2,), heads, 2.0, "1conv").eval()
    with torch.no_grad():
        for name, q in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                q.normal_(0, 1)
    net = net.to(torch.bfloat16)
    x = torch.rand(2, 3, 20, 27).bfloat16()         # reflect-padded to 24x32
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(x.double())
        gpu = copy.deepcopy(net).cuda()
        assert gpu.native_supported(x.cuda())
        native = gpu(x.cuda()).cpu()
        plain = gpu(x.cuda(), native=False).cpu()
    err_native = (native.double() - ref).abs().max().item()
    err_plain = (plain.double() - ref).abs().max().item()
    print(f"MLP swin model embed={embed} native_err={err_native:.3e} "
          f"plain_err={err_plain:.3e}")
    assert err_native <= 2.0 * err_plain
