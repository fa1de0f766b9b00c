"""ops.conv_ragged (conv_ragged_bf16_kernel) against the fp64 conv of the same
bf16 inputs, with test_conv_dense_gpu.py's bound at the REAL Cin (the padded
products are exact zeros):

    T     = conv2d(|x|, |w|) + |bias| + |res|
    bound = 2^-8 * |ref| + (KS * KS * Cin + 8) * 2^-23 * T

Every case asserts max(err / bound) <= 1 and prints it as "RAGGED ...".

Cases (one 16 x 16 rectangle a block, 4 waves x 4 rows, 64-wide Cout tiles,
32-channel K chunks): 180 -> 180 has a 20-channel last chunk in 8-byte pieces
and three Cout tiles, the last 52 wide, on 2 x 2 ragged rectangles; 240 -> 60
a 16-byte partial last chunk and one tile narrower than 64; 60 -> 240 a
28-channel last chunk, four tiles, the residual exactly out's slice; 3 x 5 is
less than one rectangle; N = 2 puts a second image behind the first; 4 -> 4
at H = 1 is one chunk of 4 channels with both row halos outside; ksize 1; and
180-wide slices of 256-wide buffers whose other channels are NaN.
"""
import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# n, h, w, cin, cout, ksize, lrelu, res, bias, ld (0: whole tensors)
CASES = [
    (1, 17, 18, 180, 180, 3, None, "res", "bf16", 0),
    (1, 17, 18, 240, 60, 3, 0.2, None, "bf16", 0),
    (1, 9, 13, 60, 240, 3, None, "inplace", "bf16", 0),
    (1, 3, 5, 240, 64, 3, 0.01, None, "fp32", 0),
    (2, 5, 6, 180, 64, 3, None, None, None, 0),
    (1, 1, 17, 4, 4, 3, None, None, "bf16", 0),
    (1, 17, 18, 60, 60, 1, 0.2, None, "bf16", 0),
    (1, 9, 13, 180, 180, 3, None, "res", "bf16", 256),
]


@pytest.mark.parametrize("n,h,w,cin,cout,ks,lrelu,res,bias,ld", CASES)
def test_against_fp64(n, h, w, cin, cout, ks, lrelu, res, bias, ld):
    g = torch.Generator().manual_seed(7 * cin + h + ks)

    def nhwc(c):
        t = torch.randn(n, c, h, w, generator=g).bfloat16()
        return t.contiguous(memory_format=torch.channels_last)

    wt = (torch.randn(cout, cin, ks, ks, generator=g)
          / (ks * cin ** 0.5)).bfloat16()
    b = None if bias is None else torch.randn(cout, generator=g)
    if bias == "bf16":
        b = b.bfloat16()
    # x, out and res live in buffers 0, 1, 2 (res "inplace": in out's), at
    # channel offset 0 of whole tensors or 4 / 8 / 12 of NaN-filled wide ones
    offs = (4, 8, 12) if ld else (0, 0, 0)
    bufs = [nhwc(ld or cin), nhwc(ld or cout), nhwc(ld or cout)]
    if ld:
        for buf, c0, c in zip(bufs, offs, (cin, cout, cout)):
            keep = buf[:, c0:c0 + c].clone()
            buf.fill_(float("nan"))
            buf[:, c0:c0 + c] = keep
    ri = {None: None, "res": 2, "inplace": 1}[res]
    view = lambda bs, i, c: bs[i][:, offs[i]:offs[i] + c]  # noqa: E731

    xf, wf = view(bufs, 0, cin).double(), wt.double()
    bf = torch.zeros(cout).double() if b is None else b.double()
    ref = F.conv2d(xf, wf, bf, padding=ks // 2)
    T = F.conv2d(xf.abs(), wf.abs(), None, padding=ks // 2) \
        + bf.abs()[None, :, None, None]
    if lrelu is not None:
        ref = F.leaky_relu(ref, lrelu)
    if ri is not None:
        rf = view(bufs, ri, cout).double()
        ref, T = ref + rf, T + rf.abs()
    bound = 2.0 ** -8 * ref.abs() + (ks * ks * cin + 8) * 2.0 ** -23 * T

    dev = [t.to(DEV) for t in bufs]
    x, out = view(dev, 0, cin), view(dev, 1, cout)
    assert ops.conv_ragged_supported(x, wt.to(DEV), out)
    wp = ops.conv_ragged_prepare(wt.to(DEV))
    got = ops.conv_ragged(
        x, wp, None if b is None else b.to(DEV), out, ksize=ks, lrelu=lrelu,
        res=None if ri is None else view(dev, ri, cout))
    assert got.data_ptr() == out.data_ptr()
    after = [d.cpu() for d in dev]
    y = view(after, 1, cout)
    assert torch.isfinite(y.float()).all()
    worst = ((y.double() - ref).abs() / bound).max().item()
    print(f"RAGGED N={n} {h}x{w} Cin={cin} Cout={cout} ks={ks} lrelu={lrelu} "
          f"res={res} ld={ld} err/bound={worst:.3f}")
    assert worst <= 1.0
    # every byte outside the written slice is bit-unchanged
    for i, (before, aft) in enumerate(zip(bufs, after)):
        b16, a16 = before.view(torch.int16), aft.view(torch.int16)
        if i == 1:
            b16, a16 = b16.clone(), a16.clone()
            b16[:, offs[1]:offs[1] + cout] = 0
            a16[:, offs[1]:offs[1] + cout] = 0
        assert torch.equal(b16, a16)


def _bad(name):
    """Arguments of a legal call with one of them broken."""
    def nhwc(c):
        return torch.zeros(1, c, 4, 4, dtype=torch.bfloat16, device=DEV
                           ).contiguous(memory_format=torch.channels_last)

    buf = nhwc(192)
    a = dict(x=buf[:, :60], w_prepared=torch.zeros(
        64, 3, 3, 64, device=DEV, dtype=torch.bfloat16),
        bias=torch.zeros(36, device=DEV), out=buf[:, 60:96])
    kw = {}
    if name == "x":
        a["x"] = buf[0, :60]
    elif name == "w_prepared":
        a["w_prepared"] = a["w_prepared"][:36]     # not padded to 64 rows
    elif name == "bias":
        a["bias"] = torch.zeros(35, device=DEV)
    elif name == "out":
        a["out"] = buf[:, 40:76]                   # shares channels with x
    elif name == "res":
        kw["res"] = buf[:, 80:116]                 # partly overlaps out
    elif name == "lrelu":
        kw["lrelu"] = "0.2"
    elif name == "ksize":
        kw["ksize"] = 5
    return a, kw


@pytest.mark.parametrize(
    "name", ["x", "w_prepared", "bias", "out", "res", "lrelu", "ksize"])
def test_bad_argument_raises(name):
    a, kw = _bad(name)
    with pytest.raises(ValueError, match=name):
        ops.conv_ragged(a["x"], a["w_prepared"], a["bias"], a["out"], **kw)
