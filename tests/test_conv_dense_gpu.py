"""ops.conv3x3_dense (conv3x3_dense_bf16_kernel) against the fp64 conv of the
same bf16 inputs, with the bound derived from the arithmetic:

    T     = |alpha| * (conv2d(|x|, |w|) + |bias|) + |beta| * |res1| + |res2|
    bound = 2^-8 * |ref| + (9 * Cin + 8) * 2^-23 * T

(the output's bf16 rounding with the usual factor 2, plus the fp32
accumulation over 9 * Cin exact products and the epilogue's operations).
Every case asserts max(err / bound) <= 1 and prints it as "DENSE ...".

Shapes follow the kernel's 16 x 16 block rectangle (4 waves x 4 rows): 3x5
is smaller than one rectangle and leaves three waves with nothing to store;
17x18 is 2 x 2 rectangles, ragged by one row and two columns, so halos cross
block borders on both axes; 1x17 has H = 1 (both row halos outside the image)
and two rectangles; N = 2 at 5x6 puts a second image right behind the first.
Every Cin of the trunk (and 256, the widest) runs inside one workspace with
Cout 32 written back into it; Cout 64 goes to a second buffer.
"""
import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(n, h, w, cin, cout, mode, seed):
    """CPU bf16 inputs: (workspace, w_prep, bias, other buffer, res2 source)."""
    g = torch.Generator().manual_seed(seed)
    ld = max(192, cin + 32)

    def nhwc(c):
        t = torch.randn(n, c, h, w, generator=g).bfloat16()
        return t.contiguous(memory_format=torch.channels_last)

    ws = nhwc(ld)
    wp = (torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).bfloat16()
    bias = torch.randn(cout, generator=g)
    bias = bias if mode == "fp32_bias" else bias.bfloat16()
    return ws, wp, (None if mode == "no_bias" else bias), nhwc(ld), nhwc(64)


CASES = [(1, 17, 18, cin, 32, "lrelu") for cin in (64, 96, 128, 160, 192, 256)]
CASES += [
    (1, 3, 5, 64, 32, "lrelu"),
    (1, 1, 17, 96, 32, "fp32_bias"),
    (2, 5, 6, 64, 32, "no_bias"),
    (1, 17, 18, 192, 64, "plain"),
    (2, 9, 13, 192, 64, "alpha_res1_beta"),
    (1, 17, 18, 64, 64, "both_res"),
    (1, 9, 13, 128, 64, "inplace_res"),
]


@pytest.mark.parametrize("n,h,w,cin,cout,mode", CASES)
def test_against_fp64(n, h, w, cin, cout, mode):
    ws, wp, bias, other, r2src = make(n, h, w, cin, cout, mode, 7 * cin + h)
    kw, alpha, beta = {}, 1.0, 1.0
    res1 = res2 = None
    if cout == 32:      # back into the workspace, as conv 1-4 of a block
        dst, c0 = 0, cin
        if mode == "lrelu":
            kw["lrelu"] = 0.2
    else:               # conv 5: into the other buffer
        dst, c0 = 1, 0
        if mode in ("alpha_res1_beta", "both_res"):
            alpha, beta, res1 = 0.04, 0.2, (0, 0)
        if mode == "both_res":
            res2 = (2, 0)
        if mode == "inplace_res":
            alpha, res2 = 0.2, (1, 0)      # exactly out's slice
    bufs = [ws.clone(), other.clone(), r2src.clone()]
    bufs[0][:, cin:] = float("nan")        # unread channels must stay unread
    view = lambda bc: bufs[bc[0]][:, bc[1]:bc[1] + cout]  # noqa: E731
    xf = bufs[0][:, :cin].double()
    r1f = None if res1 is None else view(res1).double()
    r2f = None if res2 is None else view(res2).double()
    wf = wp.double().permute(0, 3, 1, 2)
    bf = torch.zeros(cout).double() if bias is None else bias.double()
    ref = alpha * F.conv2d(xf, wf, bf, padding=1)
    T = abs(alpha) * (F.conv2d(xf.abs(), wf.abs(), None, padding=1)
                      + bf.abs()[None, :, None, None])
    if r1f is not None:
        ref, T = ref + beta * r1f, T + abs(beta) * r1f.abs()
    if r2f is not None:
        ref, T = ref + r2f, T + r2f.abs()
    if "lrelu" in kw:
        ref = F.leaky_relu(ref, kw["lrelu"])
    bound = 2.0 ** -8 * ref.abs() + (9 * cin + 8) * 2.0 ** -23 * T

    dev = [b.to(DEV) for b in bufs]
    dview = lambda bc: dev[bc[0]][:, bc[1]:bc[1] + cout]  # noqa: E731
    x, out = dev[0][:, :cin], dview((dst, c0))
    assert ops.conv3x3_dense_supported(x, wp.to(DEV), out)
    got = ops.conv3x3_dense(
        x, wp.to(DEV), None if bias is None else bias.to(DEV), out,
        alpha=alpha, beta=beta,
        res1=None if res1 is None else dview(res1),
        res2=None if res2 is None else dview(res2), **kw,
    )
    assert got.data_ptr() == out.data_ptr()
    res = [d.cpu() for d in dev]
    y = res[dst][:, c0:c0 + cout]
    assert torch.isfinite(y.float()).all()
    worst = ((y.double() - ref).abs() / bound).max().item()
    print(f"DENSE N={n} {h}x{w} Cin={cin} Cout={cout} {mode} "
          f"err/bound={worst:.3f}")
    assert worst <= 1.0
    # every byte outside the written slice is bit-unchanged
    for i, (before, after) in enumerate(zip(bufs, res)):
        b16, a16 = before.view(torch.int16), after.view(torch.int16)
        if i == dst:
            b16, a16 = b16.clone(), a16.clone()
            b16[:, c0:c0 + cout] = 0
            a16[:, c0:c0 + cout] = 0
        assert torch.equal(b16, a16)


def _bad(name):
    """Arguments of a legal call with one of them broken."""
    buf = torch.zeros(1, 192, 4, 4, dtype=torch.bfloat16, device=DEV)
    buf = buf.contiguous(memory_format=torch.channels_last)
    a = dict(x=buf[:, :64], w_prep=torch.zeros(32, 3, 3, 64, device=DEV,
                                                dtype=torch.bfloat16),
             bias=torch.zeros(32, device=DEV), out=buf[:, 64:96])
    kw = {}
    if name == "x":
        a["x"] = buf[0, :64]
    elif name == "w_prep":
        a["w_prep"] = a["w_prep"][:, :, :, :32]
    elif name == "bias":
        a["bias"] = torch.zeros(31, device=DEV)
    elif name == "out":
        a["out"] = buf[:, 32:64]            # shares channels with x
    elif name == "res1":
        kw["res1"] = buf[:, 96:160]         # 64 channels for a 32-wide out
    elif name == "res2":
        kw["res2"] = buf[:, 80:112]         # partly overlaps out
    elif name == "lrelu":
        kw["lrelu"] = "0.2"
    return a, kw


@pytest.mark.parametrize(
    "name", ["x", "w_prep", "bias", "out", "res1", "res2", "lrelu"])
def test_bad_argument_raises(name):
    a, kw = _bad(name)
    with pytest.raises(ValueError, match=name):
        ops.conv3x3_dense(a["x"], a["w_prep"], a["bias"], a["out"], **kw)
