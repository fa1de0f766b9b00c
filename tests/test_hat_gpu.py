"""HAT on the GPU: the native route (both attentions on hat_attn_bf16_kernel,
tokens kept [B, H, W, C]) against the fp64 run of the same bf16 weights.

As in tests/test_swinir_gpu.py the end-to-end tolerance is measured, not
fixed: the native error may be at most twice the error of the native=False
bf16 route on the same input (an equally valid different rounding order).
Prints both errors as "HAT ...".
"""
import copy

import pytest
import torch

from sdwd_amd.models.hat import HAT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("embed,heads,compress,squeeze", [(180, 6, 3, 30),
                                                          (144, 6, 24, 24)])
def test_native_against_fp64_and_plain(embed, heads, compress, squeeze):
    torch.manual_seed(embed)
    net = HAT(embed, (2, 2), heads, 2.0, compress, squeeze).eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.normal_(0, 1)                     # std 1: the bias matters
    net = net.to(torch.bfloat16)                    # the weights under test
    x = torch.rand(2, 3, 20, 27).bfloat16()         # reflect-padded to 32x32
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(x.double())
        gpu = copy.deepcopy(net).to(DEV)
        assert gpu.native_supported(x.to(DEV))
        native = gpu(x.to(DEV)).cpu()
        plain = gpu(x.to(DEV), native=False).cpu()
    assert native.shape == (2, 3, 80, 108) and native.dtype == torch.bfloat16
    err_native = (native.double() - ref).abs().max().item()
    err_plain = (plain.double() - ref).abs().max().item()
    print(f"HAT embed={embed} heads={heads} 2x3x20x27 "
          f"max|ref|={ref.abs().max().item():.4f} "
          f"native_err={err_native:.3e} plain_err={err_plain:.3e}")
    assert err_native <= 2.0 * err_plain
