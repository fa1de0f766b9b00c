"""RRDBNet on the GPU: the native route (trunk on conv3x3_dense_bf16_kernel)
against the fp64 run of the same bf16 weights.

The end-to-end tolerance cannot be derived through 30-odd roundings, so it is
measured against the reference route: the native error may be at most twice
the error of the native=False bf16 route on the same input. The factor 2
allows for a different but equally valid rounding order (the fused
third-block residual rounds once where the composed route rounds twice).
Prints both errors as "ESRGAN ...".
"""
import copy

import pytest
import torch

from sdwd_amd.models.esrgan import RRDBNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_native_against_fp64_and_composed():
    torch.manual_seed(3)
    net = RRDBNet(nf=64, gc=32, nb=2).eval()
    net = net.to(torch.bfloat16)                    # the weights under test
    x = torch.rand(2, 3, 20, 24).bfloat16()
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(x.double())
        gpu = copy.deepcopy(net).to(DEV)
        assert gpu.native_supported(x.to(DEV))
        native = gpu(x.to(DEV)).cpu()
        again = gpu(x.to(DEV)).cpu()
        composed = gpu(x.to(DEV), native=False).cpu()
    assert native.shape == (2, 3, 80, 96) and native.dtype == torch.bfloat16
    assert torch.equal(native, again)               # no atomics
    err_native = (native.double() - ref).abs().max().item()
    err_composed = (composed.double() - ref).abs().max().item()
    print(f"ESRGAN nb=2 2x3x20x24 max|ref|={ref.abs().max().item():.4f} "
          f"native_err={err_native:.3e} composed_err={err_composed:.3e}")
    assert err_native <= 2.0 * err_composed
