"""Compact Real-ESRGAN upscalers (SRVGGNetCompact) on the CPU: the module
against the network written out with functional calls, loading under both key
prefixes, the registry route, the loader's rejections, and the CPU route of
ops.conv_compact."""
import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import save_file

NF = 64


def compact_state(num_conv=2, nf=NF, scale=4, seed=0, prelu=True):
    """Real-ESRGAN's SRVGGNetCompact state dict, fp32."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    widths = [3] + [nf] * (num_conv + 1) + [3 * scale * scale]
    for i, (cin, cout) in enumerate(zip(widths, widths[1:])):
        sd[f"body.{2 * i}.weight"] = torch.randn(
            cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
        sd[f"body.{2 * i}.bias"] = torch.randn(cout, generator=g) * 0.1
        if prelu and i <= num_conv:
            sd[f"body.{2 * i + 1}.weight"] = torch.randn(nf, generator=g) * 0.3
    return sd


def compact_reference(sd, x, scale=4):
    last = max(int(k.split(".")[1]) for k in sd)
    out = x
    for k in range(0, last + 1, 2):
        out = F.conv2d(out, sd[f"body.{k}.weight"], sd[f"body.{k}.bias"],
                       padding=1)
        if k < last:
            out = F.prelu(out, sd[f"body.{k + 1}.weight"])
    return F.pixel_shuffle(out, scale) + F.interpolate(x, scale_factor=scale)


@pytest.mark.parametrize("prefix", ["", "params.", "params_ema."])
def test_file_round_trip_matches_reference(tmp_path, prefix):
    from sdwd_amd.models.esrgan import SRVGGNetCompact, load_esrgan

    sd = compact_state(num_conv=3)
    path = str(tmp_path / "c.safetensors")
    save_file({prefix + k: v for k, v in sd.items()}, path)
    net = load_esrgan(path)
    assert isinstance(net, SRVGGNetCompact)
    assert (net.nf, net.num_conv, net.scale) == (NF, 3, 4)
    x = torch.rand(2, 3, 7, 9, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        out = net(x)
    assert out.shape == (2, 3, 28, 36)
    assert torch.allclose(out, compact_reference(sd, x), rtol=1e-5, atol=1e-6)


def test_load_upscaler_returns_a_compact_model(tmp_path, monkeypatch):
    from sdwd_amd.models import registry
    from sdwd_amd.models.esrgan import SRVGGNetCompact

    monkeypatch.setenv("SDWD_UPSCALER_DIR", str(tmp_path))
    registry.clear_cache()
    save_file(compact_state(num_conv=1),
              str(tmp_path / "General-4xV3.safetensors"))
    net = registry.load_upscaler("general-4xv3")
    assert isinstance(net, SRVGGNetCompact) and net.num_conv == 1
    registry.clear_cache()


@pytest.mark.parametrize("breakage", ["scale2", "nf32", "relu", "stray_key"])
def test_unsupported_compact_model_raises(tmp_path, breakage):
    from sdwd_amd.models.esrgan import load_esrgan

    sd = compact_state(
        num_conv=1, scale=2 if breakage == "scale2" else 4,
        nf=32 if breakage == "nf32" else NF, prelu=breakage != "relu")
    if breakage == "stray_key":
        sd["upsampler.weight"] = torch.zeros(1)
    path = str(tmp_path / "m.safetensors")
    save_file(sd, path)
    with pytest.raises(ValueError, match="supported"):
        load_esrgan(path)


@pytest.mark.parametrize("variant", ["prelu", "pre_act", "shuffle"])
def test_conv_compact_cpu_route_matches_formula(variant):
    from sdwd_amd import ops

    g = torch.Generator().manual_seed(4)
    cout = 48 if variant == "shuffle" else NF
    x = torch.randn(2, NF, 5, 6, generator=g)
    w = torch.randn(cout, NF, 3, 3, generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    slope = torch.randn(NF, generator=g)
    pre = torch.randn(NF, generator=g)
    base = torch.rand(2, 3, 5, 6, generator=g)
    wp = w.permute(0, 2, 3, 1).contiguous()
    if variant == "shuffle":
        got = ops.conv_compact(x, wp, b, shuffle_base=base)
        want = F.pixel_shuffle(F.conv2d(x, w, b, padding=1), 4) + (
            F.interpolate(base, scale_factor=4))
    else:
        p = pre if variant == "pre_act" else None
        got = ops.conv_compact(x, wp, b, slope=slope, pre_slope=p)
        xin = x if p is None else F.prelu(x, p)
        want = F.prelu(F.conv2d(xin, w, b, padding=1), slope)
    assert got.shape == want.shape
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError, match="slope"):
        ops.conv_compact(x, wp, b)
