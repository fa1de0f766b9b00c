"""ESRGAN upscalers on the CPU: loading under both key namings, the module
against an RRDBNet written out here, and the SDWD_UPSCALER_DIR plumbing
(hires fix, /sdapi/v1/upscalers)."""
import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import save_file

NF, GC, NB = 8, 4, 2


def tiny_state(seed=0):
    """A new-arch RRDBNet state dict (nf 8, gc 4, nb 2), fp32."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cin, cout):
        sd[f"{name}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) / (
            3 * cin ** 0.5)
        sd[f"{name}.bias"] = torch.randn(cout, generator=g) * 0.1

    conv("conv_first", 3, NF)
    for n in range(NB):
        for k in (1, 2, 3):
            for j in range(1, 5):
                conv(f"body.{n}.rdb{k}.conv{j}", NF + (j - 1) * GC, GC)
            conv(f"body.{n}.rdb{k}.conv5", NF + 4 * GC, NF)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, NF, NF)
    conv("conv_last", NF, 3)
    return sd


def old_names(sd):
    fixed = {"conv_first": "model.0", "conv_body": f"model.1.sub.{NB}",
             "conv_up1": "model.3", "conv_up2": "model.6",
             "conv_hr": "model.8", "conv_last": "model.10"}
    out = {}
    for key, val in sd.items():
        stem, leaf = key.rsplit(".", 1)
        if stem in fixed:
            out[f"{fixed[stem]}.{leaf}"] = val
        else:
            _, n, rdb, conv = stem.split(".")
            out[f"model.1.sub.{n}.RDB{rdb[3:]}.{conv}.0.{leaf}"] = val
    return out


def rrdbnet_reference(sd, x):
    def conv(name, t):
        return F.conv2d(t, sd[f"{name}.weight"], sd[f"{name}.bias"], padding=1)

    def lrelu(t):
        return F.leaky_relu(t, 0.2)

    feat = conv("conv_first", x)
    body = feat
    for n in range(NB):
        rrdb_in = body
        for k in (1, 2, 3):
            p = f"body.{n}.rdb{k}"
            x1 = lrelu(conv(f"{p}.conv1", body))
            x2 = lrelu(conv(f"{p}.conv2", torch.cat([body, x1], 1)))
            x3 = lrelu(conv(f"{p}.conv3", torch.cat([body, x1, x2], 1)))
            x4 = lrelu(conv(f"{p}.conv4", torch.cat([body, x1, x2, x3], 1)))
            x5 = conv(f"{p}.conv5", torch.cat([body, x1, x2, x3, x4], 1))
            body = x5 * 0.2 + body
        body = body * 0.2 + rrdb_in
    feat = feat + conv("conv_body", body)
    feat = lrelu(conv("conv_up1", F.interpolate(feat, scale_factor=2)))
    feat = lrelu(conv("conv_up2", F.interpolate(feat, scale_factor=2)))
    return conv("conv_last", lrelu(conv("conv_hr", feat)))


def test_both_key_namings_load_and_match_reference(tmp_path):
    from sdwd_amd.models.esrgan import load_esrgan

    sd = tiny_state()
    save_file(sd, str(tmp_path / "new.safetensors"))
    save_file(old_names(sd), str(tmp_path / "old.safetensors"))
    new = load_esrgan(str(tmp_path / "new.safetensors"))
    old = load_esrgan(str(tmp_path / "old.safetensors"))
    assert (new.nf, new.gc, new.nb) == (old.nf, old.gc, old.nb) == (NF, GC, NB)
    a, b = new.state_dict(), old.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    x = torch.rand(1, 3, 12, 10, generator=torch.Generator().manual_seed(1))
    ref = rrdbnet_reference(sd, x)
    with torch.no_grad():
        for net in (new, old):
            out = net(x)
            assert out.shape == (1, 3, 48, 40)
            assert torch.allclose(out, ref, rtol=1e-5, atol=1e-6)


def test_dense_op_composed_route_matches_formula():
    # the CPU route of ops.conv3x3_dense: channel slices of one workspace
    from sdwd_amd import ops

    g = torch.Generator().manual_seed(2)
    ws = torch.randn(1, 48, 6, 7, generator=g).contiguous(
        memory_format=torch.channels_last)
    w = torch.randn(8, 16, 3, 3, generator=g) * 0.1
    b = torch.randn(8, generator=g)
    want = F.leaky_relu(
        0.5 * F.conv2d(ws[:, :16], w, b, padding=1) + 2.0 * ws[:, 24:32]
        + ws[:, 16:24], 0.2)
    keep = ws.clone()
    ops.conv3x3_dense(ws[:, :16], w.permute(0, 2, 3, 1).contiguous(), b,
                      ws[:, 16:24], alpha=0.5, res1=ws[:, 24:32], beta=2.0,
                      res2=ws[:, 16:24], lrelu=0.2)
    assert torch.allclose(ws[:, 16:24], want, rtol=1e-5, atol=1e-6)
    assert torch.equal(ws[:, :16], keep[:, :16])
    assert torch.equal(ws[:, 24:], keep[:, 24:])


@pytest.mark.parametrize("breakage", ["unknown_key", "unshuffle", "suffix"])
def test_unsupported_layout_raises(tmp_path, breakage):
    from sdwd_amd.models.esrgan import load_esrgan

    sd = tiny_state()
    path = tmp_path / ("m.pth" if breakage == "suffix" else "m.safetensors")
    if breakage == "unknown_key":
        sd = {"layers.0.attn.qkv.weight": torch.zeros(4, 4)}
    elif breakage == "unshuffle":
        sd["conv_first.weight"] = torch.zeros(NF, 12, 3, 3)
    save_file(sd, str(path))
    with pytest.raises(ValueError, match="supported"):
        load_esrgan(str(path))


def test_hires_fix_and_listing_use_the_directory(tmp_path, monkeypatch):
    from sdwd_amd.models import registry
    from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

    monkeypatch.setenv("SDWD_UPSCALER_DIR", str(tmp_path))
    registry.clear_cache()
    pipe = StableDiffusionPipeline("tiny", device="cpu")

    def run():
        return pipe.generate(PipelineRequest(
            prompt="hr px", steps=2, width=64, height=64, seeds=[8],
            enable_hr=True, hr_scale=2.0, hr_steps=2, denoising_strength=0.6,
            hr_upscaler="tiny-esrgan 4X",
        )).images

    fallback = run()                      # nothing in the directory: bicubic
    save_file(tiny_state(), str(tmp_path / "Tiny-ESRGAN 4x.safetensors"))
    model = run()                         # matched case-insensitively
    assert model.shape == fallback.shape == (1, 128, 128, 3)
    assert not torch.equal(model, fallback)

    from fastapi.testclient import TestClient

    from sdwd_amd.api.server import create_app
    from sdwd_amd.parallel.engine import LocalEngine

    client = TestClient(create_app(LocalEngine(model="tiny", devices=["cpu"])))
    ups = client.get("/sdapi/v1/upscalers").json()
    assert [u["name"] for u in ups[:5]] == ["None", "Nearest", "Bilinear",
                                            "Bicubic", "Lanczos"]
    assert ups[5:] == [{
        "name": "Tiny-ESRGAN 4x", "model_name": "Tiny-ESRGAN 4x",
        "model_path": str(tmp_path / "Tiny-ESRGAN 4x.safetensors"),
        "scale": 4,
    }]
    monkeypatch.setenv("SDWD_UPSCALER_DIR", str(tmp_path / "missing"))
    assert len(client.get("/sdapi/v1/upscalers").json()) == 5
