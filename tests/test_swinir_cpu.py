"""SwinIR on the CPU: the op's torch route against a per-window loop, the
zero-padded head rows, loading, and the SDWD_UPSCALER_DIR plumbing."""
import pytest
import torch
from safetensors.torch import save_file

from sdwd_amd import ops
from sdwd_amd.models import registry
from sdwd_amd.models.esrgan import RRDBNet
from sdwd_amd.models.swinir import (SwinIR, WindowAttention, load_swinir,
                                    relative_position_index,
                                    swinir_from_state_dict)


def tiny_state(seed=0, **kw):
    """BasicSR-named SwinIR state dict (embed 16, 2 heads, depths [2, 1])
    under params_ema., with the stored mask and index buffers."""
    torch.manual_seed(seed)
    cfg = dict(embed_dim=16, depths=(2, 1), num_heads=2, mlp_ratio=2.0,
               resi_connection="1conv", num_feat=8)
    cfg.update(kw)
    net = SwinIR(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.normal_(0, 0.1)
    sd = {f"params_ema.{k}": v for k, v in net.state_dict().items()}
    blk = "params_ema.layers.0.residual_group.blocks.1."
    sd[blk + "attn_mask"] = torch.zeros(64, 64, 64)
    sd[blk + "attn.relative_position_index"] = relative_position_index()
    return net, sd


@pytest.mark.parametrize("shift", [0, 4])
def test_torch_route_equals_window_loop(shift):
    g = torch.Generator().manual_seed(shift)
    b, h, w, heads, d = 2, 16, 24, 2, 6
    qkv = torch.randn(b, h, w, 3, heads, d, generator=g, dtype=torch.float64)
    bias = torch.randn(heads, 64, 64, generator=g, dtype=torch.float64)
    out = ops.attention_swin(qkv, bias, 0.4, shift)

    def region(r, n):  # of a shifted-frame coordinate
        return 0 if r < n - 8 else (1 if r < n - 4 else 2)

    want = torch.empty(b, h, w, heads * d, dtype=torch.float64)
    for wy in range(h // 8):
        for wx in range(w // 8):
            ys = [8 * wy + i for i in range(8) for _ in range(8)]
            xs = [8 * wx + j for _ in range(8) for j in range(8)]
            reg = torch.tensor([3 * region(y, h) + region(x, w)
                                for y, x in zip(ys, xs)])
            gy = [(y + shift) % h for y in ys]
            gx = [(x + shift) % w for x in xs]
            q, k, v = qkv[:, gy, gx].permute(2, 0, 3, 1, 4)  # [b, heads, 64, d]
            s = 0.4 * q @ k.transpose(-2, -1) + bias
            if shift:
                s = s - 100.0 * (reg[:, None] != reg[None, :])
            o = torch.softmax(s, -1) @ v
            want[:, gy, gx] = o.transpose(1, 2).reshape(b, 64, heads * d)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match="multiple of the window"):
        ops.attention_swin(qkv[:, :12], bias, 0.4, shift)


def test_padded_heads_equal_stored_heads():
    torch.manual_seed(1)
    att = WindowAttention(60, 2).double()           # head dim 30 -> 32
    with torch.no_grad():
        att.relative_position_bias_table.normal_()
    x = torch.randn(1, 8, 16, 60, dtype=torch.float64)
    with torch.no_grad():
        wide = att(x, 4, padded=True, native=False)
        stored = att(x, 4, padded=False, native=False)
    assert att.prepared()[0].shape == (3 * 2 * 32, 60)
    assert att.prepared()[3].dtype == torch.float32
    # the gathered bias is held in fp32 for the kernel: 2^-24 relative
    assert torch.allclose(wide, stored, rtol=0, atol=1e-6)


def test_state_dict_round_trip_and_unsupported(tmp_path):
    net, sd = tiny_state(resi_connection="3conv", depths=(2, 1, 2))
    got = swinir_from_state_dict(sd)
    assert (got.embed_dim, got.depths, got.num_heads, got.mlp_hidden,
            got.resi_connection) == (16, (2, 1, 2), 2, 32, "3conv")
    x = torch.rand(1, 3, 10, 13)
    with torch.no_grad():
        out = got(x)
        assert out.shape == (1, 3, 40, 52)
        assert torch.equal(out, net.eval()(x))
    plain = {k[len("params_ema."):]: v for k, v in sd.items()}
    shuffle = {k: v for k, v in plain.items() if not k.startswith("conv_up")}
    shuffle["upsample.0.weight"] = torch.zeros(32, 8, 3, 3)
    window7 = dict(plain)
    for k in plain:
        if k.endswith("relative_position_bias_table"):
            window7[k] = torch.zeros(13 * 13, 2)
    for bad in (shuffle, window7):
        with pytest.raises(ValueError, match="Not supported: pixelshuffle"):
            swinir_from_state_dict(bad)
    save_file(plain, str(tmp_path / "m.safetensors"))
    assert load_swinir(str(tmp_path / "m.safetensors")).depths == (2, 1, 2)


def test_upscaler_dir_dispatch_and_hires_fix(tmp_path, monkeypatch):
    from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

    monkeypatch.setenv("SDWD_UPSCALER_DIR", str(tmp_path))
    registry.clear_cache()
    _, sd = tiny_state()
    save_file(sd, str(tmp_path / "SwinIR_4x.safetensors"))
    save_file(RRDBNet(nf=8, gc=4, nb=1).state_dict(),
              str(tmp_path / "ESRGAN_4x.safetensors"))
    assert isinstance(registry.load_upscaler("swinir_4x"), SwinIR)
    assert isinstance(registry.load_upscaler("esrgan_4x"), RRDBNet)

    pipe = StableDiffusionPipeline("tiny", device="cpu")

    def run(name):
        return pipe.generate(PipelineRequest(
            prompt="hr px", steps=2, width=64, height=64, seeds=[8],
            enable_hr=True, hr_scale=2.0, hr_steps=2, denoising_strength=0.6,
            hr_upscaler=name,
        )).images

    model, fallback = run("SwinIR_4x"), run("SwinIR_8x")
    assert model.shape == fallback.shape == (1, 128, 128, 3)
    assert not torch.equal(model, fallback)
    registry.clear_cache()
