"""HAT on the CPU: the op's torch route against a per-window loop over token
coordinates, the bias offset table, loading, and the SDWD_UPSCALER_DIR
plumbing."""
import pytest
import torch
from safetensors.torch import save_file

from sdwd_amd import ops
from sdwd_amd.models import registry
from sdwd_amd.models.esrgan import RRDBNet, upscale_image
from sdwd_amd.models.hat import (HAT, hat_from_state_dict,
                                 relative_position_index_oca,
                                 relative_position_index_sa)
from sdwd_amd.models.swinir import SwinIR

INDEX = {16: relative_position_index_sa(), 24: relative_position_index_oca()}


def tiny(seed=0):
    torch.manual_seed(seed)
    net = HAT(16, (2, 1), 2, 2.0, compress_ratio=4, squeeze_factor=8,
              num_feat=8)
    with torch.no_grad():
        for p in net.parameters():
            p.normal_(0, 0.1)
    return net.eval()


@pytest.mark.parametrize("kw,shift", [(16, 8), (24, 0)])
def test_torch_route_equals_window_loop(kw, shift):
    g = torch.Generator().manual_seed(kw)
    b, h, w, heads, d = 2, 32, 48, 2, 6
    qkv = torch.randn(b, h, w, 3, heads, d, generator=g, dtype=torch.float64)
    table = torch.randn((kw + 15) ** 2, heads, generator=g,
                        dtype=torch.float64)
    bias = table[INDEX[kw]].permute(2, 0, 1)            # [heads, 256, kw*kw]
    out = ops.attention_hat(qkv, ops.window_bias_offsets(table, INDEX[kw], kw),
                            0.4, shift, kw)

    def region(r, n):  # of a shifted-frame coordinate
        return 0 if r < n - 16 else (1 if r < n - 8 else 2)

    pad = (kw - 16) // 2
    zero = torch.zeros(b, 1, 3, heads, d, dtype=torch.float64)
    want = torch.empty(b, h, w, heads * d, dtype=torch.float64)
    for wy in range(h // 16):
        for wx in range(w // 16):
            qs = [(16 * wy + i, 16 * wx + j)
                  for i in range(16) for j in range(16)]
            ks = [(16 * wy - pad + i, 16 * wx - pad + j)
                  for i in range(kw) for j in range(kw)]
            gy = [(y + shift) % h for y, _ in qs]
            gx = [(x + shift) % w for _, x in qs]
            q = qkv[:, gy, gx, 0].transpose(1, 2)       # [b, heads, 256, d]
            if kw == 16:
                kv = qkv[:, gy, gx]
            else:                   # out-of-grid keys are present and zero
                kv = torch.cat([qkv[:, y, x][:, None] if 0 <= y < h
                                and 0 <= x < w else zero for y, x in ks], 1)
            k, v = kv[:, :, 1].transpose(1, 2), kv[:, :, 2].transpose(1, 2)
            s = 0.4 * q @ k.transpose(-2, -1) + bias
            if shift:
                reg = torch.tensor([3 * region(y, h) + region(x, w)
                                    for y, x in qs])
                s = s - 100.0 * (reg[:, None] != reg[None, :])
            o = torch.softmax(s, -1) @ v
            want[:, gy, gx] = o.transpose(1, 2).reshape(b, 256, heads * d)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match="multiple of the window"):
        ops.attention_hat(qkv[:, :24], bias, 0.4, shift, kw)


@pytest.mark.parametrize("kw", [16, 24])
def test_window_bias_offsets(kw):
    index = INDEX[kw]
    assert (kw == 24) == bool((index < 0).any())        # OCA's wrap around
    table = torch.randn((kw + 15) ** 2, 3, dtype=torch.float64)
    off = ops.window_bias_offsets(table, index, kw)
    assert off.shape == (3, kw + 15, kw + 15)
    q, k = torch.arange(16), torch.arange(kw)
    d = k[None, :] - q[:, None] + 15                    # [16, kw]
    expand = off[:, d[:, None, :, None], d[None, :, None, :]]
    assert torch.equal(expand.reshape(3, 256, kw * kw),
                       table[index].permute(2, 0, 1))
    bad = index.clone()
    bad[37, 101] = (bad[37, 101] + 1) % table.shape[0]
    with pytest.raises(ValueError, match="not translation invariant"):
        ops.window_bias_offsets(table, bad, kw)


def test_state_dict_round_trip_and_dispatch(tmp_path, monkeypatch):
    net = tiny()
    sd = {f"params_ema.{k}": v.clone() for k, v in net.state_dict().items()}
    # the stored buffers are the authority: a mirrored table and index give
    # the same network only if the loader keeps the file's index
    sd["params_ema.relative_position_index_SA"] = 960 - INDEX[16]
    blk = "params_ema.layers.0.residual_group.blocks.1."
    sd[blk + "attn_mask"] = torch.zeros(4, 256, 256)
    got = hat_from_state_dict(sd)
    assert (got.embed_dim, got.depths, got.num_heads, got.mlp_hidden,
            got.compress_ratio, got.squeeze_factor) == (16, (2, 1), 2, 32, 4, 8)
    x = torch.rand(1, 3, 20, 27)
    with torch.no_grad():
        for m in net.modules():
            if getattr(m, "kw", None) == 16:
                m.relative_position_bias_table.copy_(
                    m.relative_position_bias_table.flip(0))
        out = got(x)
        assert out.shape == (1, 3, 80, 108)
        assert torch.allclose(out, net(x), rtol=0, atol=1e-6)
    plain = {k[len("params_ema."):]: v for k, v in sd.items()
             if not k.endswith("attn_mask")}
    x2 = {k: v for k, v in plain.items() if k != "upsample.2.weight"}
    with pytest.raises(ValueError, match="Not supported: 2x / 3x"):
        hat_from_state_dict(x2)

    monkeypatch.setenv("SDWD_UPSCALER_DIR", str(tmp_path))
    registry.clear_cache()
    save_file({k: v.contiguous() for k, v in plain.items()},
              str(tmp_path / "HAT_4x.safetensors"))
    save_file(SwinIR(16, (1,), 2, num_feat=8).state_dict(),
              str(tmp_path / "SwinIR_4x.safetensors"))
    save_file(RRDBNet(nf=8, gc=4, nb=1).state_dict(),
              str(tmp_path / "ESRGAN_4x.safetensors"))
    hat = registry.load_upscaler("hat_4x")
    assert isinstance(hat, HAT)
    assert isinstance(registry.load_upscaler("swinir_4x"), SwinIR)
    assert isinstance(registry.load_upscaler("esrgan_4x"), RRDBNet)
    up = upscale_image(hat, x)
    assert up.shape == (1, 3, 80, 108)
    assert torch.allclose(up, out.clamp(0, 1), rtol=0, atol=1e-6)
    registry.clear_cache()
