"""models/scunet.py on the CPU: the plain route against an independent literal
implementation written here (einsum attention over partitioned windows,
masked_fill_(-inf), F.conv_transpose2d), and the loader."""
import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import save_file

from sdwd_amd.models.hat import is_hat_state_dict
from sdwd_amd.models.scunet import (SCUNet, is_scunet_state_dict, load_scunet,
                                    scunet_from_state_dict)
from sdwd_amd.models.swinir import is_swinir_state_dict


def small_model(seed=0):
    net = SCUNet(config=[1] * 7, dim=64).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(("ln1.weight", "ln2.weight")):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                fan = p[0].numel() if p.dim() > 1 else 16
                p.copy_(torch.randn(p.shape, generator=g) * fan ** -0.5)
    return net


def wmsa(sd, pre, x, shift):
    b, h, w, c = x.shape
    heads = c // 32
    if shift:
        x = torch.roll(x, (-4, -4), (1, 2))
    hw, ww = h // 8, w // 8
    x = x.view(b, hw, 8, ww, 8, c).transpose(2, 3).reshape(b, hw * ww, 64, c)
    qkv = F.linear(x, sd[pre + "embedding_layer.weight"],
                   sd[pre + "embedding_layer.bias"])
    q, k, v = qkv.view(b, hw * ww, 64, 3 * heads, 32).permute(3, 0, 1, 2, 4) \
        .chunk(3, dim=0)
    sim = torch.einsum("hbwpc,hbwqc->hbwpq", q, k) * 32 ** -0.5
    cord = torch.tensor([[i, j] for i in range(8) for j in range(8)])
    rel = cord[:, None, :] - cord[None, :, :] + 7
    sim = sim + sd[pre + "relative_position_params"][
        :, rel[..., 0], rel[..., 1]][:, None, None]
    if shift:
        m = torch.zeros(hw, ww, 8, 8, 8, 8, dtype=torch.bool)
        m[-1, :, :4, :, 4:, :] = True
        m[-1, :, 4:, :, :4, :] = True
        m[:, -1, :, :4, :, 4:] = True
        m[:, -1, :, 4:, :, :4] = True
        sim.masked_fill_(m.view(1, 1, hw * ww, 64, 64), float("-inf"))
    out = torch.einsum("hbwij,hbwjc->hbwic", sim.softmax(-1), v)
    out = out.permute(1, 2, 3, 0, 4).reshape(b, hw * ww, 64, c)
    out = F.linear(out, sd[pre + "linear.weight"], sd[pre + "linear.bias"])
    out = out.view(b, hw, ww, 8, 8, c).transpose(2, 3).reshape(b, h, w, c)
    return torch.roll(out, (4, 4), (1, 2)) if shift else out


def literal(sd, x, config):
    def block(pre, x, shift):
        c = x.shape[1] // 2
        a = F.conv2d(x, sd[pre + "conv1_1.weight"], sd[pre + "conv1_1.bias"])
        cx, tx = a[:, :c], a[:, c:].permute(0, 2, 3, 1)
        cx = cx + F.conv2d(F.relu(F.conv2d(cx, sd[pre + "conv_block.0.weight"],
                                           padding=1)),
                           sd[pre + "conv_block.2.weight"], padding=1)
        t = pre + "trans_block."

        def ln(n, v):
            return F.layer_norm(v, (c,), sd[t + n + ".weight"],
                                sd[t + n + ".bias"])

        tx = tx + wmsa(sd, t + "msa.", ln("ln1", tx), shift)
        hid = F.gelu(F.linear(ln("ln2", tx), sd[t + "mlp.0.weight"],
                              sd[t + "mlp.0.bias"]))
        tx = tx + F.linear(hid, sd[t + "mlp.2.weight"], sd[t + "mlp.2.bias"])
        res = torch.cat((cx, tx.permute(0, 3, 1, 2)), 1)
        return x + F.conv2d(res, sd[pre + "conv1_2.weight"],
                            sd[pre + "conv1_2.bias"])

    def stage(name, x, n, kind):
        if kind == "up":
            x = F.conv_transpose2d(x, sd[f"{name}.0.weight"], stride=2)
        for i in range(n):
            x = block(f"{name}.{i + (kind == 'up')}.", x, 4 * (i % 2))
        if kind == "down":
            x = F.conv2d(x, sd[f"{name}.{n}.weight"], stride=2)
        return x

    h, w = x.shape[2:]
    x = F.pad(x, (0, -w % 64, 0, -h % 64), mode="replicate")
    x1 = F.conv2d(x, sd["m_head.0.weight"], padding=1)
    x2 = stage("m_down1", x1, config[0], "down")
    x3 = stage("m_down2", x2, config[1], "down")
    x4 = stage("m_down3", x3, config[2], "down")
    x = stage("m_body", x4, config[3], "body")
    x = stage("m_up3", x + x4, config[4], "up")
    x = stage("m_up2", x + x3, config[5], "up")
    x = stage("m_up1", x + x2, config[6], "up")
    return F.conv2d(x + x1, sd["m_tail.0.weight"], padding=1)[:, :, :h, :w]


@pytest.mark.parametrize("config", [[1] * 7, [2, 1, 1, 1, 1, 1, 2]])
def test_plain_route_matches_literal(config):
    net = small_model()
    if config != [1] * 7:
        net = SCUNet(config=config, dim=64).eval()
        torch.manual_seed(1)
        for p in net.parameters():
            torch.nn.init.normal_(p, std=0.05)
    x = torch.rand(1, 3, 72, 100, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        out = net(x)
        ref = literal(net.state_dict(), x, config)
    assert out.shape == x.shape
    assert (out - ref).abs().max() <= 1e-4 * (1 + ref.abs().max())


def test_load_round_trip_and_detection(tmp_path):
    net = SCUNet(config=[1, 2, 1, 1, 1, 2, 1], dim=64)
    path = str(tmp_path / "scunet.safetensors")
    save_file({k: v.contiguous() for k, v in net.state_dict().items()}, path)
    back = load_scunet(path)
    assert back.config == (1, 2, 1, 1, 1, 2, 1) and back.dim == 64
    keys = list(net.state_dict())
    assert is_scunet_state_dict(keys)
    assert not is_swinir_state_dict(keys) and not is_hat_state_dict(keys)
    swin = ["conv_first.weight",
            "layers.0.residual_group.blocks.0.attn.qkv.weight"]
    hat = swin + ["layers.0.residual_group.overlap_attn.qkv.weight",
                  "layers.0.residual_group.blocks.0.conv_block.cab.0.weight"]
    rrdb = ["conv_first.weight", "body.0.rdb1.conv1.weight"]
    assert not any(is_scunet_state_dict(k) for k in (swin, hat, rrdb))


@pytest.mark.parametrize("rel_shape", [(2, 15, 15), (1, 13, 13)])
def test_other_head_dim_or_window_is_refused(rel_shape):
    sd = dict(SCUNet(config=[1] * 7, dim=64).state_dict())
    sd["m_down1.0.trans_block.msa.relative_position_params"] = \
        torch.zeros(rel_shape)
    with pytest.raises(ValueError, match="supported: SCUNet"):
        scunet_from_state_dict(sd)
