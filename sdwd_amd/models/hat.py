"""HAT upscalers (hybrid attention transformer), the 4x pixelshuffle
real-world configurations: embed 180 / 6 heads / window 16 with 6 or 12
residual groups of 6 blocks (HAT, HAT-L) and the embed-144 HAT-S, head dim
30 or 24.

The network is conv_first, a LayerNorm over the token grid, residual hybrid
attention groups (RHAG: hybrid attention blocks with a shift of 0 and 8 in
turn, one overlapping cross-attention block, a conv and the group's
residual), a final norm, conv_after_body plus the skip, and a 64-channel
pixel-shuffle tail. A hybrid attention block (HAB) adds window-16
self-attention and 0.01 x a channel-attention conv block (CAB) of the same
normed input to the residual, then the MLP. The overlapping block (OCAB)
lets each 16 x 16 query window attend to the 24 x 24 key patch centred on it.

On a bf16 GPU the tokens stay one [B, H, W, C] tensor. Both attentions run on
ops.attention_hat (hat_attn_bf16_kernel, kw 16 and 24) over the QKV GEMM's
output viewed as [B, H, W, 3, heads, 32], with the relative-position bias as
the [heads, kw+15, kw+15] offset table of ops.window_bias_offsets; nothing is
rolled, partitioned, unfolded or masked. The MLPs run on ops.swin_mlp with
the next norm fused, the convs at the embed width (a CAB's two convs, the
group conv, conv_after_body, conv_before_upsample) on ops.conv_ragged, the
tail on the 64-channel convs. A HAB's channel attention, its three-way
residual sum and norm2 run on ops.channel_gate and ops.gated_add_layer_norm
(hab_tail.hip), the OCAB's residual + norm2 on ops.add_layer_norm. Head rows
are zero-padded to 32 once per weight version exactly as models/swinir.py
does. The QKV and proj GEMMs, the CAB's GELU and pixel_shuffle stay on the
library (TODO.md, "HAT").
"""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .esrgan import MAX_INPUT_PIXELS
from .layers import FusedLayerNorm, _fp32_cached
from .swinir import (RGB_MEAN, Mlp, SwinIR, _conv, _nchw, _PatchEmbed,
                     _tokens)

WINDOW = ops.HAT_WINDOW
OVERLAP = WINDOW * 3 // 2          # overlap_ratio 0.5: 24 x 24 key patches
DPAD = ops.SWIN_DPAD
CONV_SCALE = 0.01

_SUPPORTED = (
    "supported: 4x HAT .safetensors with the pixelshuffle upsampler "
    "(conv_before_upsample, upsample.0, upsample.2, conv_last), window 16, "
    "overlap ratio 0.5, head dim <= 32, 1conv residual connections, "
    "3-channel input (HAT, HAT-L and HAT-S x4). Not supported: 2x / 3x "
    "tails, other windows, 3conv, head dims above 32, DAT"
)


def _grid(n: int) -> torch.Tensor:
    """[2, n*n] (row, column) of an n x n window, row-major."""
    return torch.stack(torch.meshgrid(torch.arange(n), torch.arange(n),
                                      indexing="ij")).flatten(1)


def relative_position_index_sa() -> torch.Tensor:
    """[256, 256] index of (query, key) into the (31 * 31)-row table of a
    HAB: Swin's formula at window 16."""
    c = _grid(WINDOW)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (WINDOW - 1)
    return rel[:, :, 0] * (2 * WINDOW - 1) + rel[:, :, 1]


def relative_position_index_oca() -> torch.Tensor:
    """[256, 576] index of (query, key of the 24 x 24 patch) into the
    (39 * 39)-row table of an OCAB. The published offset, 16 - 24 + 1 per
    axis, makes part of the entries negative: they address the table from
    its end."""
    ori, ext = _grid(WINDOW), _grid(OVERLAP)
    rel = (ext[:, None, :] - ori[:, :, None]).permute(1, 2, 0)
    rel = rel + (WINDOW - OVERLAP + 1)
    return rel[:, :, 0] * (WINDOW + OVERLAP - 1) + rel[:, :, 1]


class HatAttention(nn.Module):
    """qkv, the bias table and proj of a HAB (kw 16) or an OCAB (kw 24)."""

    def __init__(self, dim: int, heads: int, kw: int):
        super().__init__()
        self.dim, self.heads, self.hd, self.kw = dim, heads, dim // heads, kw
        self.scale = self.hd ** -0.5
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((WINDOW + kw - 1) ** 2, heads))
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self._prep_cache = None

    def prepared(self, index: torch.Tensor):
        """(qkv weight [3*heads*32, dim], qkv bias, proj weight
        [dim, heads*32], bias offsets [heads, kw+15, kw+15] in the table's
        dtype, the same in fp32), rebuilt when a source tensor changes (like
        swinir.WindowAttention.prepared)."""
        src = (self.qkv.weight, self.qkv.bias, self.proj.weight,
               self.relative_position_bias_table, index)
        key = tuple((t.data_ptr(), t._version, t.dtype) for t in src)
        if self._prep_cache is None or self._prep_cache[0] != key:
            with torch.no_grad():
                h, hd, dim = self.heads, self.hd, self.dim
                wq = self.qkv.weight.view(3, h, hd, dim)
                bq = self.qkv.bias.view(3, h, hd)
                wp = self.proj.weight.view(dim, h, hd)
                pad = DPAD - hd
                off = ops.window_bias_offsets(
                    self.relative_position_bias_table, index, self.kw)
                self._prep_cache = (
                    key,
                    F.pad(wq, (0, 0, 0, pad)).reshape(3 * h * DPAD, dim)
                    .contiguous(),
                    F.pad(bq, (0, pad)).reshape(3 * h * DPAD).contiguous(),
                    F.pad(wp, (0, pad)).reshape(dim, h * DPAD).contiguous(),
                    off, off.float().contiguous(),
                )
        return self._prep_cache[1:]

    def attend(self, x: torch.Tensor, index: torch.Tensor, shift: int,
               native: bool) -> torch.Tensor:
        """x [B, H, W, dim] (normed tokens) -> proj(attention) [B, H, W, dim].
        native: the 32-wide head rows on the kernel; otherwise the stored
        head rows on the literal route."""
        b, h, w, _ = x.shape
        wq, bq, wp, off, off32 = self.prepared(index)
        if native:
            hd, off = DPAD, off32
        else:
            wq, bq, wp = self.qkv.weight, self.qkv.bias, self.proj.weight
            hd = self.hd
        qkv = F.linear(x, wq, bq).view(b, h, w, 3, self.heads, hd)
        a = ops.attention_hat(qkv, off, self.scale, shift, self.kw,
                              native=native)
        return F.linear(a, wp, self.proj.bias)

    forward = attend


class ChannelAttention(nn.Module):
    def __init__(self, dim: int, squeeze: int):
        super().__init__()
        self.attention = nn.Sequential(
            nn.AdaptiveAvgPool2d(1), _conv(dim, dim // squeeze, 1), nn.ReLU(),
            _conv(dim // squeeze, dim, 1), nn.Sigmoid())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, C, H, W] scaled per channel; the two 1x1 convs see one
        pixel a channel, so they stay plain matrix products."""
        y = x.mean((2, 3), keepdim=True)
        c1, c2 = self.attention[1], self.attention[3]
        y = F.relu(F.conv2d(y, c1.weight, c1.bias))
        return x * torch.sigmoid(F.conv2d(y, c2.weight, c2.bias))

    def prepared(self):
        """(w1 [S, C], b1 [S], w2 [C, S], b2 [C]) in fp32 for
        ops.channel_gate, re-cast when a parameter changes (as
        layers._fp32_cached)."""
        c1, c2 = self.attention[1], self.attention[3]
        src = (c1.weight, c1.bias, c2.weight, c2.bias)
        key = tuple((t.data_ptr(), t._version) for t in src)
        cache = getattr(self, "_fp32_cache", None)
        if cache is None or cache[0] != key:
            with torch.no_grad():
                cache = (key, c1.weight.float().flatten(1).contiguous(),
                         c1.bias.float(),
                         c2.weight.float().flatten(1).contiguous(),
                         c2.bias.float())
            self._fp32_cache = cache
        return cache[1:]


class CAB(nn.Module):
    def __init__(self, dim: int, compress: int, squeeze: int):
        super().__init__()
        self.cab = nn.Sequential(
            _conv(dim, dim // compress), nn.GELU(), _conv(dim // compress, dim),
            ChannelAttention(dim, squeeze))


def _ln(m, t):
    return F.layer_norm(t, (t.shape[-1],), m.weight, m.bias, m.eps)


def _plain_conv(m, t):
    return F.conv2d(t, m.weight, m.bias, padding=m.padding)


class HAB(nn.Module):
    def __init__(self, dim, heads, hidden, shift, compress, squeeze):
        super().__init__()
        self.shift = shift
        self.norm1 = FusedLayerNorm(dim)
        self.attn = HatAttention(dim, heads, WINDOW)
        self.conv_block = CAB(dim, compress, squeeze)
        self.norm2 = FusedLayerNorm(dim)
        self.mlp = Mlp(dim, hidden)

    def forward(self, x: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
        """The plain route on [B, H, W, dim] tokens."""
        n = _ln(self.norm1, x)
        cab = self.conv_block.cab
        c = _plain_conv(cab[2], F.gelu(_plain_conv(cab[0], _nchw(n))))
        x = x + self.attn(n, index, self.shift, native=False) \
            + CONV_SCALE * _tokens(cab[3](c))
        return x + self.mlp(_ln(self.norm2, x))


class OCAB(HatAttention):
    """The published names keep an OCAB's qkv, bias table and proj on the
    block itself, so the block is its own attention object."""

    def __init__(self, dim, heads, hidden):
        super().__init__(dim, heads, OVERLAP)
        self.norm1 = FusedLayerNorm(dim)
        self.norm2 = FusedLayerNorm(dim)
        self.mlp = Mlp(dim, hidden)

    def forward(self, x: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
        """The plain route on [B, H, W, dim] tokens."""
        x = x + self.attend(_ln(self.norm1, x), index, 0, native=False)
        return x + self.mlp(_ln(self.norm2, x))


class _Group(nn.Module):
    def __init__(self, blocks, overlap_attn):
        super().__init__()
        self.blocks = nn.ModuleList(blocks)
        self.overlap_attn = overlap_attn


class RHAG(nn.Module):
    def __init__(self, dim, depth, heads, hidden, compress, squeeze):
        super().__init__()
        self.residual_group = _Group(
            (HAB(dim, heads, hidden, 0 if j % 2 == 0 else WINDOW // 2,
                 compress, squeeze) for j in range(depth)),
            OCAB(dim, heads, hidden))
        self.conv = _conv(dim, dim)


class HAT(nn.Module):
    """HAT(embed_dim, depths, heads, mlp_ratio, compress_ratio,
    squeeze_factor), window 16, overlap ratio 0.5, 4x pixelshuffle:
    [N, 3, H, W] in 0..1 -> [N, 3, 4H, 4W]."""

    # as SwinIR.native_convs: the embed-width convs on ops.conv_ragged
    native_convs = True
    _conv_native = SwinIR._conv_native
    # a HAB's channel attention + residual sum + norm2 and the OCAB's
    # residual + norm2 on hab_tail.hip; False keeps them composed in torch
    # (A/B timing)
    fused_tail = True

    def __init__(self, embed_dim: int = 180, depths=(6,) * 6,
                 num_heads: int = 6, mlp_ratio: float = 2.0,
                 compress_ratio: int = 3, squeeze_factor: int = 30,
                 num_feat: int = 64):
        super().__init__()
        if embed_dim % num_heads or embed_dim // num_heads > DPAD:
            raise ValueError(
                f"HAT: embed_dim {embed_dim} / {num_heads} heads must give "
                f"a whole head dim of at most {DPAD}; " + _SUPPORTED)
        self.embed_dim, self.depths = embed_dim, tuple(depths)
        self.num_heads = num_heads
        self.mlp_hidden = round(embed_dim * mlp_ratio)
        self.compress_ratio, self.squeeze_factor = compress_ratio, squeeze_factor
        self.num_feat, self.scale = num_feat, 4
        self.register_buffer("relative_position_index_SA",
                             relative_position_index_sa())
        self.register_buffer("relative_position_index_OCA",
                             relative_position_index_oca())
        self.conv_first = _conv(3, embed_dim)
        self.patch_embed = _PatchEmbed(embed_dim)
        self.layers = nn.ModuleList(
            RHAG(embed_dim, d, num_heads, self.mlp_hidden, compress_ratio,
                 squeeze_factor) for d in self.depths)
        self.norm = FusedLayerNorm(embed_dim)
        self.conv_after_body = _conv(embed_dim, embed_dim)
        self.conv_before_upsample = nn.Sequential(_conv(embed_dim, num_feat),
                                                  nn.LeakyReLU(0.01))
        self.upsample = nn.Sequential(
            _conv(num_feat, 4 * num_feat), nn.PixelShuffle(2),
            _conv(num_feat, 4 * num_feat), nn.PixelShuffle(2))
        self.conv_last = _conv(num_feat, 3)

    # -- the plain route: CPU, native=False, the oracle ----------------------
    def _forward_plain(self, x: torch.Tensor) -> torch.Tensor:
        sa, oca = (self.relative_position_index_SA,
                   self.relative_position_index_OCA)
        first = _plain_conv(self.conv_first, x)
        t = _ln(self.patch_embed.norm, _tokens(first))
        for layer in self.layers:
            r = t
            for blk in layer.residual_group.blocks:
                t = blk(t, sa)
            t = layer.residual_group.overlap_attn(t, oca)
            t = _tokens(_plain_conv(layer.conv, _nchw(t))) + r
        feat = _plain_conv(self.conv_after_body,
                           _nchw(_ln(self.norm, t))) + first
        feat = F.leaky_relu(_plain_conv(self.conv_before_upsample[0], feat),
                            0.01)
        for up in (self.upsample[0], self.upsample[2]):
            feat = F.pixel_shuffle(_plain_conv(up, feat), 2)
        return _plain_conv(self.conv_last, feat)

    # -- the native route: bf16 on the GPU -----------------------------------
    def native_supported(self, x: torch.Tensor) -> bool:
        """True when forward(x) runs the attention on hat_attn_bf16_kernel
        and the 64-channel tail on the native convs."""
        return bool(
            x.is_cuda and x.dtype == torch.bfloat16
            and self.conv_first.weight.dtype == torch.bfloat16
            and ops.have_ext()
            and self.num_feat == 64
        )

    def _conv(self, m: nn.Module, x: torch.Tensor, res=None) -> torch.Tensor:
        """conv (+ res) on ops.conv_ragged, or on the library for a width
        the kernel does not take (HAT-S's 6-channel CAB) or native_convs
        off. x and res are NHWC views [N, C, H, W]."""
        y = self._conv_native(m, x, res=res)
        if y is None:
            y = m(x)
            if res is not None:
                y = y + res
        return y

    def _mlp_native(self, blk, t: torch.Tensor, nxt, n=None):
        """t + mlp(norm2(t)) and the following norm `nxt` of it (or None):
        ops.swin_mlp, composed at a width it has no instantiation for. n is
        norm2(t) where the fused tail has made it already."""
        if n is None:
            n = blk.norm2(t)
        if blk.mlp.fused and ops.swin_mlp_width_supported(t.shape[-1]):
            ln = _fp32_cached(nxt) if nxt is not None else (None, None)
            return ops.swin_mlp(n, t, *blk.mlp.prepared(), *ln,
                                eps=nxt.eps if nxt is not None else 1e-5)
        h = blk.mlp(n)
        if nxt is not None:
            return ops.add_layer_norm(h, t, *_fp32_cached(nxt), nxt.eps)
        return t + h, None

    def _group_native(self, t: torch.Tensor, group: _Group) -> torch.Tensor:
        """t [B, H, W, C] through a group's HABs and its OCAB. n is norm1(t)
        of the block about to run: the second output of the previous block's
        closing ops.swin_mlp."""
        sa, oca = (self.relative_position_index_SA,
                   self.relative_position_index_OCA)
        blocks, ocab = list(group.blocks), group.overlap_attn
        n = blocks[0].norm1(t) if blocks else ocab.norm1(t)
        for j, blk in enumerate(blocks):
            cab = blk.conv_block.cab
            c = F.gelu(self._conv(cab[0], _nchw(n)))
            c = self._conv(cab[2], c)
            attn = blk.attn(n, sa, blk.shift, native=True)
            n2 = None
            if self.fused_tail and ops.hab_tail_supported(t, attn, _tokens(c)) \
                    and self.embed_dim // self.squeeze_factor \
                    <= ops.CHANNEL_GATE_MAX_S:
                gate = ops.channel_gate(_tokens(c), *cab[3].prepared(),
                                        scale=CONV_SCALE)
                t, n2 = ops.gated_add_layer_norm(
                    t, attn, _tokens(c), gate, *_fp32_cached(blk.norm2),
                    blk.norm2.eps)
            else:
                t = t + attn + CONV_SCALE * _tokens(cab[3](c))
            nxt = blocks[j + 1].norm1 if j + 1 < len(blocks) else ocab.norm1
            t, n = self._mlp_native(blk, t, nxt, n2)
        attn = ocab.attend(n, oca, 0, native=True)
        if self.fused_tail:
            t, n2 = ops.add_layer_norm(attn, t, *_fp32_cached(ocab.norm2),
                                       ocab.norm2.eps)
            return self._mlp_native(ocab, t, None, n2)[0]
        t = t + attn
        return self._mlp_native(ocab, t, None)[0]

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous(memory_format=torch.channels_last)
        first = self.conv_first(x).contiguous(
            memory_format=torch.channels_last)
        t = self.patch_embed.norm(_tokens(first))
        for layer in self.layers:
            body = self._group_native(t, layer.residual_group)
            t = _tokens(self._conv(layer.conv, _nchw(body), res=_nchw(t)))
        feat = self._conv(self.conv_after_body, _nchw(self.norm(t)), res=first)
        feat = self._conv(self.conv_before_upsample, feat)
        for up in (self.upsample[0], self.upsample[2]):
            feat = F.pixel_shuffle(up(feat), 2)        # ops.conv3x3
        return self.conv_last(feat)                    # ops.conv3x3

    def forward(self, x: torch.Tensor, native: bool = True) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("HAT: x must be [N, 3, H, W], got "
                             f"{tuple(x.shape)}")
        if x.shape[2] * x.shape[3] > MAX_INPUT_PIXELS:
            raise ValueError(
                f"HAT: input {x.shape[3]}x{x.shape[2]} exceeds the "
                "whole-image limit of 2048 x 2048 pixels (tiling is not built)"
            )
        h, w = x.shape[2:]
        mean = torch.tensor(RGB_MEAN, dtype=x.dtype,
                            device=x.device).view(1, 3, 1, 1)
        x = x - mean
        ph, pw = -h % WINDOW, -w % WINDOW
        if ph >= h or pw >= w:
            raise ValueError(
                f"HAT: input {w}x{h} is too small to reflect-pad to a "
                f"multiple of the window ({WINDOW}); both sides need at "
                "least 9 pixels")
        if ph or pw:
            x = F.pad(x, (0, pw, 0, ph), mode="reflect")
        if native and self.native_supported(x):
            out = self._forward_native(x)
        else:
            out = self._forward_plain(x)
        return out[:, :, :4 * h, :4 * w] + mean


_OCAB0 = "layers.0.residual_group.overlap_attn."
_HAB0 = "layers.0.residual_group.blocks.0."


def is_hat_state_dict(keys) -> bool:
    """True when the tensor names are a HAT's (under any stored prefix)."""
    return any(k.endswith(_OCAB0 + "qkv.weight") for k in keys)


def hat_from_state_dict(state: Dict[str, torch.Tensor]) -> HAT:
    """Build a HAT from a published state dict (optionally under the
    params_ema. / params. prefix); widths, depths, heads, the MLP, compress
    and squeeze ratios are inferred from the tensors. The stored
    relative_position_index_SA / _OCA buffers are taken as they are; stored
    attn_mask buffers are ignored."""
    for prefix in ("params_ema.", "params."):
        if any(k.startswith(prefix) for k in state):
            state = {k[len(prefix):]: v for k, v in state.items()
                     if k.startswith(prefix)}
            break
    state = {k: v for k, v in state.items() if not k.endswith(".attn_mask")}
    need = ("conv_first.weight", _HAB0 + "attn.relative_position_bias_table",
            _OCAB0 + "relative_position_bias_table",
            _HAB0 + "conv_block.cab.0.weight",
            _HAB0 + "conv_block.cab.3.attention.1.weight",
            _HAB0 + "mlp.fc1.weight")
    if not all(k in state for k in need):
        raise ValueError("load_hat: not a HAT state dict; " + _SUPPORTED)
    first, table = state[need[0]], state[need[1]]
    up = [state.get(f"upsample.{i}.weight") for i in (0, 2, 4)]
    if not all(k in state for k in ("conv_before_upsample.0.weight",
                                    "conv_after_body.weight",
                                    "conv_last.weight")) \
            or up[0] is None or up[1] is None or up[2] is not None \
            or any(u.shape[0] != 4 * u.shape[1] for u in up[:2]):
        raise ValueError("load_hat: not the 4x pixelshuffle upsampler with "
                         "1conv residual connections (a 2x, 3x or 3conv "
                         "model); " + _SUPPORTED)
    if first.dim() != 4 or first.shape[1] != 3:
        raise ValueError(f"load_hat: conv_first takes {first.shape[1]} "
                         "channels; " + _SUPPORTED)
    if table.shape[0] != (2 * WINDOW - 1) ** 2 \
            or state[need[2]].shape[0] != (WINDOW + OVERLAP - 1) ** 2:
        raise ValueError(
            f"load_hat: bias tables of {table.shape[0]} and "
            f"{state[need[2]].shape[0]} rows are not window {WINDOW} with "
            f"overlap ratio 0.5; " + _SUPPORTED)
    dim, heads = int(first.shape[0]), int(table.shape[1])
    if dim % heads or dim // heads > DPAD:
        raise ValueError(f"load_hat: head dim {dim / heads:g} (embed {dim}"
                         f", {heads} heads); " + _SUPPORTED)
    depths: List[int] = []
    for key in state:
        part = key.split(".")
        if part[0] == "layers" and part[2:4] == ["residual_group", "blocks"]:
            i, j = int(part[1]), int(part[4])
            depths.extend([0] * (i + 1 - len(depths)))
            depths[i] = max(depths[i], j + 1)
    net = HAT(dim, depths, heads, state[need[5]].shape[0] / dim,
              compress_ratio=dim // state[need[3]].shape[0],
              squeeze_factor=dim // state[need[4]].shape[0],
              num_feat=int(state["conv_last.weight"].shape[1]))
    try:
        net.load_state_dict(state, strict=True)
    except RuntimeError as exc:
        raise ValueError(f"load_hat: {exc}; " + _SUPPORTED) from None
    return net.eval()


def load_hat(path: str) -> HAT:
    """Load a HAT upscaler from a .safetensors file."""
    if not str(path).endswith(".safetensors"):
        raise ValueError(f"load_hat: '{path}' is not a .safetensors file; "
                         + _SUPPORTED)
    from safetensors.torch import load_file

    return hat_from_state_dict(load_file(path))
