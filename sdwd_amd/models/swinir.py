"""SwinIR upscalers (BasicSR definition), the `nearest+conv` 4x real-world
configurations the host ships as SwinIR_4x (embed 180 / 6 heads / 1conv and
embed 240 / 8 heads / 3conv, window 8, head dim 30).

The network is conv_first, a LayerNorm over the token grid, residual Swin
transformer blocks (RSTB: Swin blocks with a shift of 0 and 4 in turn, then a
conv and the group's residual), a final norm, conv_after_body plus the skip,
and the 64-channel upsampling tail of RRDBNet.

On a bf16 GPU the tokens stay one [B, H, W, C] tensor from conv_first to the
tail. A Swin block is: ops.layer_norm, the QKV GEMM, ops.attention_swin on the
GEMM's output viewed as [B, H, W, 3, heads, 32], the proj GEMM,
ops.add_layer_norm (residual + norm2), and ops.swin_mlp: fc1, GELU, fc2, the
residual and the next block's norm1 in one kernel (Mlp.fused). The convs at
the embed width (an RSTB's closing conv or 3conv stack, conv_after_body,
conv_before_upsample) run on ops.conv_ragged with their LeakyReLU and their
residual in the epilogue (SwinIR.native_convs). Nothing is
rolled, partitioned, masked or permuted. Each head's 30 q/k/v rows are
zero-padded to 32 once per weight version so a head row is 64 bytes: padded
q/k channels add 0 to every score and padded v channels meet zero proj
columns; the MLP's weights are zero-padded once the same way
(ops.swin_mlp_prepare), and so are the conv weights (ops.conv_ragged_prepare).
The QKV and proj GEMMs stay on the library, and so does the MLP at an embed width the kernel has no instantiation for
(no multiple of 4, or above 256), which runs composed as with Mlp.fused off.
"""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .esrgan import MAX_INPUT_PIXELS
from .layers import FusedLayerNorm, SDConv2d, _fp32_cached

WINDOW = ops.SWIN_WINDOW
DPAD = ops.SWIN_DPAD
RGB_MEAN = (0.4488, 0.4371, 0.4040)
SLOPE = 0.2

_SUPPORTED = (
    "supported: 4x SwinIR .safetensors with the nearest+conv upsampler "
    "(conv_before_upsample, conv_up1, conv_up2, conv_hr, conv_last), window "
    "8, head dim <= 32, 1conv or 3conv residual connections, 3-channel "
    "input (the real-world SwinIR-M / SwinIR-L x4 models). Not supported: "
    "pixelshuffle, pixelshuffledirect (lightweight) and denoising heads, "
    "scales other than 4, windows other than 8, head dims above 32, DAT "
    "(HAT: models/hat.py)"
)


def relative_position_index() -> torch.Tensor:
    """[64, 64] index of (query, key) into the (15 * 15)-row bias table."""
    c = torch.stack(torch.meshgrid(torch.arange(WINDOW), torch.arange(WINDOW),
                                   indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (WINDOW - 1)
    return rel[:, :, 0] * (2 * WINDOW - 1) + rel[:, :, 1]


def _conv(cin: int, cout: int, k: int = 3) -> SDConv2d:
    return SDConv2d(cin, cout, k, padding=k // 2)


def _res_conv(dim: int, kind: str) -> nn.Module:
    if kind == "1conv":
        return _conv(dim, dim)
    return nn.Sequential(
        _conv(dim, dim // 4), nn.LeakyReLU(SLOPE),
        _conv(dim // 4, dim // 4, 1), nn.LeakyReLU(SLOPE),
        _conv(dim // 4, dim),
    )


class WindowAttention(nn.Module):
    def __init__(self, dim: int, heads: int):
        super().__init__()
        self.dim, self.heads, self.hd = dim, heads, dim // heads
        self.scale = self.hd ** -0.5
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((2 * WINDOW - 1) ** 2, heads))
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self._prep_cache = None

    def gathered_bias(self) -> torch.Tensor:
        """[heads, 64, 64] in the table's dtype."""
        idx = relative_position_index().to(
            self.relative_position_bias_table.device)
        n = WINDOW * WINDOW
        return self.relative_position_bias_table[idx.view(-1)].view(
            n, n, self.heads).permute(2, 0, 1).contiguous()

    def prepared(self):
        """(qkv weight [3*heads*32, dim], qkv bias, proj weight
        [dim, heads*32], fp32 bias [heads, 64, 64]), rebuilt when a source
        tensor changes (like SDConv2d._wprep)."""
        src = (self.qkv.weight, self.qkv.bias, self.proj.weight,
               self.relative_position_bias_table)
        key = tuple((t.data_ptr(), t._version, t.dtype) for t in src)
        if self._prep_cache is None or self._prep_cache[0] != key:
            with torch.no_grad():
                h, hd, dim = self.heads, self.hd, self.dim
                wq = self.qkv.weight.view(3, h, hd, dim)
                bq = self.qkv.bias.view(3, h, hd)
                wp = self.proj.weight.view(dim, h, hd)
                pad = DPAD - hd
                self._prep_cache = (
                    key,
                    F.pad(wq, (0, 0, 0, pad)).reshape(3 * h * DPAD, dim)
                    .contiguous(),
                    F.pad(bq, (0, pad)).reshape(3 * h * DPAD).contiguous(),
                    F.pad(wp, (0, pad)).reshape(dim, h * DPAD).contiguous(),
                    self.gathered_bias().float().contiguous(),
                )
        return self._prep_cache[1:]

    def forward(self, x: torch.Tensor, shift: int, padded: bool,
                native: bool) -> torch.Tensor:
        """x [B, H, W, dim] (normed tokens) -> proj(attention) [B, H, W, dim].
        padded: the 32-wide head rows; otherwise the stored 30-wide ones."""
        b, h, w, _ = x.shape
        if padded:
            wq, bq, wp, bias = self.prepared()
            hd = DPAD
        else:
            wq, bq, wp = self.qkv.weight, self.qkv.bias, self.proj.weight
            bias, hd = self.gathered_bias(), self.hd
        qkv = F.linear(x, wq, bq).view(b, h, w, 3, self.heads, hd)
        a = ops.attention_swin(qkv, bias, self.scale, shift, native=native)
        return F.linear(a, wp, self.proj.bias)


class Mlp(nn.Module):
    # the native route runs fc1 + GELU + fc2 + residual + the following norm
    # as one ops.swin_mlp call; False keeps the composed route
    fused = True

    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)
        self._prep_cache = None

    def prepared(self):
        """ops.swin_mlp_prepare of fc1 and fc2 (zero-padded weights, fp32
        biases), rebuilt when a source tensor changes (like
        WindowAttention.prepared)."""
        src = (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)
        key = tuple((t.data_ptr(), t._version, t.dtype) for t in src)
        if self._prep_cache is None or self._prep_cache[0] != key:
            with torch.no_grad():
                self._prep_cache = (key,) + tuple(ops.swin_mlp_prepare(*src))
        return self._prep_cache[1:]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc2(F.gelu(self.fc1(x)))


class SwinBlock(nn.Module):
    def __init__(self, dim: int, heads: int, hidden: int, shift: int):
        super().__init__()
        self.shift = shift
        self.norm1 = FusedLayerNorm(dim)
        self.attn = WindowAttention(dim, heads)
        self.norm2 = FusedLayerNorm(dim)
        self.mlp = Mlp(dim, hidden)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The plain route on [B, H, W, dim] tokens."""
        def ln(m, t):
            return F.layer_norm(t, (t.shape[-1],), m.weight, m.bias, m.eps)

        x = x + self.attn(ln(self.norm1, x), self.shift, padded=False,
                          native=False)
        return x + self.mlp(ln(self.norm2, x))


class _Group(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.blocks = nn.ModuleList(blocks)


class RSTB(nn.Module):
    def __init__(self, dim: int, depth: int, heads: int, hidden: int,
                 resi: str):
        super().__init__()
        self.residual_group = _Group(
            SwinBlock(dim, heads, hidden, 0 if j % 2 == 0 else WINDOW // 2)
            for j in range(depth))
        self.conv = _res_conv(dim, resi)


class _PatchEmbed(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.norm = FusedLayerNorm(dim)


def _nchw(tokens: torch.Tensor) -> torch.Tensor:
    """[B, H, W, C] tokens as the channels_last NCHW view of the same memory."""
    return tokens.permute(0, 3, 1, 2)


def _tokens(img: torch.Tensor) -> torch.Tensor:
    return img.permute(0, 2, 3, 1)


def _ragged_prepared(conv: SDConv2d) -> torch.Tensor:
    """ops.conv_ragged_prepare of the conv's weight, rebuilt when the weight
    changes (like SDConv2d._wprep)."""
    w = conv.weight
    key = (w.data_ptr(), w._version, w.dtype)
    cache = getattr(conv, "_ragged_cache", None)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            cache = (key, ops.conv_ragged_prepare(w))
        conv._ragged_cache = cache
    return cache[1]


class SwinIR(nn.Module):
    """SwinIR(embed_dim, depths, heads, mlp_ratio, resi_connection), 4x
    nearest+conv: [N, 3, H, W] in 0..1 -> [N, 3, 4H, 4W]."""

    # the native route runs the convs at the embed width (and their 3conv
    # stacks) on ops.conv_ragged with the activation and the residual in the
    # epilogue; False keeps the library conv plus elementwise passes
    native_convs = True

    def __init__(self, embed_dim: int = 180, depths=(6,) * 6,
                 num_heads: int = 6, mlp_ratio: float = 2.0,
                 resi_connection: str = "1conv", num_feat: int = 64):
        super().__init__()
        if resi_connection not in ("1conv", "3conv"):
            raise ValueError("SwinIR: resi_connection must be 1conv or 3conv")
        if embed_dim % num_heads or embed_dim // num_heads > DPAD:
            raise ValueError(
                f"SwinIR: embed_dim {embed_dim} / {num_heads} heads must give "
                f"a whole head dim of at most {DPAD}; " + _SUPPORTED)
        self.embed_dim, self.depths = embed_dim, tuple(depths)
        self.num_heads, self.resi_connection = num_heads, resi_connection
        self.mlp_hidden = round(embed_dim * mlp_ratio)
        self.num_feat, self.scale = num_feat, 4
        self.conv_first = _conv(3, embed_dim)
        self.patch_embed = _PatchEmbed(embed_dim)
        self.layers = nn.ModuleList(
            RSTB(embed_dim, d, num_heads, self.mlp_hidden, resi_connection)
            for d in self.depths)
        self.norm = FusedLayerNorm(embed_dim)
        self.conv_after_body = _res_conv(embed_dim, resi_connection)
        self.conv_before_upsample = nn.Sequential(_conv(embed_dim, num_feat),
                                                  nn.LeakyReLU(0.01))
        self.conv_up1 = _conv(num_feat, num_feat)
        self.conv_up2 = _conv(num_feat, num_feat)
        self.conv_hr = _conv(num_feat, num_feat)
        self.conv_last = _conv(num_feat, 3)

    def _mean(self, x: torch.Tensor) -> torch.Tensor:
        return torch.tensor(RGB_MEAN, dtype=x.dtype,
                            device=x.device).view(1, 3, 1, 1)

    # -- the plain route: CPU, native=False, the oracle ----------------------
    def _forward_plain(self, x: torch.Tensor) -> torch.Tensor:
        def conv(m, t):
            if isinstance(m, nn.Sequential):
                for sub in m:
                    t = conv(sub, t) if isinstance(sub, nn.Conv2d) else sub(t)
                return t
            return F.conv2d(t, m.weight, m.bias, padding=m.padding)

        def ln(m, t):
            return F.layer_norm(t, (t.shape[-1],), m.weight, m.bias, m.eps)

        first = conv(self.conv_first, x)
        t = ln(self.patch_embed.norm, _tokens(first))
        for layer in self.layers:
            r = t
            for blk in layer.residual_group.blocks:
                t = blk(t)
            t = _tokens(conv(layer.conv, _nchw(t))) + r
        feat = conv(self.conv_after_body, _nchw(ln(self.norm, t))) + first
        feat = conv(self.conv_before_upsample, feat)
        for up in (self.conv_up1, self.conv_up2):
            feat = F.leaky_relu(
                conv(up, F.interpolate(feat, scale_factor=2, mode="nearest")),
                SLOPE)
        feat = F.leaky_relu(conv(self.conv_hr, feat), SLOPE)
        return conv(self.conv_last, feat)

    # -- the native route: bf16 on the GPU -----------------------------------
    def native_supported(self, x: torch.Tensor) -> bool:
        """True when forward(x) runs the Swin blocks on swin_attn_bf16_kernel
        and the 64-channel tail on the native convs."""
        return bool(
            x.is_cuda and x.dtype == torch.bfloat16
            and self.conv_first.weight.dtype == torch.bfloat16
            and ops.have_ext()
            and self.num_feat == 64
        )

    def _blocks_native(self, t: torch.Tensor, blocks) -> torch.Tensor:
        """t [B, H, W, C] through a group's Swin blocks. n is norm1(t) of the
        block about to run: ops.layer_norm for the first, the second output
        of the previous block's closing ops.swin_mlp (ops.add_layer_norm
        with Mlp.fused off, or at an embed width that is no multiple of 4 or
        above 256) for the rest."""
        n = blocks[0].norm1(t)
        # widths the kernel has no instantiation for keep the composed route
        fits = ops.swin_mlp_width_supported(t.shape[-1])
        for j, blk in enumerate(blocks):
            p = blk.attn(n, blk.shift, padded=True, native=True)
            t, n = ops.add_layer_norm(p, t, *_fp32_cached(blk.norm2),
                                      blk.norm2.eps)
            n1 = blocks[j + 1].norm1 if j + 1 < len(blocks) else None
            if blk.mlp.fused and fits:
                ln = _fp32_cached(n1) if n1 is not None else (None, None)
                t, n = ops.swin_mlp(n, t, *blk.mlp.prepared(), *ln,
                                    eps=n1.eps if n1 is not None else 1e-5)
                continue
            h = blk.mlp(n)
            if n1 is not None:
                t, n = ops.add_layer_norm(h, t, *_fp32_cached(n1), n1.eps)
            else:
                t = t + h
        return t

    def _conv_native(self, m: nn.Module, x: torch.Tensor, res=None):
        """act(conv(x)) + res for a conv, or a Sequential of convs and
        LeakyReLUs, on ops.conv_ragged: one launch per conv, its LeakyReLU
        and (on the last one) the residual in the epilogue. x and res are
        NHWC views [N, C, H, W]. None when native_convs is off or a conv is
        outside the kernel's range: the caller keeps the library route."""
        if not self.native_convs:
            return None
        mods = list(m) if isinstance(m, nn.Sequential) else [m]
        steps = []          # (conv, slope of the LeakyReLU behind it or None)
        for sub in mods:
            if isinstance(sub, nn.LeakyReLU) and steps and steps[-1][1] is None:
                steps[-1] = (steps[-1][0], sub.negative_slope)
            elif isinstance(sub, SDConv2d):
                steps.append((sub, None))
            else:
                return None
        if steps[-1][1] is not None and res is not None:
            return None     # the epilogue activates before the residual only
        n, _, h, w = x.shape
        outs = []
        for conv, _ in steps:
            k = conv.kernel_size
            out = torch.empty((n, conv.out_channels, h, w), dtype=x.dtype,
                              device=x.device,
                              memory_format=torch.channels_last)
            if (k[0] != k[1] or conv.padding != (k[0] // 2, k[0] // 2)
                    or conv.stride != (1, 1) or conv.dilation != (1, 1)
                    or conv.groups != 1
                    or getattr(conv, "circular", False)
                    or not ops.conv_ragged_supported(
                        outs[-1] if outs else x, conv.weight, out)):
                return None
            outs.append(out)
        for i, ((conv, slope), out) in enumerate(zip(steps, outs)):
            x = ops.conv_ragged(
                x, _ragged_prepared(conv), conv.bias, out,
                ksize=conv.kernel_size[0], lrelu=slope,
                res=res if i + 1 == len(steps) else None)
        return x

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous(memory_format=torch.channels_last)
        first = self.conv_first(x).contiguous(
            memory_format=torch.channels_last)
        t = self.patch_embed.norm(_tokens(first))
        for layer in self.layers:
            body = self._blocks_native(t, list(layer.residual_group.blocks))
            y = self._conv_native(layer.conv, _nchw(body), res=_nchw(t))
            if y is not None:
                t = _tokens(y)
            else:
                t = _tokens(layer.conv(_nchw(body))).contiguous() + t
        body = _nchw(self.norm(t))
        feat = self._conv_native(self.conv_after_body, body, res=first)
        if feat is None:
            feat = self.conv_after_body(body) + first
        body, feat = feat, self._conv_native(self.conv_before_upsample, feat)
        if feat is None:
            feat = self.conv_before_upsample(body)
        for up in (self.conv_up1, self.conv_up2):
            feat = F.leaky_relu_(up.forward_upsampled2x(feat), SLOPE)  # FOLD
        feat = feat.contiguous(memory_format=torch.channels_last)
        hr = torch.empty_like(feat)
        ops.conv3x3_dense(feat, self.conv_hr._wprep(), self.conv_hr.bias, hr,
                          lrelu=SLOPE)
        return self.conv_last(hr)                      # ops.conv3x3

    def forward(self, x: torch.Tensor, native: bool = True) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("SwinIR: x must be [N, 3, H, W], got "
                             f"{tuple(x.shape)}")
        if x.shape[2] * x.shape[3] > MAX_INPUT_PIXELS:
            raise ValueError(
                f"SwinIR: input {x.shape[3]}x{x.shape[2]} exceeds the "
                "whole-image limit of 2048 x 2048 pixels (tiling is not built)"
            )
        h, w = x.shape[2:]
        mean = self._mean(x)
        x = x - mean
        ph, pw = -h % WINDOW, -w % WINDOW
        if ph >= h or pw >= w:
            raise ValueError(
                f"SwinIR: input {w}x{h} is too small to reflect-pad to a "
                f"multiple of the window ({WINDOW}); both sides need at "
                "least 5 pixels")
        if ph or pw:
            x = F.pad(x, (0, pw, 0, ph), mode="reflect")
        if native and self.native_supported(x):
            out = self._forward_native(x)
        else:
            out = self._forward_plain(x)
        return out[:, :, :4 * h, :4 * w] + mean


_BLOCK0 = "layers.0.residual_group.blocks.0.attn."


def is_swinir_state_dict(keys) -> bool:
    """True when the tensor names are a SwinIR's (under any stored prefix)."""
    return any(k.endswith(_BLOCK0 + "qkv.weight") for k in keys)


def swinir_from_state_dict(state: Dict[str, torch.Tensor]) -> SwinIR:
    """Build a SwinIR from a BasicSR state dict (optionally under the
    params_ema. / params. prefix); widths, depths, heads, mlp_ratio and
    resi_connection are inferred from the tensors. Stored attn_mask and
    relative_position_index buffers are ignored: both are recomputed."""
    for prefix in ("params_ema.", "params."):
        if any(k.startswith(prefix) for k in state):
            state = {k[len(prefix):]: v for k, v in state.items()
                     if k.startswith(prefix)}
            break
    state = {k: v for k, v in state.items()
             if not k.endswith((".attn_mask", ".relative_position_index"))}
    table = state.get(_BLOCK0 + "relative_position_bias_table")
    first = state.get("conv_first.weight")
    if table is None or first is None:
        raise ValueError("load_swinir: not a SwinIR state dict; " + _SUPPORTED)
    if not all(k in state for k in ("conv_before_upsample.0.weight",
                                    "conv_up1.weight", "conv_up2.weight",
                                    "conv_hr.weight", "conv_last.weight")):
        raise ValueError("load_swinir: not the 4x nearest+conv upsampler "
                         "(a pixelshuffle, lightweight, 2x or denoising "
                         "model); " + _SUPPORTED)
    if first.dim() != 4 or first.shape[1] != 3:
        raise ValueError(f"load_swinir: conv_first takes {first.shape[1]} "
                         "channels; " + _SUPPORTED)
    if table.shape[0] != (2 * WINDOW - 1) ** 2:
        raise ValueError(f"load_swinir: a bias table of {table.shape[0]} rows "
                         f"is not window {WINDOW}; " + _SUPPORTED)
    dim, heads = int(first.shape[0]), int(table.shape[1])
    if dim % heads or dim // heads > DPAD:
        raise ValueError(f"load_swinir: head dim {dim / heads:g} (embed {dim}"
                         f", {heads} heads); " + _SUPPORTED)
    depths: List[int] = []
    for key in state:
        part = key.split(".")
        if part[0] == "layers" and part[2:4] == ["residual_group", "blocks"]:
            i, j = int(part[1]), int(part[4])
            depths.extend([0] * (i + 1 - len(depths)))
            depths[i] = max(depths[i], j + 1)
    hidden = state[_BLOCK0.replace("attn.", "mlp.") + "fc1.weight"].shape[0]
    resi = "1conv" if "conv_after_body.weight" in state else "3conv"
    net = SwinIR(dim, depths, heads, hidden / dim, resi,
                 num_feat=int(state["conv_hr.weight"].shape[0]))
    try:
        net.load_state_dict(state, strict=True)
    except RuntimeError as exc:
        raise ValueError(f"load_swinir: {exc}; " + _SUPPORTED) from None
    return net.eval()


def load_swinir(path: str) -> SwinIR:
    """Load a SwinIR upscaler from a .safetensors file."""
    if not str(path).endswith(".safetensors"):
        raise ValueError(f"load_swinir: '{path}' is not a .safetensors file; "
                         + _SUPPORTED)
    from safetensors.torch import load_file

    return swinir_from_state_dict(load_file(path))
