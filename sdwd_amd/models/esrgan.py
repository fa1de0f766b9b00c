"""ESRGAN-family upscalers: RRDBNet and SRVGGNetCompact (Real-ESRGAN /
BasicSR definitions).

A 4x RRDBNet is conv_first, nb residual-in-residual dense blocks (RRDB, three
dense blocks of five 3x3 convs each), conv_body plus the trunk residual, two
nearest-2x upsampling convs, conv_hr and conv_last, LeakyReLU(0.2) throughout.

On a bf16 GPU the trunk runs on ops.conv3x3_dense: a dense block lives in one
[N, nf + 4*gc, H, W] channels_last workspace laid out x | x1 | x2 | x3 | x4,
conv k reads a channel prefix and writes the next gc channels in place, and
conv 5 writes the first nf channels of the next workspace with the block's
residual (and, in the third block, the RRDB's) folded into its epilogue.
Nothing is concatenated or copied: 15 launches per RRDB. Three workspaces
rotate, because the RRDB's input must survive until its third block's conv 5
reads it as the outer residual.

A compact model (SRVGGNetCompact: "R-ESRGAN General 4xV3", "General WDN 4xV3",
"AnimeVideo") is a chain of 3x3 convs at one width, a per-channel PReLU after
each, ended by a 64 -> 48 conv, PixelShuffle(4) and + nearest4x(input). On a
bf16 GPU the stem runs on ops.conv3x3_small and every other conv on
ops.conv_compact, whose variants absorb the stem's activation, each layer's
PReLU, and the pixel shuffle with the nearest-4x residual: num_conv + 2
launches, no torch op between them.
"""
from __future__ import annotations

import re
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .layers import SDConv2d

SLOPE = 0.2
MAX_INPUT_PIXELS = 2048 * 2048

_SUPPORTED = (
    "supported: 4x RRDBNet .safetensors with 3-channel input, new-arch keys "
    "(conv_first, body.N.rdbK.convJ, conv_body, conv_up1/2, conv_hr, "
    "conv_last) or old-arch keys (model.0, model.1.sub.N.RDBK.convJ.0, ...), "
    "and 4x compact (SRVGGNetCompact) .safetensors with 64 features and "
    "per-channel PReLU (body.N keys). Not supported: 1x/2x pixel-unshuffle "
    "variants, non-3-channel input, compact models of scale 2 or 3, of "
    "another width or with ReLU / LeakyReLU, SwinIR / HAT / LDSR models"
)


def _conv(cin: int, cout: int) -> SDConv2d:
    return SDConv2d(cin, cout, 3, padding=1)


class ResidualDenseBlock(nn.Module):
    def __init__(self, nf: int, gc: int):
        super().__init__()
        for j in range(1, 5):
            setattr(self, f"conv{j}", _conv(nf + (j - 1) * gc, gc))
        self.conv5 = _conv(nf + 4 * gc, nf)

    def convs(self):
        return [getattr(self, f"conv{j}") for j in range(1, 6)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        feats = [x]
        for conv in self.convs()[:4]:
            y = F.conv2d(torch.cat(feats, 1), conv.weight, conv.bias, padding=1)
            feats.append(F.leaky_relu(y, SLOPE))
        c5 = self.conv5
        return F.conv2d(torch.cat(feats, 1), c5.weight, c5.bias,
                        padding=1) * 0.2 + x


class RRDB(nn.Module):
    def __init__(self, nf: int, gc: int):
        super().__init__()
        self.rdb1 = ResidualDenseBlock(nf, gc)
        self.rdb2 = ResidualDenseBlock(nf, gc)
        self.rdb3 = ResidualDenseBlock(nf, gc)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.rdb3(self.rdb2(self.rdb1(x))) * 0.2 + x


class RRDBNet(nn.Module):
    """RRDBNet(nf, gc, nb, scale=4): [N, 3, H, W] in 0..1 -> [N, 3, 4H, 4W]."""

    def __init__(self, nf: int = 64, gc: int = 32, nb: int = 23,
                 scale: int = 4):
        super().__init__()
        if scale != 4:
            raise ValueError(f"RRDBNet: only scale 4 is built (got {scale})")
        self.nf, self.gc, self.nb, self.scale = nf, gc, nb, scale
        self.conv_first = _conv(3, nf)
        self.body = nn.ModuleList(RRDB(nf, gc) for _ in range(nb))
        self.conv_body = _conv(nf, nf)
        self.conv_up1 = _conv(nf, nf)
        self.conv_up2 = _conv(nf, nf)
        self.conv_hr = _conv(nf, nf)
        self.conv_last = _conv(nf, 3)

    # -- the plain route: CPU, native=False, the oracle ----------------------
    def _forward_plain(self, x: torch.Tensor) -> torch.Tensor:
        def conv(m, t):
            return F.conv2d(t, m.weight, m.bias, padding=1)

        feat = conv(self.conv_first, x)
        body = feat
        for blk in self.body:
            body = blk(body)
        feat = feat + conv(self.conv_body, body)
        for up in (self.conv_up1, self.conv_up2):
            feat = F.leaky_relu(
                conv(up, F.interpolate(feat, scale_factor=2, mode="nearest")),
                SLOPE,
            )
        feat = F.leaky_relu(conv(self.conv_hr, feat), SLOPE)
        return conv(self.conv_last, feat)

    # -- the native route: bf16 on the GPU -----------------------------------
    def native_supported(self, x: torch.Tensor) -> bool:
        """True when forward(x) runs the trunk on conv3x3_dense_bf16_kernel:
        bf16 on the GPU and widths the kernel is instantiated for."""
        nf, gc = self.nf, self.gc
        return bool(
            x.is_cuda and x.dtype == torch.bfloat16
            and self.conv_first.weight.dtype == torch.bfloat16
            and ops.have_ext()
            and nf == 64 and gc == 32
            and ops.conv3x3_small_supported(3, nf)
        )

    def _trunk_native(self, feat: torch.Tensor) -> torch.Tensor:
        """feat [N, nf, H, W] -> the trunk's output as the [:, :nf] slice of
        a workspace. 15 conv3x3_dense launches per RRDB, nothing else."""
        nf, gc = self.nf, self.gc
        n, _, h, w = feat.shape
        ws = [
            torch.empty((n, nf + 4 * gc, h, w), dtype=feat.dtype,
                        device=feat.device, memory_format=torch.channels_last)
            for _ in range(3)
        ]
        ws[0][:, :nf].copy_(feat)
        cur = 0
        for blk in self.body:
            a, b, c = cur, (cur + 1) % 3, (cur + 2) % 3
            x0 = ws[a][:, :nf]
            for k, (rdb, s, d) in enumerate(
                ((blk.rdb1, a, b), (blk.rdb2, b, c), (blk.rdb3, c, b))
            ):
                src = ws[s]
                convs = rdb.convs()
                for j, conv in enumerate(convs[:4]):
                    cin = nf + j * gc
                    ops.conv3x3_dense(
                        src[:, :cin], conv._wprep(), conv.bias,
                        src[:, cin:cin + gc], lrelu=SLOPE,
                    )
                c5 = convs[4]
                if k < 2:  # 0.2 * c + x
                    ops.conv3x3_dense(
                        src, c5._wprep(), c5.bias, ws[d][:, :nf],
                        alpha=0.2, res2=src[:, :nf],
                    )
                else:      # 0.2 * (0.2 * c + x3) + x0
                    ops.conv3x3_dense(
                        src, c5._wprep(), c5.bias, ws[d][:, :nf],
                        alpha=0.04, res1=src[:, :nf], beta=0.2, res2=x0,
                    )
            cur = b
        return ws[cur][:, :nf]

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous(memory_format=torch.channels_last)
        feat = self.conv_first(x)                      # ops.conv3x3_small
        body = self._trunk_native(feat)
        body = body.contiguous(memory_format=torch.channels_last)
        feat = self.conv_body(body, residual=feat)     # ops.conv3x3, fused +
        for up in (self.conv_up1, self.conv_up2):
            feat = F.leaky_relu_(up.forward_upsampled2x(feat), SLOPE)  # FOLD
        hr = torch.empty_like(feat)
        ops.conv3x3_dense(feat, self.conv_hr._wprep(), self.conv_hr.bias, hr,
                          lrelu=SLOPE)
        return self.conv_last(hr)                      # ops.conv3x3

    def forward(self, x: torch.Tensor, native: bool = True) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("RRDBNet: x must be [N, 3, H, W], got "
                             f"{tuple(x.shape)}")
        if x.shape[2] * x.shape[3] > MAX_INPUT_PIXELS:
            raise ValueError(
                f"RRDBNet: input {x.shape[3]}x{x.shape[2]} exceeds the "
                "whole-image limit of 2048 x 2048 pixels (tiling is not built)"
            )
        if native and self.native_supported(x):
            return self._forward_native(x)
        return self._forward_plain(x)


class SRVGGNetCompact(nn.Module):
    """SRVGGNetCompact(nf, num_conv, scale=4): [N, 3, H, W] in 0..1 ->
    [N, 3, 4H, 4W]. `body` is Real-ESRGAN's module list: conv, PReLU,
    (conv, PReLU) x num_conv, conv to 3 * scale^2 channels."""

    def __init__(self, nf: int = 64, num_conv: int = 16, scale: int = 4):
        super().__init__()
        if scale != 4:
            raise ValueError("SRVGGNetCompact: only scale 4 is built "
                             f"(got {scale})")
        self.nf, self.num_conv, self.scale = nf, num_conv, scale
        mods = [_conv(3, nf), nn.PReLU(nf)]
        for _ in range(num_conv):
            mods += [_conv(nf, nf), nn.PReLU(nf)]
        mods.append(_conv(nf, 3 * scale * scale))
        self.body = nn.ModuleList(mods)

    # -- the plain route: CPU, native=False, the oracle ----------------------
    def _forward_plain(self, x: torch.Tensor) -> torch.Tensor:
        out = x
        for m in self.body:
            if isinstance(m, nn.PReLU):
                out = F.prelu(out, m.weight)
            else:
                out = F.conv2d(out, m.weight, m.bias, padding=1)
        out = F.pixel_shuffle(out, self.scale)
        return out + F.interpolate(x, scale_factor=self.scale, mode="nearest")

    # -- the native route: bf16 on the GPU -----------------------------------
    def native_supported(self, x: torch.Tensor) -> bool:
        """True when forward(x) runs every conv after the stem on
        conv_compact_bf16_kernel: bf16 on the GPU at 64 features."""
        return bool(
            x.is_cuda and x.dtype == torch.bfloat16
            and self.body[0].weight.dtype == torch.bfloat16
            and ops.have_ext()
            and self.nf == 64 and self.scale == 4 and self.num_conv >= 1
            and ops.conv3x3_small_supported(3, self.nf)
        )

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous(memory_format=torch.channels_last)
        convs, acts = self.body[0::2], self.body[1::2]
        stem = convs[0]
        feat = ops.conv3x3_small(x, stem._wprep(), stem.bias)
        pre = acts[0].weight       # the stem's PReLU, applied by the next conv
        for conv, act in zip(convs[1:-1], acts[1:]):
            feat = ops.conv_compact(feat, conv._wprep(), conv.bias,
                                    slope=act.weight, pre_slope=pre)
            pre = None
        last = convs[-1]           # + pixel shuffle + nearest4x(x)
        return ops.conv_compact(feat, last._wprep(), last.bias,
                                shuffle_base=x)

    def forward(self, x: torch.Tensor, native: bool = True) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("SRVGGNetCompact: x must be [N, 3, H, W], got "
                             f"{tuple(x.shape)}")
        if x.shape[2] * x.shape[3] > MAX_INPUT_PIXELS:
            raise ValueError(
                f"SRVGGNetCompact: input {x.shape[3]}x{x.shape[2]} exceeds "
                "the whole-image limit of 2048 x 2048 pixels (tiling is not "
                "built)"
            )
        if native and self.native_supported(x):
            return self._forward_native(x)
        return self._forward_plain(x)


# old-arch (ESRGAN "model.N") names -> new-arch names; nb is the index of the
# trunk conv inside model.1.sub
_OLD_RDB = re.compile(r"^model\.1\.sub\.(\d+)\.RDB(\d)\.conv(\d)\.0\.(weight|bias)$")
_OLD_FIXED = {"model.0": "conv_first", "model.3": "conv_up1",
              "model.6": "conv_up2", "model.8": "conv_hr",
              "model.10": "conv_last"}


def _rename_old_arch(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for key, val in state.items():
        m = _OLD_RDB.match(key)
        if m:
            out[f"body.{m[1]}.rdb{m[2]}.conv{m[3]}.{m[4]}"] = val
            continue
        stem, _, leaf = key.rpartition(".")
        if stem in _OLD_FIXED:
            out[f"{_OLD_FIXED[stem]}.{leaf}"] = val
        elif re.match(r"^model\.1\.sub\.\d+$", stem):
            out[f"conv_body.{leaf}"] = val
        else:
            raise ValueError(f"load_esrgan: unknown tensor '{key}'; "
                             + _SUPPORTED)
    return out


_COMPACT_KEY = re.compile(r"^body\.(\d+)\.(weight|bias)$")


def _compact_from_state_dict(state: Dict[str, torch.Tensor]) -> SRVGGNetCompact:
    """Real-ESRGAN's SRVGGNetCompact layout: body.0 the stem conv, odd body.k
    the PReLU slopes, the last body.k the 3 * scale^2 conv; nf, num_conv and
    scale are inferred from the tensors."""
    for key in state:
        if not _COMPACT_KEY.match(key):
            raise ValueError(f"load_esrgan: unknown tensor '{key}'; "
                             + _SUPPORTED)
    stem = state["body.0.weight"]
    last_k = max(int(_COMPACT_KEY.match(k)[1]) for k in state)
    last = state.get(f"body.{last_k}.weight")
    if stem.dim() != 4 or tuple(stem.shape[1:]) != (3, 3, 3):
        raise ValueError("load_esrgan: the compact model's stem is not a 3x3 "
                         "conv of 3 channels; " + _SUPPORTED)
    nf = stem.shape[0]
    slopes = state.get("body.1.weight")
    if slopes is None or slopes.dim() != 1 or slopes.numel() != nf:
        raise ValueError(
            "load_esrgan: the compact model's activation is not a "
            "per-channel PReLU (ReLU / LeakyReLU variant); " + _SUPPORTED)
    if last_k % 2 or last_k < 2 or last is None or last.dim() != 4:
        raise ValueError("load_esrgan: the compact model does not end in a "
                         "conv; " + _SUPPORTED)
    scale = round((last.shape[0] / 3) ** 0.5)
    if 3 * scale * scale != last.shape[0] or scale != 4:
        raise ValueError(
            f"load_esrgan: compact model with {last.shape[0]} output "
            "channels (scale is not 4); " + _SUPPORTED)
    if nf != 64:
        raise ValueError(f"load_esrgan: compact model with {nf} features; "
                         + _SUPPORTED)
    net = SRVGGNetCompact(nf=nf, num_conv=(last_k - 2) // 2, scale=scale)
    try:
        net.load_state_dict(state, strict=True)
    except RuntimeError as exc:
        raise ValueError(f"load_esrgan: {exc}; " + _SUPPORTED) from None
    return net.eval()


def esrgan_from_state_dict(state: Dict[str, torch.Tensor]) -> nn.Module:
    """Build an RRDBNet (either key naming; nf, gc and nb inferred from the
    tensors) or, when there is no conv_first and the body.N tensors are a
    compact model's, an SRVGGNetCompact."""
    for prefix in ("params_ema.", "params."):
        state = {k[len(prefix):] if k.startswith(prefix) else k: v
                 for k, v in state.items()}
    if "conv_first.weight" not in state and "body.0.weight" in state and (
            "body.1.weight" not in state or state["body.1.weight"].dim() == 1):
        return _compact_from_state_dict(state)
    if any(k.startswith("model.") for k in state):
        state = _rename_old_arch(state)
    first = state.get("conv_first.weight")
    c1 = state.get("body.0.rdb1.conv1.weight")
    if first is None or c1 is None or "conv_up2.weight" not in state:
        raise ValueError("load_esrgan: not a 4x RRDBNet state dict; "
                         + _SUPPORTED)
    if first.dim() != 4 or first.shape[1] != 3 or first.shape[2:] != (3, 3):
        raise ValueError(
            f"load_esrgan: conv_first takes {first.shape[1]} channels (a "
            "pixel-unshuffle or non-RGB variant); " + _SUPPORTED
        )
    nb = 1 + max(int(k.split(".")[1]) for k in state if k.startswith("body."))
    net = RRDBNet(nf=first.shape[0], gc=c1.shape[0], nb=nb)
    try:
        net.load_state_dict(state, strict=True)
    except RuntimeError as exc:
        raise ValueError(f"load_esrgan: {exc}; " + _SUPPORTED) from None
    return net.eval()


def load_esrgan(path: str) -> nn.Module:
    """Load an ESRGAN-family upscaler (RRDBNet or SRVGGNetCompact) from a
    .safetensors file."""
    if not str(path).endswith(".safetensors"):
        raise ValueError(f"load_esrgan: '{path}' is not a .safetensors file; "
                         + _SUPPORTED)
    from safetensors.torch import load_file

    return esrgan_from_state_dict(load_file(path))


@torch.no_grad()
def upscale_image(net: nn.Module, rgb: torch.Tensor, size=None) -> torch.Tensor:
    """net: a 4x upscaler (RRDBNet, SRVGGNetCompact, models/swinir.py SwinIR
    or models/hat.py HAT) or the 1x models/scunet.py SCUNet.
    rgb [N, 3, H, W] in 0..1 (any float dtype, any device) -> the model's
    output in fp32, clamped to 0..1, on rgb's device; with size = (h, w)
    resized to it by the pipeline's Lanczos stand-in (antialiased bicubic),
    as the host upscales past the target and resizes down."""
    p = next(net.parameters())
    out = net(rgb.to(device=p.device, dtype=p.dtype)).float().clamp(0, 1)
    if size is not None and tuple(out.shape[2:]) != tuple(size):
        out = F.interpolate(out, size=tuple(size), mode="bicubic",
                            antialias=True).clamp(0, 1)
    return out.to(rgb.device)
