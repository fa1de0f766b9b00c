"""SCUNet (KAIR's Swin-Conv UNet), the host's `ScuNET GAN` / `ScuNET PSNR`
upscalers: a 1x restoration network (the caller resizes its output), window
8, head dim 32, KAIR's module and key names.

m_head (3x3) -> m_down1..3 (ConvTransBlocks at branch widths dim/2, dim,
2 dim, each stage closed by a 2x2 stride-2 conv) -> m_body (4 dim) ->
m_up3..1 (a 2x2 stride-2 transposed conv, then blocks) -> m_tail (3x3), with
the UNet's skips added, not concatenated. A ConvTransBlock is a 1x1 conv, a
split into a conv half (3x3, ReLU, 3x3, + itself) and a transformer half
(x + msa(ln1 x); x + mlp(ln2 x), blocks alternating shift 0 and 4), the
concatenation, a 1x1 conv and the block's residual.

On a bf16 GPU a stage lives in NHWC buffers [B, H, W, 2c] and nothing is
split, concatenated, rolled or partitioned: conv1_1, both 3x3 convs (ReLU and
the conv half's residual in the epilogue) and conv1_2 (the block's residual
in the epilogue) run on ops.conv_ragged over channel slices, writing the
conv half of the cat buffer in place. The transformer half reads its slice of
conv1_1's output: at c = 32 and 64 ops.window_attn_block computes LN1, QKV,
attention, proj, the residual and LN2 in one kernel; at c = 128 and 256 the
same is composed from ops.layer_norm, the library GEMMs, ops.attention_swin
and ops.add_layer_norm. ops.swin_mlp closes it at every width; its output is
copied into the transformer half of the cat buffer (the MLP kernel writes
contiguous rows). The head, the tail, the 2x2 stride-2 convs and the
transposed convs stay on the library.
"""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .esrgan import MAX_INPUT_PIXELS

WINDOW = ops.SWIN_WINDOW
HEAD_DIM = ops.WINDOW_BLOCK_HEAD
PAD_TO = 64

_SUPPORTED = (
    "supported: SCUNet .safetensors (scunet_color_real_gan / "
    "scunet_color_real_psnr and same-shaped models): 3-channel input, window "
    "8, head dim 32, seven stages of any depth, dim 64. Not supported: "
    "other windows, head dims or widths, grayscale models, .pth files, DAT"
)


def _cached(mod: nn.Module, name: str, src, build):
    """build() cached on the module per version of the source tensors (like
    SDConv2d._wprep)."""
    key = tuple((t.data_ptr(), t._version, t.dtype) for t in src)
    cache = getattr(mod, name, None)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            cache = (key, build())
        setattr(mod, name, cache)
    return cache[1]


def _ragged(conv: nn.Conv2d) -> torch.Tensor:
    return _cached(conv, "_ragged_cache", (conv.weight,),
                   lambda: ops.conv_ragged_prepare(conv.weight))


def _f32(mod: nn.Module):
    return _cached(mod, "_f32_cache", (mod.weight, mod.bias),
                   lambda: (mod.weight.float().contiguous(),
                            mod.bias.float().contiguous()))


class WMSA(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.dim, self.heads = dim, dim // HEAD_DIM
        self.scale = HEAD_DIM ** -0.5
        self.embedding_layer = nn.Linear(dim, 3 * dim)
        self.relative_position_params = nn.Parameter(
            torch.zeros(self.heads, 2 * WINDOW - 1, 2 * WINDOW - 1))
        self.linear = nn.Linear(dim, dim)

    def prepared(self):
        """(wqkv_p, bqkv, rel, wp_p, bp): the staged weights of
        ops.window_attn_block and fp32 vectors."""
        e, lin, rel = self.embedding_layer, self.linear, \
            self.relative_position_params

        def build():
            wq, wp = ops.window_attn_block_prepare(e.weight, lin.weight)
            return (wq, e.bias.float().contiguous(), rel.float().contiguous(),
                    wp, lin.bias.float().contiguous())

        return _cached(self, "_prep_cache",
                       (e.weight, e.bias, rel, lin.weight, lin.bias), build)

    def gathered_bias(self) -> torch.Tensor:
        """[heads, 64, 64] fp32: rel gathered by `relation`, what
        ops.attention_swin reads at the widths the fused kernel leaves."""
        def build():
            c = torch.tensor([[i, j] for i in range(WINDOW)
                              for j in range(WINDOW)],
                             device=self.relative_position_params.device)
            r = c[:, None, :] - c[None, :, :] + WINDOW - 1
            return self.relative_position_params.float()[
                :, r[:, :, 0], r[:, :, 1]].contiguous()

        return _cached(self, "_bias_cache", (self.relative_position_params,),
                       build)


class Block(nn.Module):
    """trans_block: x + msa(ln1 x), then x + mlp(ln2 x), on [B, H, W, c]."""

    def __init__(self, dim: int, shift: int):
        super().__init__()
        self.shift = shift
        self.ln1 = nn.LayerNorm(dim)
        self.msa = WMSA(dim)
        self.ln2 = nn.LayerNorm(dim)
        self.mlp = nn.Sequential(nn.Linear(dim, 4 * dim), nn.GELU(),
                                 nn.Linear(4 * dim, dim))

    def _attn_args(self, native: bool):
        m = self.msa
        if native:
            wq, bq, rel, wp, bp = m.prepared()
            return (*_f32(self.ln1), wq, bq, rel, wp, bp, *_f32(self.ln2))
        return (self.ln1.weight, self.ln1.bias, m.embedding_layer.weight,
                m.embedding_layer.bias, m.relative_position_params,
                m.linear.weight, m.linear.bias, self.ln2.weight, self.ln2.bias)

    def mlp_prepared(self):
        fc1, fc2 = self.mlp[0], self.mlp[2]
        src = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
        return _cached(self, "_mlp_cache", src,
                       lambda: tuple(ops.swin_mlp_prepare(*src)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The plain route."""
        y, n2 = ops.window_attn_block(x, *self._attn_args(False),
                                      self.msa.scale, self.shift,
                                      self.ln1.eps, native=False)
        return y + self.mlp(n2)

    def attention_native(self, x: torch.Tensor, fused: bool):
        """(y, LN2(y)) of the attention half, contiguous, for a bf16 view x:
        one kernel where ops.window_attn_block takes the width and `fused`
        allows it, else the five-launch composed route."""
        m = self.msa
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        n2 = torch.empty_like(y)
        if fused and ops.window_attn_block_supported(x, y, n2):
            return ops.window_attn_block(
                x, *self._attn_args(True), m.scale, self.shift, self.ln1.eps,
                out=(y, n2))
        b, h, w, c = x.shape
        xc = x.contiguous()
        n1 = ops.layer_norm(xc, *_f32(self.ln1), self.ln1.eps)
        qkv = F.linear(n1, m.embedding_layer.weight, m.embedding_layer.bias)
        a = ops.attention_swin(qkv.view(b, h, w, 3, m.heads, HEAD_DIM),
                               m.gathered_bias(), m.scale, self.shift)
        p = F.linear(a, m.linear.weight, m.linear.bias)
        return ops.add_layer_norm(p, xc, *_f32(self.ln2), self.ln2.eps)


class ConvTransBlock(nn.Module):
    def __init__(self, dim: int, shift: int):
        super().__init__()
        self.dim = dim
        self.conv1_1 = nn.Conv2d(2 * dim, 2 * dim, 1)
        self.conv_block = nn.Sequential(
            nn.Conv2d(dim, dim, 3, padding=1, bias=False), nn.ReLU(),
            nn.Conv2d(dim, dim, 3, padding=1, bias=False))
        self.trans_block = Block(dim, shift)
        self.conv1_2 = nn.Conv2d(2 * dim, 2 * dim, 1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The plain route, NCHW."""
        conv_x, trans_x = torch.split(self.conv1_1(x), self.dim, dim=1)
        conv_x = self.conv_block(conv_x) + conv_x
        trans_x = self.trans_block(trans_x.permute(0, 2, 3, 1))
        res = self.conv1_2(torch.cat((conv_x, trans_x.permute(0, 3, 1, 2)),
                                     dim=1))
        return x + res

    def forward_native(self, x, a, cat, t, out, fused: bool):
        """x, a, cat, out: NCHW views of NHWC [B, H, W, 2c] buffers, t of a
        [B, H, W, c] one. Returns out = x + conv1_2(cat)."""
        c = self.dim
        ops.conv_ragged(x, _ragged(self.conv1_1), self.conv1_1.bias, a,
                        ksize=1)
        ops.conv_ragged(a[:, :c], _ragged(self.conv_block[0]), None, t,
                        ksize=3, lrelu=0.0)
        ops.conv_ragged(t, _ragged(self.conv_block[2]), None, cat[:, :c],
                        ksize=3, res=a[:, :c])
        blk = self.trans_block
        y, n2 = blk.attention_native(a[:, c:].permute(0, 2, 3, 1), fused)
        s, _ = ops.swin_mlp(n2, y, *blk.mlp_prepared())
        cat[:, c:].copy_(s.permute(0, 3, 1, 2))
        return ops.conv_ragged(cat, _ragged(self.conv1_2), self.conv1_2.bias,
                               out, ksize=1, res=x)


class SCUNet(nn.Module):
    """SCUNet(in_nc, config, dim): [N, 3, H, W] in 0..1 -> [N, 3, H, W]."""

    scale = 1
    # the native route runs the attention half at c = 32 and 64 on
    # ops.window_attn_block; False keeps the composed route there as well
    fused_attention = True

    def __init__(self, in_nc: int = 3, config=(4,) * 7, dim: int = 64):
        super().__init__()
        config = tuple(int(n) for n in config)
        if in_nc != 3 or len(config) != 7 or min(config) < 1 \
                or dim != 64:
            raise ValueError(f"SCUNet: in_nc {in_nc}, config {config}, dim "
                             f"{dim}; " + _SUPPORTED)
        self.config, self.dim = config, dim

        def blocks(c, n):
            return [ConvTransBlock(c, 0 if i % 2 == 0 else WINDOW // 2)
                    for i in range(n)]

        def down(c):
            return nn.Conv2d(c, 2 * c, 2, 2, bias=False)

        def up(c):
            return nn.ConvTranspose2d(c, c // 2, 2, 2, bias=False)

        self.m_head = nn.Sequential(nn.Conv2d(in_nc, dim, 3, padding=1,
                                              bias=False))
        self.m_down1 = nn.Sequential(*blocks(dim // 2, config[0]), down(dim))
        self.m_down2 = nn.Sequential(*blocks(dim, config[1]), down(2 * dim))
        self.m_down3 = nn.Sequential(*blocks(2 * dim, config[2]),
                                     down(4 * dim))
        self.m_body = nn.Sequential(*blocks(4 * dim, config[3]))
        self.m_up3 = nn.Sequential(up(8 * dim), *blocks(2 * dim, config[4]))
        self.m_up2 = nn.Sequential(up(4 * dim), *blocks(dim, config[5]))
        self.m_up1 = nn.Sequential(up(2 * dim), *blocks(dim // 2, config[6]))
        self.m_tail = nn.Sequential(nn.Conv2d(dim, in_nc, 3, padding=1,
                                              bias=False))

    def native_supported(self, x: torch.Tensor) -> bool:
        """True when forward(x) runs the blocks on the HIP kernels."""
        return bool(x.is_cuda and x.dtype == torch.bfloat16
                    and self.m_head[0].weight.dtype == torch.bfloat16
                    and ops.have_ext())

    def _stage(self, stage: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
        """A stage on the native route: library convs as they come, the
        blocks ping-ponging between two NHWC buffers."""
        bufs = None
        for m in stage:
            if not isinstance(m, ConvTransBlock):
                x = m(x).contiguous(memory_format=torch.channels_last)
                continue
            if bufs is None:
                x = x.contiguous(memory_format=torch.channels_last)
                n, c2, h, w = x.shape

                def nhwc(c):
                    return torch.empty((n, h, w, c), dtype=x.dtype,
                                       device=x.device).permute(0, 3, 1, 2)

                a, cat, t = nhwc(c2), nhwc(c2), nhwc(c2 // 2)
                bufs = [nhwc(c2), nhwc(c2)]
            out = bufs[0] if x.data_ptr() != bufs[0].data_ptr() else bufs[1]
            x = m.forward_native(x, a, cat, t, out, self.fused_attention)
        return x

    def _forward(self, x: torch.Tensor, native: bool) -> torch.Tensor:
        if native:
            x = x.contiguous(memory_format=torch.channels_last)
            run = self._stage
        else:
            def run(stage, t):
                return stage(t)
        x1 = run(self.m_head, x)
        x2 = run(self.m_down1, x1)
        x3 = run(self.m_down2, x2)
        x4 = run(self.m_down3, x3)
        x = run(self.m_body, x4)
        x = run(self.m_up3, x + x4)
        x = run(self.m_up2, x + x3)
        x = run(self.m_up1, x + x2)
        return run(self.m_tail, x + x1)

    def forward(self, x: torch.Tensor, native: bool = True) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("SCUNet: x must be [N, 3, H, W], got "
                             f"{tuple(x.shape)}")
        if x.shape[2] * x.shape[3] > MAX_INPUT_PIXELS:
            raise ValueError(
                f"SCUNet: input {x.shape[3]}x{x.shape[2]} exceeds the "
                "whole-image limit of 2048 x 2048 pixels (tiling is not built)"
            )
        h, w = x.shape[2:]
        ph, pw = -h % PAD_TO, -w % PAD_TO
        if ph or pw:
            x = F.pad(x, (0, pw, 0, ph), mode="replicate")
        out = self._forward(x, native and self.native_supported(x))
        return out[:, :, :h, :w]


_REL0 = "m_down1.0.trans_block.msa.relative_position_params"


def is_scunet_state_dict(keys) -> bool:
    """True when the tensor names are a SCUNet's."""
    keys = set(keys)
    return "m_head.0.weight" in keys and _REL0 in keys


def scunet_from_state_dict(state: Dict[str, torch.Tensor]) -> SCUNet:
    """Build a SCUNet from a KAIR state dict; config and dim are inferred
    from the tensors."""
    if not is_scunet_state_dict(state):
        raise ValueError("load_scunet: not a SCUNet state dict; " + _SUPPORTED)
    head, rel = state["m_head.0.weight"], state[_REL0]
    dim = int(head.shape[0])
    if head.dim() != 4 or head.shape[1] != 3:
        raise ValueError(f"load_scunet: m_head takes {head.shape[1]} "
                         "channels; " + _SUPPORTED)
    if rel.dim() != 3 or tuple(rel.shape[1:]) != (2 * WINDOW - 1,) * 2:
        raise ValueError(f"load_scunet: relative_position_params "
                         f"{tuple(rel.shape)} is not window {WINDOW}; "
                         + _SUPPORTED)
    if dim % 2 or rel.shape[0] * HEAD_DIM != dim // 2:
        raise ValueError(f"load_scunet: head dim {dim / 2 / rel.shape[0]:g} "
                         f"(dim {dim}, {rel.shape[0]} heads at the first "
                         "stage); " + _SUPPORTED)
    stages = ["m_down1", "m_down2", "m_down3", "m_body", "m_up3", "m_up2",
              "m_up1"]
    config: List[int] = [0] * 7
    for key in state:
        part = key.split(".")
        if part[0] in stages and len(part) > 2 and part[2] == "trans_block":
            i = stages.index(part[0])
            config[i] = max(config[i], int(part[1]) + (0 if i > 3 else 1))
    try:
        net = SCUNet(3, config, dim)
        net.load_state_dict(state, strict=True)
    except (RuntimeError, ValueError) as exc:
        raise ValueError(f"load_scunet: {exc}; " + _SUPPORTED) from None
    return net.eval()


def load_scunet(path: str) -> SCUNet:
    """Load a SCUNet upscaler from a .safetensors file."""
    if not str(path).endswith(".safetensors"):
        raise ValueError(f"load_scunet: '{path}' is not a .safetensors file; "
                         + _SUPPORTED)
    from safetensors.torch import load_file

    return scunet_from_state_dict(load_file(path))
