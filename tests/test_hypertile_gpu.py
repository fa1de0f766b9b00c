"""GPU tests of Hypertile: flash_fwd_bf16_v3's windowed addressing mode
(ops.attention_window_bshd) against the fp64 oracle of
tests/attention_oracle.py and against v3 itself on materialised window
copies, then the transformer block and a whole-step graphed generation.

q/k/v are strided slices of one [B, S, 3*H*D] tensor, as CrossAttention
makes them from its fused QKV GEMM. The windowed kernel walks the same 64-key
tiles in the same order with the same arithmetic as v3 on a window's
contiguous copy, so the two are compared bit for bit; the oracle's v3 bound
(exact=False: the default scale is no power of two) is applied per window.
"""
import pytest
import torch

import attention_oracle as A
from sdwd_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _qkv(b, s, h, d, seed, dev=None):
    """Strided q, k, v views [B, S, H, D] of one [B, S, 3*H*D] bf16 tensor."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b, s, 3 * h * d, generator=g).bfloat16()
    if dev is not None:
        qkv = qkv.to(dev)
    c = h * d
    return tuple(qkv[..., i * c:(i + 1) * c].unflatten(-1, (h, d))
                 for i in range(3))


def _fused(q, k, v, dev):
    """Contiguous [B, S, H, D] q, k, v -> strided views of one fused tensor."""
    b, s, h, d = q.shape
    qkv = torch.cat([t.reshape(b, s, h * d) for t in (q, k, v)], -1).to(dev)
    c = h * d
    return tuple(qkv[..., i * c:(i + 1) * c].unflatten(-1, (h, d))
                 for i in range(3))


# (grid, window, D, B, H): what each one reaches is in the issue's list
CASES = [
    pytest.param((8, 8), (4, 4), 40, 2, 2, id="8x8-4x4-d40"),        # window < one key tile, 4 windows
    pytest.param((40, 48), (20, 24), 40, 2, 2, id="40x48-20x24-d40"),  # tw !| 64, 480 tokens: ragged tile and q block
    pytest.param((32, 48), (32, 16), 64, 2, 2, id="32x48-32x16-d64"),  # tw | 64, nh = 1, nw = 3
    pytest.param((50, 25), (25, 25), 64, 2, 2, id="50x25-25x25-d64"),  # odd width, 625 tokens: 3 q blocks
    pytest.param((16, 192), (16, 96), 80, 2, 2, id="16x192-16x96-d80"),  # tw > 64
    pytest.param((16, 128), (16, 64), 160, 2, 2, id="16x128-16x64-d160"),  # 128-row blocks
    pytest.param((64, 64), (32, 32), 40, 1, 1, id="64x64-32x32-d40"),  # the shipped case
]


@pytest.mark.parametrize("grid,window,d,b,h", CASES)
def test_windowed_kernel(dev, grid, window, d, b, h):
    gh, gw = grid
    q, k, v = _qkv(b, gh * gw, h, d, seed=gh * 1000 + gw + d, dev=dev)
    assert ops.attention_window_supported(q, k, v)
    assert not q.is_contiguous()
    dpad, rows = ops.ext().attention_window_plan(d)
    assert dpad == (d + 15) // 16 * 16 and rows == (256 if dpad <= 96 else 128)

    out = ops.attention_window_bshd(q, k, v, grid=grid, window=window)
    assert out.shape == (b, gh * gw, h, d) and out.dtype == torch.bfloat16
    # every row finite and written: the whole tensor, not a sample
    assert torch.isfinite(out.float()).all()

    # bit-equal to v3 on materialised window copies, scattered back
    qw, kw, vw = (ops.window_split(t, grid, window).contiguous()
                  for t in (q, k, v))
    ref = ops.window_merge(
        ops.attention_bshd(qw, kw, vw, variant="v3"), grid, window)
    assert torch.equal(out, ref)

    # the oracle's v3 bound per window, at the default scale
    ow = ops.window_split(out, grid, window)
    orc = A.Oracle(qw.permute(0, 2, 1, 3), kw.permute(0, 2, 1, 3),
                   vw.permute(0, 2, 1, 3), A.default_scale(d))
    worst = orc.worst(ow.permute(0, 2, 1, 3), exact=False)
    print(f"grid {grid} window {window} D={d}: worst err/bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("d", [40, 64, 160])
def test_whole_grid_window_is_plain_v3(dev, d):
    # 320 keys: the measured dispatch of attention_bshd is v3 at every head
    # dim from 256 keys on, so "what attention_bshd returns" is v3's output
    q, k, v = _qkv(2, 16 * 20, 2, d, seed=d, dev=dev)
    out = ops.attention_window_bshd(q, k, v, grid=(16, 20), window=(16, 20))
    assert torch.equal(out, ops.attention_bshd(q, k, v, variant="v3"))
    assert torch.equal(out, ops.attention_bshd(q, k, v))


def test_rescale_under_window_addressing(dev):
    """The ramp inputs of the oracle module, one set per window of a 2x2
    split (10x20 windows: 200 tokens, four key tiles, the last ragged, tw
    dividing nothing), so v3's defer-max rescale branch runs on windowed
    addresses. The scale is exact, hence exact=True as in the v3 tests."""
    grid, window, d, h = (20, 40), (10, 20), 40, 2
    s = window[0] * window[1]
    per_window = [A.rescale_inputs("ramp", d, sq=s, sk=s, h=h, seed=w)
                  for w in range(4)]
    scale = per_window[0][3]
    # [4 windows, S, H, D] -> the grid's token order, batch 1
    qw, kw, vw = (torch.stack([p[i].permute(1, 0, 2) for p in per_window])
                  for i in range(3))
    orc = A.Oracle(qw.permute(0, 2, 1, 3), kw.permute(0, 2, 1, 3),
                   vw.permute(0, 2, 1, 3), scale)
    for w in range(4):
        for hh in range(h):
            assert A.tile_walk(orc.s[w, hh])["triggers"] > 0
    q, k, v = _fused(*(ops.window_merge(t, grid, window)
                       for t in (qw, kw, vw)), dev)
    out = ops.attention_window_bshd(q, k, v, grid=grid, window=window,
                                    scale=scale)
    ow = ops.window_split(out, grid, window).permute(0, 2, 1, 3)
    worst = orc.worst(ow, exact=True)
    print(f"rescale through windows: worst err/bound {worst:.3f}")
    assert worst <= 1.0
    ref = ops.attention_bshd(qw.to(dev), kw.to(dev), vw.to(dev), scale,
                             variant="v3")
    assert torch.equal(out, ops.window_merge(ref, grid, window))


def test_bad_arguments_raise(dev):
    q, k, v = _qkv(1, 64, 2, 40, seed=1, dev=dev)
    with pytest.raises(ValueError, match="window"):
        ops.attention_window_bshd(q, k, v, grid=(8, 8), window=(3, 4))
    with pytest.raises(ValueError, match="grid"):
        ops.attention_window_bshd(q, k, v, grid=(8, 9), window=(4, 3))
    # the extension checks again, whatever the wrapper let through
    ext = ops.ext()
    with pytest.raises(RuntimeError, match="window width"):
        ext.attention_window_bshd(q, k, v, 8, 8, 4, 3, 0.1)
    with pytest.raises(RuntimeError, match="token count"):
        ext.attention_window_bshd(q, k, v, 8, 16, 4, 4, 0.1)
    q2, k2, v2 = (t[..., ::2] for t in _qkv(1, 64, 2, 80, seed=2, dev=dev))
    assert not ops.attention_window_supported(q2, k2, v2)
    with pytest.raises(RuntimeError, match="unit stride"):
        ext.attention_window_bshd(q2, k2, v2, 8, 8, 4, 4, 0.1)


def test_block_native_equals_copies(dev):
    """One level-0 BasicTransformerBlock at C = 320 (8 heads of 40), grid
    16x16 cut 2x2: the windowed kernel against the materialised windows."""
    from sdwd_amd.models.unet import BasicTransformerBlock, CrossAttention

    torch.manual_seed(31)
    blk = BasicTransformerBlock(320, 64, 8).to(dev, torch.bfloat16).eval()
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 256, 320, generator=g).bfloat16().to(dev)
    ctx = torch.randn(2, 7, 64, generator=g).bfloat16().to(dev)
    window = (16, 16, 8, 8)
    assert CrossAttention.window_native
    with torch.no_grad():
        native = blk(x, ctx, (16, 16), window)
        blk.attn1.window_native = False
        copies = blk(x, ctx, (16, 16), window)
        plain = blk(x, ctx, (16, 16))
    assert torch.isfinite(native.float()).all()
    assert torch.equal(native, copies)
    assert not torch.equal(native, plain)


def test_graphed_generation_equals_eager(dev, monkeypatch):
    """Tiny UNet widened to model_channels = 320 at 64x64 pixels: its VAE
    halves once, so level 0 is a 32x32 grid cut into 2x2 windows of 16x16.
    The whole-step graph replays what the eager run computes."""
    import zlib
    from dataclasses import replace

    from sdwd_amd.models.clip import CLIPTextEncoder
    from sdwd_amd.models.registry import ModelBundle, _seeded_init
    from sdwd_amd.models.unet import UNetConfig, UNetModel
    from sdwd_amd.models.vae import AutoencoderKL, VAEConfig
    from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

    def bundle():
        te = CLIPTextEncoder(d_model=64, layers=2, heads=2, max_len=77)
        cfg = UNetConfig.tiny()
        cfg.model_channels, cfg.num_heads = 320, 8
        unet = UNetModel(cfg)
        vae = AutoencoderKL(VAEConfig.tiny())
        for off, m in enumerate((te, unet, vae)):
            _seeded_init(m, zlib.crc32(b"tiny-320") % (2 ** 31) + off)
        b = ModelBundle("tiny-320", te, None, unet, vae, context_dim=64)
        return b.eval().to(dev, torch.bfloat16)

    req = PipelineRequest(prompt="tiled cow", steps=3, width=64, height=64,
                          seeds=[5, 6], hypertile_unet=True)
    seen = []
    windowed = ops.attention_window_bshd

    def spy(q, k, v, grid, window, scale=None, native=True):
        seen.append((tuple(grid), tuple(window), native,
                     ops.attention_window_supported(q, k, v)))
        return windowed(q, k, v, grid, window, scale, native)

    monkeypatch.setenv("SDWD_HIPGRAPH", "0")
    eager = StableDiffusionPipeline(bundle(), device=dev)
    with monkeypatch.context() as m:
        m.setattr(ops, "attention_window_bshd", spy)
        a = eager.generate(req)
    assert seen and all(s == ((32, 32), (16, 16), True, True) for s in seen)
    assert "Hypertile U-Net: True" in a.infotexts[0]
    off = eager.generate(replace(req, hypertile_unet=False))
    assert not torch.equal(a.images, off.images)
    assert "Hypertile" not in off.infotexts[0]

    monkeypatch.setenv("SDWD_HIPGRAPH", "1")
    graphed = StableDiffusionPipeline(bundle(), device=dev)
    b = graphed.generate(req)
    caches = list(graphed._wholestep_cache.values())
    assert caches and all(g.cache and not g.failed for g in caches)
    assert torch.equal(a.images, b.images)
    assert torch.equal(b.images, graphed.generate(req).images)
