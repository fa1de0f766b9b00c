"""GPU tests for the norm path: register-resident add+LayerNorm, the
division-free GroupNorm apply, the tile-layout statistics kernel, add_gn and
the GroupNorm side channel through the UNet. Tolerances are the ones
tests/test_ops_gpu.py uses for the same ops.
"""
import pytest
import torch
import torch.nn.functional as F

from sdwd_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def relerr(out, ref):
    return ((out.float() - ref.float()).abs().max() /
            ref.float().abs().max().clamp_min(1e-6)).item()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _gn_ref(x, groups, w, b, silu):
    ref = F.group_norm(x.float(), groups, w.float(), b.float(), 1e-5)
    return F.silu(ref) if silu else ref


class TestAddLayerNormRegisters:
    # 8: one lane; 320/328: one partly filled vector slice per lane;
    # 520: lane 0 alone holds a second slice; 640: two slices; 1032 and
    # 1280: three, the last partly filled; 1536: three full slices.
    # R = 5 is not a multiple of the 4 rows per block.
    @pytest.mark.parametrize("D", [8, 320, 328, 520, 640, 1032, 1280, 1536])
    def test_sum_exact_ln_close(self, dev, D):
        torch.manual_seed(D)
        x = torch.randn(5, D, device=dev, dtype=torch.bfloat16)
        r = torch.randn_like(x)
        w = torch.randn(D, device=dev)
        b = torch.randn(D, device=dev)
        s, ln = ops.add_layer_norm(x, r, w, b)
        fsum = x.float() + r.float()
        assert torch.equal(s, fsum.to(torch.bfloat16))
        ref_ln = F.layer_norm(fsum, (D,), w, b, 1e-5)
        err = relerr(ln, ref_ln)
        print(f"add+LN D={D}: relerr {err:.3e}")
        assert err < 0.05


class TestGroupNormApply:
    # cg = 10 (vectors straddling groups), two columns per thread (C = 2560),
    # HW not a multiple of the row chunk, HW not a multiple of 128 (short
    # last tile), HW < 128, and one tile-eligible shape (HW = 128)
    @pytest.mark.parametrize("N,C,H,W,G", [
        (3, 320, 8, 8, 32),
        (2, 16, 16, 8, 2),
        (1, 2560, 8, 8, 32),
        (2, 64, 24, 24, 8),
        (1, 128, 40, 24, 32),
    ])
    @pytest.mark.parametrize("silu", [True, False])
    def test_vs_fp32(self, dev, N, C, H, W, G, silu):
        torch.manual_seed(C + H)
        x = _cl(torch.randn(N, C, H, W, device=dev, dtype=torch.bfloat16)
                * 1.5 + 0.3)
        w = torch.randn(C, device=dev)
        b = torch.randn(C, device=dev)
        out = ops.group_norm_silu(x, w, b, G, 1e-5, silu)
        assert out.is_contiguous(memory_format=torch.channels_last)
        err = relerr(out, _gn_ref(x, G, w, b, silu))
        print(f"GN apply {(N, C, H, W, G)} silu={silu}: relerr {err:.3e}")
        assert err < 0.03


class TestAddGn:
    @pytest.mark.parametrize("N,C,H,W,carries", [
        (2, 320, 16, 8, True),
        (2, 64, 16, 16, True),
        (1, 320, 8, 8, False),   # HW = 64: no 128-row tile
    ])
    def test_add_gn(self, dev, N, C, H, W, carries):
        torch.manual_seed(W)
        a = _cl(torch.randn(N, C, H, W, device=dev, dtype=torch.bfloat16))
        b = _cl(torch.randn(N, C, H, W, device=dev, dtype=torch.bfloat16))
        out = ops.add_gn(a, b)
        assert torch.equal(out, a + b)
        assert out.is_contiguous(memory_format=torch.channels_last)
        assert hasattr(out, "_sdwd_gnp") == carries
        if not carries:
            return
        gnp, tpi, _ = out._sdwd_gnp
        assert tpi == H * W // 128
        assert tuple(gnp.shape) == (N * tpi, 2, C)
        w = torch.randn(C, device=dev)
        bias = torch.randn(C, device=dev)
        fused = ops.group_norm_silu(out, w, bias, 32, 1e-5, True)
        std = ops.group_norm_silu(out.clone(), w, bias, 32, 1e-5, True)
        assert (fused.float() - std.float()).abs().max() <= 0.05
        err = relerr(fused, _gn_ref(out, 32, w, bias, True))
        print(f"add_gn {(N, C, H, W)}: relerr {err:.3e}")
        assert err < 0.03

    def test_strided_operand_falls_back(self, dev):
        a = torch.randn(2, 64, 16, 16, device=dev, dtype=torch.bfloat16)
        b = _cl(torch.randn_like(a))
        out = ops.add_gn(a, b)      # a is NCHW-contiguous: plain add
        assert torch.equal(out, a + b)
        assert not hasattr(out, "_sdwd_gnp")


class TestTileStats:
    def test_matches_direct_sums(self, dev):
        """The partial layout itself: [N*HW/128][2][C] sums over 128-row
        tiles, against a direct fp32 reduction."""
        torch.manual_seed(4)
        x = _cl(torch.randn(2, 320, 16, 16, device=dev,
                            dtype=torch.bfloat16))
        gnp = ops.ext().gn_tile_stats(x)
        rows = x.permute(0, 2, 3, 1).reshape(4, 128, 320).float()
        assert tuple(gnp.shape) == (4, 2, 320)
        # 128 fp32 adds of O(1) values: ~1e-5 relative
        assert torch.allclose(gnp[:, 0], rows.sum(1), rtol=1e-4, atol=1e-3)
        assert torch.allclose(gnp[:, 1], (rows * rows).sum(1),
                              rtol=1e-4, atol=1e-3)

    def test_missing_partials_are_attached_once(self, dev, monkeypatch):
        x = _cl(torch.randn(1, 64, 16, 16, device=dev, dtype=torch.bfloat16))
        w = torch.randn(64, device=dev)
        b = torch.randn(64, device=dev)
        mod = ops.ext()
        calls = []
        orig = mod.gn_tile_stats
        monkeypatch.setattr(
            mod, "gn_tile_stats", lambda t: calls.append(1) or orig(t)
        )
        first = ops.group_norm_silu(x, w, b, 32)
        assert hasattr(x, "_sdwd_gnp")
        second = ops.group_norm_silu(x, w, b, 32)
        assert len(calls) == 1
        assert torch.equal(first, second)
        x.add_(1.0)                 # in-place write invalidates the cache
        ops.group_norm_silu(x, w, b, 32)
        assert len(calls) == 2


class TestOneSidedConcat:
    def test_concat_carries_partials(self, dev):
        """a comes from a conv with partials, b from nowhere: the concat
        still carries partials, and group 21 (cg = 3 over 64 + 32 channels)
        straddles the boundary."""
        torch.manual_seed(6)
        x = _cl(torch.randn(2, 64, 16, 16, device=dev, dtype=torch.bfloat16))
        conv = torch.nn.Conv2d(64, 64, 3, padding=1).to(dev, torch.bfloat16)
        wprep = conv.weight.permute(0, 2, 3, 1).contiguous()
        a = ops.conv3x3(x, wprep, conv.bias, None, 1, collect_gn=True)
        assert hasattr(a, "_sdwd_gnp")
        b = _cl(torch.randn(2, 32, 16, 16, device=dev, dtype=torch.bfloat16))
        cat = ops.cat_channels_gn(a, b)
        assert torch.equal(cat, torch.cat([a, b], dim=1))
        assert hasattr(cat, "_sdwd_gnp")
        assert tuple(cat._sdwd_gnp[0].shape) == (4, 2, 96)
        w = torch.randn(96, device=dev)
        bias = torch.randn(96, device=dev)
        out = ops.group_norm_silu(cat, w, bias, 32, 1e-5, True)
        err = relerr(out, _gn_ref(cat, 32, w, bias, True))
        print(f"one-sided concat: relerr {err:.3e}")
        assert err < 0.03


class TestUNetSideChannel:
    def test_one_stats_read_per_forward(self, dev, monkeypatch):
        """Every GroupNorm of a tile-eligible UNet gets its statistics from
        a producer; only the stem conv's output is read for them."""
        from sdwd_amd.models.unet import UNetConfig, UNetModel

        torch.manual_seed(0)
        cfg = UNetConfig(
            model_channels=64, channel_mult=[1, 2], num_res_blocks=1,
            transformer_depth=[1, 1], context_dim=64, num_heads=2, groups=32,
        )
        net = UNetModel(cfg).to(dev, torch.bfloat16).eval()
        x = torch.randn(2, 4, 32, 32, device=dev, dtype=torch.bfloat16)
        t = torch.full((2,), 500.0, device=dev)
        ctx = torch.randn(2, 77, 64, device=dev, dtype=torch.bfloat16)

        mod = ops.ext()
        calls = []
        orig = mod.gn_tile_stats
        monkeypatch.setattr(
            mod, "gn_tile_stats", lambda v: calls.append(1) or orig(v)
        )
        with torch.no_grad():
            out = net(x, t, ctx)
        assert torch.isfinite(out.float()).all()
        print(f"stats reads per forward: {len(calls)}")
        assert len(calls) <= 1

        # same forward with the side channel cut: every GroupNorm reads
        # its input for the statistics instead
        monkeypatch.setattr(ops, "_attach_gn_partials", lambda y, g: None)
        calls.clear()
        with torch.no_grad():
            ref = net(x, t, ctx)
        assert len(calls) > 1
        err = relerr(out, ref)
        print(f"side channel vs none: relerr {err:.3e}")
        assert err < 0.05
