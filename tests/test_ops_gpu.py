"""GPU numerics tests: every HIP kernel vs a plain PyTorch fp32 reference
of the same op (SURVEY.md §4 kernel tier). All marked gpu; they fail loudly
if the extension is missing (no eager fallback on GPU by design).
"""
import math

import pytest
import torch

from sdwd_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def relerr(out, ref):
    return ((out.float() - ref.float()).abs().max() /
            ref.float().abs().max().clamp_min(1e-6)).item()


class TestExtensionLoads:
    def test_ext_present(self):
        # the load must come from the in-tree .so, not a silent fallback
        assert ops.have_ext(), "HIP extension missing on a GPU box"
        mod = ops.ext()
        assert hasattr(mod, "attention_fwd")


class TestMfmaLayout:
    """Empirical check of the assumed MFMA fragment layouts (probe.hip)."""

    def test_32x32x16(self, dev):
        torch.manual_seed(0)
        A = torch.randn(32, 16, device=dev)
        B = torch.randn(16, 32, device=dev)
        C = ops.ext().probe_mfma32(A, B)
        ref = (A.bfloat16().float() @ B.bfloat16().float())
        assert relerr(C, ref) < 0.02, "32x32x16 fragment layout wrong"

    def test_16x16x32(self, dev):
        torch.manual_seed(1)
        A = torch.randn(16, 32, device=dev)
        B = torch.randn(32, 16, device=dev)
        C = ops.ext().probe_mfma16(A, B)
        ref = (A.bfloat16().float() @ B.bfloat16().float())
        assert relerr(C, ref) < 0.02, "16x16x32 fragment layout wrong"


class TestElementwise:
    def test_silu_bf16(self, dev):
        x = torch.randn(3, 1000, device=dev, dtype=torch.bfloat16)
        out = ops.silu(x)
        ref = torch.nn.functional.silu(x.float())
        assert relerr(out, ref) < 0.02

    def test_geglu_bf16(self, dev):
        x = torch.randn(5, 33, 256, device=dev, dtype=torch.bfloat16)
        out = ops.geglu(x)
        a, g = x.float().chunk(2, dim=-1)
        ref = a * torch.nn.functional.gelu(g)
        assert out.shape == (5, 33, 128)
        assert relerr(out, ref) < 0.02

    def test_geglu_odd_dim(self, dev):
        x = torch.randn(4, 10, device=dev, dtype=torch.bfloat16)
        out = ops.geglu(x)
        a, g = x.float().chunk(2, dim=-1)
        ref = a * torch.nn.functional.gelu(g)
        assert relerr(out, ref) < 0.02

    def test_euler_step(self, dev):
        x = torch.randn(2, 4, 64, 64, device=dev, dtype=torch.bfloat16)
        den = torch.randn_like(x)
        out = ops.euler_step(x, den, 14.6, 10.0)
        d = (x.float() - den.float()) / 14.6
        ref = x.float() + d * (10.0 - 14.6)
        assert relerr(out, ref) < 0.02

    def test_axpby_f32(self, dev):
        x = torch.randn(999, device=dev)
        y = torch.randn(999, device=dev)
        out = ops.add_noise(x, y, 0.3, 1.7)
        assert relerr(out, 0.3 * x + 1.7 * y) < 1e-5


class TestNorms:
    @pytest.mark.parametrize("shape,groups", [
        ((2, 320, 64, 64), 32),
        ((3, 128, 30, 30), 32),   # odd HW -> scalar path
        ((2, 32, 8, 8), 8),
    ])
    def test_group_norm_silu(self, dev, shape, groups):
        x = torch.randn(*shape, device=dev, dtype=torch.bfloat16)
        w = torch.randn(shape[1], device=dev)
        b = torch.randn(shape[1], device=dev)
        out = ops.group_norm_silu(x, w, b, groups)
        ref = torch.nn.functional.silu(
            torch.nn.functional.group_norm(x.float(), groups, w, b, 1e-5)
        )
        assert relerr(out, ref) < 0.05

    def test_group_norm_no_silu(self, dev):
        x = torch.randn(2, 64, 16, 16, device=dev, dtype=torch.bfloat16)
        w = torch.ones(64, device=dev)
        b = torch.zeros(64, device=dev)
        out = ops.group_norm(x, w, b, 32)
        ref = torch.nn.functional.group_norm(x.float(), 32, w, b, 1e-5)
        assert relerr(out, ref) < 0.05

    @pytest.mark.parametrize("D", [64, 320, 768, 1280, 77])
    def test_layer_norm(self, dev, D):
        x = torch.randn(4, 100, D, device=dev, dtype=torch.bfloat16)
        w = torch.randn(D, device=dev)
        b = torch.randn(D, device=dev)
        out = ops.layer_norm(x, w, b)
        ref = torch.nn.functional.layer_norm(x.float(), (D,), w, b, 1e-5)
        assert relerr(out, ref) < 0.05


class TestAttention:
    @pytest.mark.parametrize("B,H,Sq,Sk,D", [
        (2, 8, 256, 256, 40),    # SD1.5 level-3 self-attn shape class
        (2, 8, 1024, 1024, 80),  # level-2
        (1, 8, 256, 256, 160),   # level-1 (and mid)
        (2, 8, 64, 64, 160),     # mid-block
        (2, 8, 256, 77, 40),     # cross-attn (ragged kv tile)
        (1, 10, 128, 128, 64),   # SDXL head shape
        (1, 1, 100, 100, 32),    # ragged q & kv
        (1, 1, 64, 64, 512),     # VAE mid (fallback path)
    ])
    def test_vs_fp32_reference(self, dev, B, H, Sq, Sk, D):
        torch.manual_seed(42)
        q = torch.randn(B, H, Sq, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn(B, H, Sk, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(B, H, Sk, D, device=dev, dtype=torch.bfloat16)
        scale = 1.0 / math.sqrt(D)
        out = ops.attention(q, k, v)
        s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
        ref = torch.matmul(s.softmax(dim=-1), v.float())
        err = relerr(out, ref)
        assert err < 0.04, f"attention err {err} at D={D}"

    def test_spiked_scores_rescale(self, dev):
        """One late key built from q.mean(dim=2) * 10. That is a mean over
        256 random rows (sigma ~0.66 per element), an ordinary key: the
        running max grows ~4 log2 units at the last tile, under v3's
        defer-max threshold of 8, so no rescale after tile 0 fires. Kept as
        a plain random-data case; the rescale path itself is tested by
        tests/test_attention_gpu.py::TestRescale."""
        B, H, S, D = 1, 2, 256, 80
        q = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16)
        k[:, :, -1] = q.mean(dim=2) * 10
        scale = 1.0 / math.sqrt(D)
        out = ops.attention(q, k, v)
        s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
        ref = torch.matmul(s.softmax(dim=-1), v.float())
        assert relerr(out, ref) < 0.04

    def test_row_softmax(self, dev):
        x = torch.randn(64, 300, device=dev)
        ref = torch.softmax(x * 0.5, dim=-1)
        ops.ext().row_softmax_(x, 0.5)
        assert relerr(x, ref) < 1e-4


class TestPipelineGPU:
    def test_tiny_txt2img_on_gpu(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        res = pipe.generate(
            PipelineRequest(prompt="gpu cow", steps=3, width=64, height=64,
                            seeds=[5, 6])
        )
        assert res.images.shape == (2, 64, 64, 3)
        assert torch.isfinite(res.images.float()).all()

    def test_whole_step_graph_matches_eager(self, dev, monkeypatch):
        """The whole-step hipGraph (CFG + UNet + combine in one replay)
        must reproduce the eager images bit-for-bit-ish across steps AND
        across a second generation that re-binds new conditioning."""
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        base = dict(prompt="graphed", steps=3, width=64, height=64,
                    seeds=[11], cfg_scale=7.0)
        monkeypatch.setenv("SDWD_HIPGRAPH", "0")
        eager = StableDiffusionPipeline("tiny", device=dev)
        a = eager.generate(PipelineRequest(**base)).images
        a2 = eager.generate(
            PipelineRequest(**{**base, "prompt": "other"})
        ).images
        monkeypatch.setenv("SDWD_HIPGRAPH", "1")
        graphed = StableDiffusionPipeline("tiny", device=dev)
        b = graphed.generate(PipelineRequest(**base)).images
        # second generation re-binds conditioning into the SAME graph
        b2 = graphed.generate(
            PipelineRequest(**{**base, "prompt": "other"})
        ).images
        assert (a.float() - b.float()).abs().max() <= 1.0
        assert (a2.float() - b2.float()).abs().max() <= 1.0
        assert not torch.equal(b, b2)  # conditioning rebind took effect

    @pytest.mark.parametrize("sampler", ["Heun", "DPM2", "DPM++ 2M", "UniPC"])
    def test_graph_multi_eval_samplers(self, dev, monkeypatch, sampler):
        """Multi-eval samplers hold the FIRST model eval's eps across the
        second replay - the graph out-buffer must not alias (regression:
        the static buffer was returned uncloned)."""
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        base = dict(prompt="ms", steps=3, width=64, height=64, seeds=[3],
                    sampler_name=sampler, cfg_scale=7.0)
        monkeypatch.setenv("SDWD_HIPGRAPH", "0")
        a = StableDiffusionPipeline("tiny", device=dev).generate(
            PipelineRequest(**base)
        ).images
        monkeypatch.setenv("SDWD_HIPGRAPH", "1")
        b = StableDiffusionPipeline("tiny", device=dev).generate(
            PipelineRequest(**base)
        ).images
        assert (a.float() - b.float()).abs().max() <= 1.0, sampler

    def test_sd15_one_step(self, dev):
        """One real SD1.5 denoise step at 512x512 (bf16)."""
        from sdwd_amd.models import load_model

        m = load_model("sd15", device=dev, dtype=torch.bfloat16, cache=False)
        x = torch.randn(2, 4, 64, 64, device=dev, dtype=torch.bfloat16)
        t = torch.full((2,), 500.0, device=dev)
        ctx = torch.randn(2, 77, 768, device=dev, dtype=torch.bfloat16)
        with torch.no_grad():
            eps = m.unet(x, t, ctx)
        assert eps.shape == x.shape
        assert torch.isfinite(eps.float()).all()


class TestAttentionBSHD:
    @pytest.mark.parametrize("B,S,H,D", [
        (2, 256, 8, 40),
        (2, 1024, 8, 80),
        (1, 64, 8, 160),
        (3, 100, 2, 64),
    ])
    def test_bshd_vs_reference(self, dev, B, S, H, D):
        torch.manual_seed(7)
        q = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
        from sdwd_amd import ops as O

        out = O.attention_bshd(q, k, v)
        scale = 1.0 / math.sqrt(D)
        qp = q.permute(0, 2, 1, 3).float()
        kp = k.permute(0, 2, 1, 3).float()
        vp = v.permute(0, 2, 1, 3).float()
        s = torch.matmul(qp, kp.transpose(-1, -2)) * scale
        ref = torch.matmul(s.softmax(-1), vp).permute(0, 2, 1, 3)
        assert relerr(out, ref) < 0.04

    def test_bhsd_strided_no_copy(self, dev):
        """The [B,H,S,D] entry works on a transposed (non-contiguous) view."""
        B, S, H, D = 2, 128, 4, 80
        q = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn_like(q)
        v = torch.randn_like(q)
        qt = q.transpose(1, 2)  # [B,H,S,D] non-contiguous
        out = ops.attention(qt, k.transpose(1, 2), v.transpose(1, 2))
        ref = ops.attention(
            qt.contiguous(), k.transpose(1, 2).contiguous(),
            v.transpose(1, 2).contiguous(),
        )
        assert relerr(out, ref) < 1e-4


class TestGroupNormNHWC:
    @pytest.mark.parametrize("shape,groups", [
        ((2, 320, 64, 64), 32),
        ((4, 1280, 8, 8), 32),
        ((2, 128, 512, 512), 32),
        ((1, 2560, 16, 16), 32),
        ((2, 32, 16, 16), 8),
    ])
    def test_channels_last_matches_fp32(self, dev, shape, groups):
        x = torch.randn(*shape, device=dev, dtype=torch.bfloat16)
        xc = x.to(memory_format=torch.channels_last)
        w = torch.randn(shape[1], device=dev)
        b = torch.randn(shape[1], device=dev)
        out = ops.group_norm_silu(xc, w, b, groups)
        assert out.is_contiguous(memory_format=torch.channels_last)
        ref = torch.nn.functional.silu(
            torch.nn.functional.group_norm(x.float(), groups, w, b, 1e-5)
        )
        assert relerr(out.contiguous(), ref) < 0.05

    def test_nhwc_equals_nchw_path(self, dev):
        x = torch.randn(3, 64, 32, 32, device=dev, dtype=torch.bfloat16)
        w = torch.randn(64, device=dev)
        b = torch.randn(64, device=dev)
        a = ops.group_norm_silu(x, w, b, 32)
        c = ops.group_norm_silu(
            x.to(memory_format=torch.channels_last), w, b, 32
        ).contiguous()
        assert relerr(a, c) < 0.02


class TestConv3x3:
    @pytest.mark.parametrize("N,Cin,H,W,Cout,stride", [
        (2, 64, 16, 16, 64, 1),
        (2, 320, 32, 32, 320, 1),
        (1, 320, 64, 64, 320, 1),
        (2, 640, 17, 17, 320, 1),   # odd spatial
        (2, 320, 32, 32, 320, 2),   # downsample
        (1, 2560, 8, 8, 1280, 1),   # concat shape
        (1, 128, 96, 96, 40, 1),    # Cout not multiple of tile
        (2, 320, 15, 15, 192, 1),   # M remainder + small Cout
    ])
    def test_vs_conv2d(self, dev, N, Cin, H, W, Cout, stride):
        torch.manual_seed(3)
        x = torch.randn(N, Cin, H, W, device=dev, dtype=torch.bfloat16)
        conv = torch.nn.Conv2d(Cin, Cout, 3, stride=stride, padding=1)
        conv = conv.to(dev, torch.bfloat16)
        ref = torch.nn.functional.conv2d(
            x.float(), conv.weight.float(), conv.bias.float(),
            stride=stride, padding=1,
        )
        xc = x.contiguous(memory_format=torch.channels_last)
        wprep = conv.weight.permute(0, 2, 3, 1).contiguous()
        out = ops.conv3x3(xc, wprep, conv.bias, None, stride)
        err = relerr(out.contiguous(), ref)
        assert err < 0.05, f"conv err {err}"

    @pytest.mark.parametrize("N,Cin,H,W,Cout", [
        (2, 64, 16, 16, 64),      # UNet upsample shape class
        (1, 512, 24, 24, 512),    # VAE decoder up
        (1, 256, 33, 17, 128),    # odd spatial
    ])
    def test_fused_upsample_conv(self, dev, N, Cin, H, W, Cout):
        torch.manual_seed(7)
        x = torch.randn(N, Cin, H, W, device=dev, dtype=torch.bfloat16)
        conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1).to(dev, torch.bfloat16)
        up = torch.nn.functional.interpolate(
            x.float(), scale_factor=2, mode="nearest"
        )
        ref = torch.nn.functional.conv2d(
            up, conv.weight.float(), conv.bias.float(), padding=1
        )
        xc = x.contiguous(memory_format=torch.channels_last)
        wprep = conv.weight.permute(0, 2, 3, 1).contiguous()
        out = ops.ups2x_conv3x3(xc, wprep, conv.bias)
        err = relerr(out.contiguous(), ref)
        assert err < 0.05, f"ups2x conv err {err}"

    @pytest.mark.parametrize("N,Cin,H,W,Cout,stride", [
        (2, 4, 64, 64, 320, 1),    # UNet conv_in
        (2, 9, 64, 64, 320, 1),    # inpaint-model conv_in
        (1, 3, 96, 96, 128, 1),    # VAE encoder conv_in
        (1, 4, 64, 64, 512, 1),    # VAE decoder conv_in
        (1, 4, 33, 33, 320, 2),    # strided + odd spatial
    ])
    def test_smallcin_vs_conv2d(self, dev, N, Cin, H, W, Cout, stride):
        torch.manual_seed(5)
        x = torch.randn(N, Cin, H, W, device=dev, dtype=torch.bfloat16)
        conv = torch.nn.Conv2d(Cin, Cout, 3, stride=stride, padding=1)
        conv = conv.to(dev, torch.bfloat16)
        ref = torch.nn.functional.conv2d(
            x.float(), conv.weight.float(), conv.bias.float(),
            stride=stride, padding=1,
        )
        xc = x.contiguous(memory_format=torch.channels_last)
        wprep = conv.weight.permute(0, 2, 3, 1).contiguous()
        out = ops.conv3x3_small(xc, wprep, conv.bias, stride)
        err = relerr(out.contiguous(), ref)
        assert err < 0.05, f"smallcin conv err {err}"

    def test_gn_partials_match_standard(self, dev):
        """Conv-epilogue GN partials: the fused-stats GroupNorm must match
        the standard two-pass path (stats over the same stored values,
        different summation order only) and the fp32 reference."""
        torch.manual_seed(9)
        x = torch.randn(2, 64, 32, 32, device=dev, dtype=torch.bfloat16)
        conv = torch.nn.Conv2d(64, 64, 3, padding=1).to(dev, torch.bfloat16)
        xc = x.contiguous(memory_format=torch.channels_last)
        wprep = conv.weight.permute(0, 2, 3, 1).contiguous()
        y = ops.conv3x3(xc, wprep, conv.bias, None, 1, collect_gn=True)
        assert hasattr(y, "_sdwd_gnp"), "partials not attached"
        w = torch.randn(64, device=dev)
        b = torch.randn(64, device=dev)
        fused = ops.group_norm_silu(y, w, b, 8, 1e-5, True)
        std = ops.group_norm_silu(y.clone(), w, b, 8, 1e-5, True)
        assert (fused.float() - std.float()).abs().max() <= 0.05
        ref = torch.nn.functional.silu(
            torch.nn.functional.group_norm(
                y.float(), 8, w.float(), b.float()
            )
        )
        assert relerr(fused.contiguous(), ref) < 0.03
        # v4 path (big channels) + chan_bias/residual variants
        x2 = torch.randn(1, 320, 32, 32, device=dev, dtype=torch.bfloat16)
        c2 = torch.nn.Conv2d(320, 320, 3, padding=1).to(dev, torch.bfloat16)
        res = torch.randn_like(x2).contiguous(
            memory_format=torch.channels_last
        )
        y2 = ops.conv3x3(
            x2.contiguous(memory_format=torch.channels_last),
            c2.weight.permute(0, 2, 3, 1).contiguous(), c2.bias, res, 1,
            collect_gn=True, variant="v4",
        )
        assert hasattr(y2, "_sdwd_gnp")
        w2 = torch.randn(320, device=dev)
        b2 = torch.randn(320, device=dev)
        f2 = ops.group_norm_silu(y2, w2, b2, 32, 1e-5, True)
        ref2 = torch.nn.functional.silu(
            torch.nn.functional.group_norm(
                y2.float(), 32, w2.float(), b2.float()
            )
        )
        assert relerr(f2.contiguous(), ref2) < 0.03

    def test_fused_residual(self, dev):
        x = torch.randn(2, 64, 16, 16, device=dev, dtype=torch.bfloat16)
        res = torch.randn(2, 64, 16, 16, device=dev, dtype=torch.bfloat16)
        conv = torch.nn.Conv2d(64, 64, 3, padding=1).to(dev, torch.bfloat16)
        ref = torch.nn.functional.conv2d(
            x.float(), conv.weight.float(), conv.bias.float(), padding=1
        ) + res.float()
        xc = x.contiguous(memory_format=torch.channels_last)
        rc = res.contiguous(memory_format=torch.channels_last)
        wprep = conv.weight.permute(0, 2, 3, 1).contiguous()
        out = ops.conv3x3(xc, wprep, conv.bias, rc, 1)
        assert relerr(out.contiguous(), ref) < 0.05

    def test_sdconv_module_dispatch(self, dev):
        from sdwd_amd.models.layers import SDConv2d

        conv = SDConv2d(320, 320, 3, padding=1).to(dev, torch.bfloat16)
        x = torch.randn(2, 320, 32, 32, device=dev, dtype=torch.bfloat16)
        out = conv(x.contiguous(memory_format=torch.channels_last))
        ref = torch.nn.functional.conv2d(
            x.float(), conv.weight.float(), conv.bias.float(), padding=1
        )
        assert relerr(out.contiguous(), ref) < 0.05

    def test_sdconv_1x1_gemm(self, dev):
        from sdwd_amd.models.layers import SDConv2d

        conv = SDConv2d(320, 640, 1).to(dev, torch.bfloat16)
        x = torch.randn(2, 320, 16, 16, device=dev, dtype=torch.bfloat16)
        out = conv(x)
        ref = torch.nn.functional.conv2d(
            x.float(), conv.weight.float(), conv.bias.float()
        )
        assert relerr(out.contiguous(), ref) < 0.05

    def test_fused_chan_bias(self, dev):
        """Time-embedding projection as per-(sample,channel) epilogue bias."""
        x = torch.randn(3, 64, 16, 16, device=dev, dtype=torch.bfloat16)
        cb = torch.randn(3, 64, device=dev, dtype=torch.bfloat16)
        conv = torch.nn.Conv2d(64, 64, 3, padding=1).to(dev, torch.bfloat16)
        ref = torch.nn.functional.conv2d(
            x.float(), conv.weight.float(), conv.bias.float(), padding=1
        ) + cb.float()[:, :, None, None]
        xc = x.contiguous(memory_format=torch.channels_last)
        wprep = conv.weight.permute(0, 2, 3, 1).contiguous()
        out = ops.conv3x3(xc, wprep, conv.bias, None, 1, chan_bias=cb)
        assert relerr(out.contiguous(), ref) < 0.05


def _conv_case(dev, N, Cin, H, W, Cout, stride, extras=False, seed=11):
    """Inputs for one conv (channels_last x, prepared weight, bias, optional
    residual + chan_bias) and its fp32 F.conv2d reference."""
    torch.manual_seed(seed)
    x = torch.randn(N, Cin, H, W, device=dev, dtype=torch.bfloat16)
    conv = torch.nn.Conv2d(Cin, Cout, 3, stride=stride, padding=1)
    conv = conv.to(dev, torch.bfloat16)
    ref = torch.nn.functional.conv2d(
        x.float(), conv.weight.float(), conv.bias.float(),
        stride=stride, padding=1,
    )
    res = cb = None
    if extras:
        res = torch.randn_like(ref, dtype=torch.bfloat16).contiguous(
            memory_format=torch.channels_last
        )
        cb = torch.randn(N, Cout, device=dev, dtype=torch.bfloat16)
        ref = ref + res.float() + cb.float()[:, :, None, None]
    xc = x.contiguous(memory_format=torch.channels_last)
    wprep = conv.weight.permute(0, 2, 3, 1).contiguous()
    return xc, wprep, conv.bias, res, cb, ref


class TestConv3x3Variants:
    """The 256x256 v4 kernel forced at the smallest shapes that reach its
    edges (the default dispatch only picks it on grids of >= 256 tiles)."""

    def test_dispatch_table(self):
        # conv3x3_plan(N, H, W, Cin, Cout, stride, force) -> (full 256-col
        # v4 tiles, remainder cols on v2, remainder uses BN=64); host only
        plan = ops.ext().conv3x3_plan
        table = [
            # N, Cin, H, W, Cout, stride, force -> expected
            ((128, 320, 64, 64, 320, 1, 0), (1, 64, True)),
            ((128, 640, 32, 32, 640, 1, 0), (2, 128, False)),
            ((128, 960, 32, 32, 640, 1, 0), (2, 128, False)),
            ((16, 512, 64, 64, 512, 1, 0), (2, 0, None)),
            ((128, 1280, 16, 16, 1280, 1, 0), (0, 1280, False)),
            ((8, 320, 64, 64, 320, 1, 0), (0, 320, False)),
            ((2, 320, 32, 32, 320, 1, 0), (0, 320, True)),
            ((128, 320, 64, 64, 320, 1, 2), (0, 320, False)),
            ((1, 64, 17, 17, 320, 1, 4), (1, 64, True)),
        ]
        for (N, Cin, H, W, Cout, stride, force), want in table:
            got = tuple(plan(N, H, W, Cin, Cout, stride, force))
            if want[2] is None:  # no remainder launch: the flag is moot
                got, want = got[:2], want[:2]
            assert got == want, (N, Cin, H, W, Cout, stride, force, got)

    @pytest.mark.parametrize("N,Cin,H,W,Cout,stride,extras", [
        # 2 M-tiles (2nd: 33 live rows); one 256-col tile + 64-col v2 tail
        (1, 64, 17, 17, 320, 1, False),
        # one partial M-tile of 64 rows; 2 K-chunks/plane, 2 column tiles
        (1, 128, 16, 16, 512, 2, False),
        # residual + chan_bias together
        (2, 64, 16, 16, 256, 1, True),
    ])
    def test_v4_vs_conv2d(self, dev, N, Cin, H, W, Cout, stride, extras):
        xc, wprep, bias, res, cb, ref = _conv_case(
            dev, N, Cin, H, W, Cout, stride, extras
        )
        plan = ops.ext().conv3x3_plan(N, H, W, Cin, Cout, stride, 4)
        assert plan[0] == Cout // 256, "v4 was not reachable at this shape"
        outs = {}
        for variant in ("v4", "v2"):
            out = ops.conv3x3(
                xc, wprep, bias, res, stride, chan_bias=cb, variant=variant
            )
            outs[variant] = out
            err = relerr(out.contiguous(), ref)
            print(f"conv {variant} {(N, Cin, H, W, Cout, stride)} "
                  f"relerr {err:.3e}")
            assert err < 0.05, f"conv {variant} err {err}"
        print(f"v4 bit-equal to v2: {torch.equal(outs['v4'], outs['v2'])}")

    @pytest.mark.parametrize("N,Cin,H,W,Cout", [
        (2, 64, 16, 16, 256),   # 4 slots of 128 rows
        (1, 64, 16, 8, 256),    # M=128: the tile's second half is empty
    ])
    def test_v4_gn_partials(self, dev, N, Cin, H, W, Cout):
        xc, wprep, bias, _, _, _ = _conv_case(dev, N, Cin, H, W, Cout, 1)
        y = ops.conv3x3(
            xc, wprep, bias, None, 1, collect_gn=True, variant="v4"
        )
        assert hasattr(y, "_sdwd_gnp"), "partials not attached"
        gnp = y._sdwd_gnp[0]
        M = N * H * W
        assert tuple(gnp.shape) == (M // 128, 2, Cout)
        # sums over the STORED bf16 values of each slot's 128 rows
        v = y.permute(0, 2, 3, 1).reshape(M // 128, 128, Cout).double()
        s_ref, q_ref = v.sum(1), (v * v).sum(1)
        s_err = (gnp[:, 0].double() - s_ref).abs()
        q_err = (gnp[:, 1].double() - q_ref).abs()
        print(f"gn partial worst sum err/bound "
              f"{(s_err / (1e-4 * v.abs().sum(1))).max().item():.3e}, "
              f"sumsq err/bound {(q_err / (1e-4 * q_ref)).max().item():.3e}")
        assert (s_err <= 1e-4 * v.abs().sum(1)).all()
        assert (q_err <= 1e-4 * q_ref).all()
        w = torch.randn(Cout, device=dev)
        b = torch.randn(Cout, device=dev)
        fused = ops.group_norm_silu(y, w, b, 32, 1e-5, True)
        ref = torch.nn.functional.silu(
            torch.nn.functional.group_norm(
                y.float(), 32, w.float(), b.float()
            )
        )
        assert relerr(fused.contiguous(), ref) < 0.03

    def test_unknown_variant_raises(self, dev):
        xc, wprep, bias, _, _, _ = _conv_case(dev, 2, 64, 16, 16, 64, 1)
        with pytest.raises(ValueError):
            ops.conv3x3(xc, wprep, bias, None, 1, variant="bogus")

    def test_explicit_v2_equals_auto(self, dev):
        # a shape where the automatic dispatch is the v2 kernel
        xc, wprep, bias, _, _, _ = _conv_case(dev, 2, 64, 16, 16, 64, 1)
        auto = ops.conv3x3(xc, wprep, bias, None, 1, variant="auto")
        v2 = ops.conv3x3(xc, wprep, bias, None, 1, variant="v2")
        assert torch.equal(auto, v2)


class TestAddLayerNorm:
    @pytest.mark.parametrize("D", [320, 640, 1280])
    def test_fused_matches(self, dev, D):
        x = torch.randn(4, 64, D, device=dev, dtype=torch.bfloat16)
        r = torch.randn_like(x)
        w = torch.randn(D, device=dev)
        b = torch.randn(D, device=dev)
        s, ln = ops.add_layer_norm(x, r, w, b)
        ref_s = x.float() + r.float()
        ref_ln = torch.nn.functional.layer_norm(ref_s, (D,), w, b, 1e-5)
        assert relerr(s, ref_s) < 0.05
        assert relerr(ln, ref_ln) < 0.05


class TestCrossDeviceConsistency:
    def test_tiny_pipeline_gpu_matches_cpu(self, dev):
        """bf16 GPU pipeline vs fp32 CPU pipeline on the same request: same
        trajectory class (loose tolerance for precision differences)."""
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        req = PipelineRequest(prompt="xdev", steps=2, width=64, height=64,
                              seeds=[21], sampler_name="Euler")
        cpu = StableDiffusionPipeline("tiny", device="cpu").generate(req)
        gpu = StableDiffusionPipeline("tiny", device=dev).generate(req)
        diff = (cpu.images.float() - gpu.images.float()).abs()
        assert diff.mean() < 8.0, f"mean abs diff {diff.mean()} too high"

    @pytest.mark.parametrize("sampler", [
        "Euler a", "Heun", "DPM++ 2M", "DPM++ SDE", "DPM2 a", "UniPC",
        "LMS", "Restart", "DPM fast", "DPM adaptive", "LCM",
    ])
    def test_sampler_trajectory_gpu_matches_cpu(self, dev, sampler):
        """Per-sampler trajectory check (round-1 verdict: beyond
        finiteness): the bf16 GPU run of EACH sampler must land near its
        fp32 CPU trajectory — a wrong update rule on the fused GPU step
        kernels diverges far beyond precision noise."""
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        req = PipelineRequest(prompt="traj", steps=4, width=64, height=64,
                              seeds=[33], sampler_name=sampler)
        cpu = StableDiffusionPipeline("tiny", device="cpu").generate(req)
        gpu = StableDiffusionPipeline("tiny", device=dev).generate(req)
        diff = (cpu.images.float() - gpu.images.float()).abs()
        assert diff.mean() < 8.0, f"{sampler}: mean abs diff {diff.mean()}"


class TestLoRAGPU:
    def test_lora_on_gpu_pipeline(self, dev):
        """LoRA merge/unmerge through the GPU pipeline (also exercises the
        SDConv2d prepped-weight cache invalidation)."""
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        base = dict(steps=2, width=64, height=64, seeds=[3])
        plain = pipe.generate(PipelineRequest(prompt="cow", **base)).images
        lora = pipe.generate(
            PipelineRequest(prompt="cow <lora:gstyle:1.0>", **base)
        ).images
        plain2 = pipe.generate(PipelineRequest(prompt="cow", **base)).images
        assert not torch.equal(plain, lora)
        assert torch.equal(plain, plain2)


class TestInpaintingGPU:
    def test_mask_runs_on_gpu(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        init = torch.randint(0, 255, (1, 64, 64, 3), dtype=torch.uint8)
        lat = pipe.encode_image(init, seeds=[5])
        mask = torch.zeros(64, 64, dtype=torch.uint8)
        mask[:, 32:] = 255
        res = pipe.generate(
            PipelineRequest(prompt="gpu paint", steps=3, width=64, height=64,
                            seeds=[5], init_latents=lat, mask_image=mask)
        )
        assert res.images.shape == (1, 64, 64, 3)
        assert torch.isfinite(res.images.float()).all()

    def test_soft_inpainting_runs_on_gpu(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        init = torch.full((1, 64, 64, 3), 180, dtype=torch.uint8)
        lat = pipe.encode_image(init, seeds=[6])
        mask = torch.zeros(64, 64, dtype=torch.uint8)
        mask[:, 32:] = 255
        common = dict(prompt="soft", steps=3, width=64, height=64,
                      seeds=[6], init_latents=lat, mask_image=mask,
                      denoising_strength=1.0)
        hard = pipe.generate(PipelineRequest(**common)).images
        soft = pipe.generate(
            PipelineRequest(**common, soft_inpainting=True)
        ).images
        soft2 = pipe.generate(
            PipelineRequest(**common, soft_inpainting=True)
        ).images
        assert not torch.equal(hard, soft)
        assert torch.equal(soft, soft2)


class TestXLInpaintGPU:
    def test_tiny_xl_inpaint_generates(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny-xl-inpaint", device=dev)
        init = torch.full((1, 64, 64, 3), 120, dtype=torch.uint8)
        lat = pipe.encode_image(init, seeds=[2])
        mask = torch.zeros(64, 64, dtype=torch.uint8)
        mask[:, 32:] = 255
        res = pipe.generate(PipelineRequest(
            prompt="xl inpaint", steps=2, width=64, height=64, seeds=[2],
            init_latents=lat, mask_image=mask, denoising_strength=0.8,
        ))
        assert res.images.shape == (1, 64, 64, 3)
        assert torch.isfinite(res.images.float()).all()


class TestRefinerGPU:
    def test_refiner_lineage_on_gpu(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny-xl", device=dev)
        res = pipe.generate(PipelineRequest(
            prompt="refined", steps=3, width=64, height=64, seeds=[3],
            refiner_model="tiny-xl-refiner", refiner_switch_at=0.5,
        ))
        assert res.images.shape == (1, 64, 64, 3)
        assert torch.isfinite(res.images.float()).all()


class TestRegionalGPU:
    def test_regional_runs_and_differs(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        base = dict(steps=3, width=64, height=64, seeds=[21])
        plain = pipe.generate(
            PipelineRequest(prompt="sky", **base)
        ).images
        req = PipelineRequest(
            prompt="sky BREAK red tree BREAK blue lake",
            regional_mode="columns", regional_ratios="1,1",
            regional_base_ratio=0.2, **base,
        )
        a = pipe.generate(req)
        b = pipe.generate(req)
        assert torch.equal(a.images, b.images)
        assert not torch.equal(plain, a.images)
        assert "RP Active: True" in a.infotexts[0]


class TestDeterminismGPU:
    def test_same_request_same_images(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        req = PipelineRequest(prompt="det", steps=3, width=64, height=64,
                              seeds=[13, 14])
        a = pipe.generate(req).images
        b = pipe.generate(req).images
        assert torch.equal(a, b), "GPU pipeline must be run-to-run exact"


class TestAllSamplersGPU:
    def test_every_sampler_runs_on_gpu(self, dev):
        from sdwd_amd.pipeline import (
            PipelineRequest,
            StableDiffusionPipeline,
            sampler_names,
        )

        pipe = StableDiffusionPipeline("tiny", device=dev)
        for name in sampler_names():
            res = pipe.generate(
                PipelineRequest(prompt="s", steps=3, width=64, height=64,
                                seeds=[1], sampler_name=name)
            )
            assert torch.isfinite(res.images.float()).all(), name


class TestVaeDownsampleGPU:
    def test_asym_pad_encode_matches_cpu_fp32(self, dev):
        """VAE encode (ldm asymmetric-pad downsample) on GPU bf16 vs CPU
        fp32: the sampling grid must agree (only precision noise differs)."""
        from sdwd_amd.models import load_model
        from sdwd_amd.pipeline import StableDiffusionPipeline

        gp = StableDiffusionPipeline("tiny", device=dev)
        # cache=False: sharing the cached bundle would move gp's weights
        # to CPU/fp32 under its feet
        cp = StableDiffusionPipeline(
            load_model("tiny", device="cpu", dtype=torch.float32,
                       cache=False),
            device="cpu", dtype=torch.float32,
        )
        img = torch.randint(0, 255, (2, 64, 64, 3), dtype=torch.uint8)
        lg = gp.encode_image(img, seeds=[1, 2]).float().cpu()
        lc = cp.encode_image(img, seeds=[1, 2]).float()
        assert lg.shape == lc.shape == (2, 4, 32, 32)
        rel = (lg - lc).abs().mean() / lc.abs().mean().clamp_min(1e-6)
        assert rel < 0.15, f"latent grids diverge: rel={rel}"


class TestRefinerGPU:
    def test_same_model_refiner_identity_on_gpu(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        base = dict(prompt="r", steps=3, width=64, height=64, seeds=[7])
        a = pipe.generate(PipelineRequest(**base)).images
        b = pipe.generate(
            PipelineRequest(**base, refiner_model="tiny",
                            refiner_switch_at=0.5)
        ).images
        assert torch.equal(a, b)


class TestVPredictionGPU:
    def test_v_model_generates_on_gpu(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny-v", device=dev)
        res = pipe.generate(
            PipelineRequest(prompt="v", steps=3, width=64, height=64,
                            seeds=[3])
        )
        assert torch.isfinite(res.images.float()).all()
        assert res.images.float().std() > 1.0


class TestPromptFeaturesGPU:
    def test_editing_and_composition_on_gpu(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        base = dict(steps=3, width=64, height=64, seeds=[5])
        edited = pipe.generate(
            PipelineRequest(prompt="a [cat:dog:0.5] x", **base)
        ).images
        comp = pipe.generate(
            PipelineRequest(prompt="a cat AND a dog:0.5", **base)
        ).images
        plain = pipe.generate(PipelineRequest(prompt="a cat", **base)).images
        for out in (edited, comp):
            assert torch.isfinite(out.float()).all()
            assert not torch.equal(out, plain)


class TestInpaintModelGPU:
    def test_9ch_model_generates(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny-inpaint", device=dev)
        res = pipe.generate(
            PipelineRequest(prompt="i", steps=2, width=64, height=64,
                            seeds=[1])
        )
        assert torch.isfinite(res.images.float()).all()


class TestLongPromptGPU:
    def test_cross_attention_154_keys(self, dev):
        """Two-chunk prompts give Sk=154 cross-attention (2*64 + 26 tail);
        numerics vs fp32 reference at the exact production layout."""
        from sdwd_amd import ops

        torch.manual_seed(5)
        b, sq, sk, h, d = 2, 1024, 154, 8, 40
        q = torch.randn(b, sq, h, d, device=dev, dtype=torch.bfloat16)
        k = torch.randn(b, sk, h, d, device=dev, dtype=torch.bfloat16)
        v = torch.randn(b, sk, h, d, device=dev, dtype=torch.bfloat16)
        out = ops.attention_bshd(q, k, v)
        qf = q.float().permute(0, 2, 1, 3)
        kf = k.float().permute(0, 2, 1, 3)
        vf = v.float().permute(0, 2, 1, 3)
        s = torch.matmul(qf, kf.transpose(-1, -2)) * (d ** -0.5)
        ref = torch.matmul(s.softmax(-1), vf).permute(0, 2, 1, 3)
        err = (out.float() - ref).abs().max().item()
        assert err < 0.06, err

    def test_long_prompt_pipeline_gpu(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline("tiny", device=dev)
        prompt = " ".join(f"w{i}" for i in range(100))
        res = pipe.generate(
            PipelineRequest(prompt=prompt, steps=2, width=64, height=64,
                            seeds=[4])
        )
        assert torch.isfinite(res.images.float()).all()
