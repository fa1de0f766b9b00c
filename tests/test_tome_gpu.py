"""GPU tests of token merging: the tome.hip kernels against the fp64 oracle
(tests/tome_oracle.py) and the CPU ops, the gathered add+LN, the block and
the pipeline.

Match bound (tome_oracle's docstring): with s the fp64 scores and
E0 = (C + 16) * 2^-23, every src row must have

    max_j s - s[node_idx] <= 2 E0      |node_max - s[node_idx]| <= E0

and rows whose fp64 top-two gap exceeds 2 E0 must return exactly the
oracle's index. Merge, unmerge and the gathered add+LN are compared bit for
bit: the CPU ops do the same fp32 adds in the same order, one division, one
rounding.
"""
from unittest import mock

import numpy as np
import pytest
import torch

import tome_oracle as T
from sdwd_amd import ops

pytestmark = pytest.mark.gpu

C = T.WIDTH
E0 = T.e0(C)
SHAPES = list(T.SHAPES)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _match_gpu(x, h, w, dev):
    xg = x.to(dev)
    assert ops.tome_match_supported(xg)
    node_max, node_idx = ops.tome_match(xg, h, w)
    assert node_max.dtype == torch.float32 and node_idx.dtype == torch.int32
    return node_max.cpu().double().numpy(), node_idx.cpu().long().numpy()


def _check_against_scores(s, node_max, node_idx, tag):
    """The two bounds and the exact-index rule; returns the excused share."""
    nd = s.shape[-1]
    assert node_idx.min() >= 0 and node_idx.max() < nd
    top, want = T.match(s)
    at = np.take_along_axis(s, node_idx[..., None], -1)[..., 0]
    d_arg = (top - at).max()
    d_max = np.abs(node_max - at).max()
    clear = T.top_two_gap(s) > 2 * E0
    wrong = int(((node_idx != want) & clear).sum())
    excused = float((~clear).mean())
    print(f"{tag}: max_j s - s[idx] {d_arg:.3e} (<= {2 * E0:.3e}), "
          f"|node_max - s[idx]| {d_max:.3e} (<= {E0:.3e}), "
          f"wrong clear rows {wrong}, excused {100 * excused:.2f}%")
    assert d_arg <= 2 * E0
    assert d_max <= E0
    assert wrong == 0
    return excused


class TestMatch:
    @pytest.mark.parametrize("hw", SHAPES)
    def test_random(self, dev, hw):
        h, w = hw
        x = T.random_input(h, w)
        s = T.scores(x, h, w)
        # the fixed seeds keep the oracle's own near-ties under 2%
        assert float((T.top_two_gap(s) <= 2 * E0).mean()) <= 0.02
        node_max, node_idx = _match_gpu(x, h, w, dev)
        excused = _check_against_scores(s, node_max, node_idx, f"random {hw}")
        assert excused <= 0.02

    @pytest.mark.parametrize("hw", SHAPES)
    def test_planted(self, dev, hw):
        h, w = hw
        x, pi = T.planted_input(h, w)
        s = T.scores(x, h, w)
        _, want = T.match(s)
        assert np.array_equal(want, pi.numpy())  # the plant holds in fp64
        assert bool((T.top_two_gap(s) > 2 * E0).all())  # no excuses
        node_max, node_idx = _match_gpu(x, h, w, dev)
        assert np.array_equal(node_idx, pi.numpy())
        _check_against_scores(s, node_max, node_idx, f"planted {hw}")

    def test_ties_lowest_index_wins(self, dev):
        """Duplicated dst rows: (low, high) pairs with the low index in
        either half-wave's accumulator rows and in either dst tile."""
        h, w = 24, 24
        # crow: rows 0-3 belong to half 0, 4-7 to half 1, 8-11 to half 0...
        pairs = [(3, 7), (5, 9), (10, 64 + 10), (20, 64 + 1), (40, 128 + 15)]
        lows = [p[0] for p in pairs]

        def target(b, i, nd):
            return lows[i % len(lows)] if i % 3 == 0 else (7 * i + 3 * b) % nd

        x, pi = T.planted_input(h, w, seed=1, target=target)
        src, dst = T.partition(h, w)
        # the duplicates go in after the plant: a src row that the default
        # rule aimed at a HIGH index keeps its old target's direction and
        # now matches nothing closely
        for lo, hi in pairs:
            x[:, dst[hi]] = x[:, dst[lo]]
        highs = [p[1] for p in pairs]
        pi_np = pi.numpy()
        s = T.scores(x, h, w)
        for lo, hi in pairs:
            assert np.array_equal(s[:, :, lo], s[:, :, hi])
        top, want = T.match(s)
        aimed = np.isin(pi_np, lows)
        assert aimed.sum() >= 2 * len(pairs)
        assert np.array_equal(want[aimed], pi_np[aimed])
        node_max, node_idx = _match_gpu(x, h, w, dev)
        assert np.array_equal(node_idx[aimed], pi_np[aimed])
        assert not np.isin(node_idx, highs).any()
        _check_against_scores(s, node_max, node_idx, "ties (24, 24)")

    def test_table_safety_ragged_edges(self, dev):
        """N = 252, Ns = 189, Nd = 63: the last dst row of a ragged tile and
        the last src row of a ragged block. The row staged behind the last
        dst row is masked, so every index stays below Nd."""
        h, w = 18, 14
        src, dst = T.partition(h, w)
        assert (h * w, len(src), len(dst)) == (252, 189, 63)

        def target(b, i, nd):
            return nd - 1 if i % 2 == 0 or i >= 186 else (5 * i + b) % nd

        x, pi = T.planted_input(h, w, seed=2, target=target)
        s = T.scores(x, h, w)
        assert np.array_equal(T.match(s)[1], pi.numpy())
        node_max, node_idx = _match_gpu(x, h, w, dev)
        assert node_idx.max() == len(dst) - 1
        assert np.array_equal(node_idx, pi.numpy())
        assert np.isfinite(node_max).all()
        # the tables themselves: int32, in range, a partition of the tokens
        st, dt = ops.tome_partition(h, w, dev)
        assert st.dtype == dt.dtype == torch.int32
        both = torch.cat([st, dt]).cpu().long().sort().values
        assert torch.equal(both, torch.arange(h * w))

    def test_composed_route_for_other_widths(self, dev):
        x = T.random_input(9, 11, c=64).to(dev)
        assert not ops.tome_match_supported(x)
        assert not ops.tome_match_supported(T.random_input(9, 11).to(dev).float())
        node_max, node_idx = ops.tome_match(x, 9, 11)
        cm, ci = ops.tome_match(x.cpu(), 9, 11)
        s = T.scores(x, 9, 11)
        at = np.take_along_axis(
            s, node_idx.cpu().long().numpy()[..., None], -1)[..., 0]
        assert (s.max(-1) - at).max() <= 2 * T.e0(64)
        assert node_idx.dtype == ci.dtype == torch.int32
        assert node_max.shape == cm.shape


def _synthetic_match(h, w, seed):
    """(node_max, node_idx) with ties in node_max, a dst with no member and
    one that the 12 strongest src tokens all point to."""
    src, dst = T.partition(h, w)
    ns, nd = len(src), len(dst)
    g = torch.Generator().manual_seed(seed)
    node_max = (torch.rand(T.BATCH, ns, generator=g) * 32).floor() / 64
    node_idx = torch.randint(2, nd, (T.BATCH, ns), generator=g)
    heavy = torch.randperm(ns, generator=g)[:12]
    node_max[:, heavy] = 0.75 + torch.arange(12) / 64.0
    node_idx[:, heavy] = 0           # dst 0: more than 8 members
    return node_max, node_idx.to(torch.int32)  # dst 1: never a target


def _rs(h, w):
    src, _ = T.partition(h, w)
    n = h * w
    return [n // 4, n // 2, len(src)]


class TestPlan:
    @pytest.mark.parametrize("hw", SHAPES)
    def test_gpu_plan_equals_cpu_plan(self, dev, hw):
        h, w = hw
        node_max, node_idx = _synthetic_match(h, w, 5)
        for r in _rs(h, w):
            cpu = ops.tome_plan(node_max, node_idx, h, w, r)
            gpu = ops.tome_plan(node_max.to(dev), node_idx.to(dev), h, w, r)
            for a, b in zip(cpu.tensors(), gpu.tensors()):
                assert b.is_cuda and b.dtype == torch.int32
                assert torch.equal(a, b.cpu())
            assert torch.equal(cpu.dst_tok, gpu.dst_tok.cpu())


class TestMergeUnmerge:
    @pytest.mark.parametrize("hw", SHAPES)
    def test_bit_equal_to_cpu_ops(self, dev, hw):
        h, w = hw
        x = T.random_input(h, w, seed=3)
        node_max, node_idx = _synthetic_match(h, w, 6)
        for r in _rs(h, w):
            cpu = ops.tome_plan(node_max, node_idx, h, w, r)
            gpu = ops.tome_plan(node_max.to(dev), node_idx.to(dev), h, w, r)
            count = (cpu.seg_start[:, 1:] - cpu.seg_start[:, :-1])
            assert int(count[:, 0].min()) > 8 and int(count[:, 1].max()) == 0
            want = ops.tome_merge(x, cpu)
            xg = x.to(dev)
            assert ops.tome_match_supported(xg)
            with mock.patch.object(
                    ops.ext(), "tome_merge", wraps=ops.ext().tome_merge
            ) as kernel:
                got = ops.tome_merge(xg, gpu)
            assert kernel.call_count == 1  # tome.hip, not the torch route
            assert got.shape == (T.BATCH, h * w - r, C)
            assert torch.equal(got.cpu(), want)
            # and the composed GPU route, the block's A/B partner
            assert torch.equal(
                ops.tome_merge(x.to(dev), gpu, native=False).cpu(), want)
            back = ops.tome_unmerge(got, gpu)
            assert back.shape == (T.BATCH, h * w, C)
            assert torch.equal(back.cpu(), ops.tome_unmerge(want, cpu))

    def test_merge_close_to_fp64(self, dev):
        h, w = 18, 14
        x = T.random_input(h, w, seed=4)
        node_max, node_idx = _synthetic_match(h, w, 7)
        r = h * w // 2
        gpu = ops.tome_plan(node_max.to(dev), node_idx.to(dev), h, w, r)
        ref = T.merge(x, h, w, T.plan(node_max.numpy(), node_idx.numpy(),
                                      h, w, r))
        got = ops.tome_merge(x.to(dev), gpu).cpu().double().numpy()
        # an fp32 sum of k + 1 <= 190 terms is within k 2^-24 sum|x_m| of
        # the exact one, so the mean within k 2^-24 max|x|; then one fp32
        # division (2^-24) and one bf16 rounding (half an ulp: 2^-8), both
        # relative
        bound = (2.0 ** -8 + 2.0 ** -23) * np.abs(ref) \
            + 190 * 2.0 ** -24 * float(x.float().abs().max())
        assert (np.abs(got - ref) <= bound).all()


class TestGatheredAddLayerNorm:
    @pytest.mark.parametrize("hw", [(16, 16), (9, 11)])
    def test_equals_ungathered_on_unmerged(self, dev, hw):
        h, w = hw
        n = h * w
        g = torch.Generator().manual_seed(8)
        x = torch.randn(T.BATCH, n, C, generator=g).to(torch.bfloat16).to(dev)
        node_max, node_idx = _synthetic_match(h, w, 9)
        r = n // 2
        plan = ops.tome_plan(node_max.to(dev), node_idx.to(dev), h, w, r)
        y = torch.randn(T.BATCH, n - r, C, generator=g).to(torch.bfloat16)
        y = y.to(dev)
        wt = torch.randn(C, generator=g).to(dev)
        bs = torch.randn(C, generator=g).to(dev)
        s0, l0 = ops.add_layer_norm(x, ops.tome_unmerge(y, plan), wt, bs, 1e-5)
        s1, l1 = ops.add_layer_norm(x, y, wt, bs, 1e-5, gather=plan.slot)
        assert torch.equal(s0, s1) and torch.equal(l0, l1)


def _block(dev):
    from sdwd_amd.models.unet import BasicTransformerBlock

    torch.manual_seed(11)
    blk = BasicTransformerBlock(C, 64, 8).to(dev, torch.bfloat16).eval()
    return blk


def _block_inputs(h, w, seed, dev):
    """Planted so that both match routes give one plan at ratio 0.375: half
    of the src tokens sit next to their dst (cos ~ 1), half far away."""
    src, _ = T.partition(h, w)
    noise = torch.where(torch.arange(len(src)) % 2 == 0, 2.0 ** -6, 0.5)
    x, _ = T.planted_input(h, w, seed=seed, noise=noise)
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn(T.BATCH, 7, 64, generator=g).to(torch.bfloat16)
    return x.to(dev), ctx.to(dev)


class TestBlock:
    def test_native_equals_composed(self, dev):
        h, w = 16, 16
        blk = _block(dev)
        blk.tome_ratio = 0.375
        assert ops.tome_merge_count(h, w, 0.375) == 96
        x, ctx = _block_inputs(h, w, 21, dev)
        assert ops.tome_match_supported(x)
        with torch.no_grad():
            blk.tome_native = True
            p1 = blk._tome_plan(x, (h, w))
            out1 = blk(x, ctx, (h, w))
            blk.tome_native = False
            p0 = blk._tome_plan(x, (h, w))
            out0 = blk(x, ctx, (h, w))
            blk.tome_ratio = 0.0
            plain = blk(x, ctx, (h, w))
        for a, b in zip(p0.tensors(), p1.tensors()):
            assert torch.equal(a, b)
        assert torch.isfinite(out1.float()).all()
        assert torch.equal(out0, out1)
        assert not torch.equal(out1, plain)

    def test_graph_replay_equals_eager(self, dev):
        h, w = 16, 16
        blk = _block(dev)
        blk.tome_ratio = 0.5
        x0, ctx = _block_inputs(h, w, 22, dev)
        x1 = T.random_input(h, w, seed=23).to(dev)
        sx = x0.clone()
        with torch.no_grad():
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):
                    blk(sx, ctx, (h, w))
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = blk(sx, ctx, (h, w))
            for x in (x1, x0):
                sx.copy_(x)
                graph.replay()
                torch.cuda.synchronize(dev)
                assert torch.equal(out, blk(x, ctx, (h, w)))


class TestPipeline:
    def test_graphs_on_equals_off_and_repeatable(self, dev, monkeypatch):
        """Tiny UNet widened to model_channels = 320 (the kernels' width) at
        128x128: N = 4096 tokens at level 0."""
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

        req = PipelineRequest(prompt="merged cow", steps=3, width=128,
                              height=128, seeds=[5, 6],
                              token_merging_ratio=0.5)
        f = VAEConfig.tiny().downsample_factor
        seen = []
        merge = ops.tome_merge

        def spy(x, plan, native=True):
            seen.append((tuple(x.shape), ops.tome_match_supported(x), native))
            return merge(x, plan, native)

        monkeypatch.setenv("SDWD_HIPGRAPH", "0")
        eager = StableDiffusionPipeline(bundle(), device=dev)
        with monkeypatch.context() as m:
            m.setattr(ops, "tome_merge", spy)
            a = eager.generate(req)
        n0 = (128 // f) ** 2
        assert seen and all(
            s[0][1:] == (n0, 320) and s[1] and s[2] for s in seen)
        assert "Token merging ratio: 0.5" in a.infotexts[0]
        assert torch.equal(a.images, eager.generate(req).images)
        off = eager.generate(replace(req, token_merging_ratio=0.0))
        assert not torch.equal(a.images, off.images)
        assert "Token merging" not in off.infotexts[0]

        monkeypatch.setenv("SDWD_HIPGRAPH", "1")
        graphed = StableDiffusionPipeline(bundle(), device=dev)
        b = graphed.generate(req)
        caches = list(graphed._wholestep_cache.values())
        assert caches and all(g.cache and not g.failed for g in caches)
        assert torch.equal(a.images, b.images)
        assert torch.equal(b.images, graphed.generate(req).images)
