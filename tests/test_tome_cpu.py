"""Token merging on the CPU: the ops' torch paths against the fp64 oracle
(tests/tome_oracle.py), the plan's invariants, the block, the tiny pipeline,
the engine, the API, the infotext and the X/Y/Z axis.
"""
import base64
import json
from dataclasses import replace

import numpy as np
import pytest
import torch

import tome_oracle as T
from sdwd_amd import ops
from sdwd_amd.models import load_model
from sdwd_amd.models.unet import BasicTransformerBlock
from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline
from sdwd_amd.pipeline.pipeline import token_merging_ratio_for
from sdwd_amd.utils.infotext import parse_infotext

SHAPES = list(T.SHAPES)
COUNTS = {(16, 16): (64, 192), (18, 14): (63, 189), (24, 24): (144, 432),
          (9, 11): (20, 79)}


def _synthetic_match(h, w, seed):
    """(node_max with many ties, node_idx) for plan tests."""
    src, dst = T.partition(h, w)
    g = torch.Generator().manual_seed(seed)
    node_max = (torch.rand(T.BATCH, len(src), generator=g) * 16).floor() / 16
    node_idx = torch.randint(0, len(dst), (T.BATCH, len(src)), generator=g)
    return node_max, node_idx.to(torch.int32)


class TestPartition:
    @pytest.mark.parametrize("hw", SHAPES)
    def test_counts_and_membership(self, hw):
        h, w = hw
        src, dst = ops.tome_partition(h, w, "cpu")
        assert src.dtype == dst.dtype == torch.int32
        assert (dst.numel(), src.numel()) == COUNTS[hw]
        assert dst.numel() == (h // 2) * (w // 2)
        osrc, odst = T.partition(h, w)
        assert np.array_equal(src.numpy(), osrc)
        assert np.array_equal(dst.numpy(), odst)
        for t in dst.tolist():
            y, x = divmod(t, w)
            assert y % 2 == 0 and x % 2 == 0
            assert y < 2 * (h // 2) and x < 2 * (w // 2)
        both = torch.cat([src, dst]).long().sort().values
        assert torch.equal(both, torch.arange(h * w))

    def test_odd_tail_is_src(self):
        h, w = 9, 11
        src, _ = ops.tome_partition(h, w, "cpu")
        s = set(src.tolist())
        assert all((h - 1) * w + x in s for x in range(w))
        assert all(y * w + (w - 1) in s for y in range(h))

    def test_cached(self):
        a = ops.tome_partition(16, 16, "cpu")
        b = ops.tome_partition(16, 16, "cpu")
        assert a[0] is b[0] and a[1] is b[1]

    @pytest.mark.parametrize("hw", SHAPES)
    def test_merge_count(self, hw):
        h, w = hw
        n, ns = h * w, COUNTS[hw][1]
        assert ops.tome_merge_count(h, w, 0.0) == 0
        assert ops.tome_merge_count(h, w, 0.5) == int(n * 0.5) == n // 2
        assert ops.tome_merge_count(h, w, 0.3) == int(n * 0.3)
        assert ops.tome_merge_count(h, w, 0.9) == ns  # the clamp at Ns
        assert int(n * 0.9) > ns
        assert ops.tome_merge_count(h, w, 0.9) == T.merge_count(h, w, 0.9)

    def test_no_dst_no_merging(self):
        assert ops.tome_merge_count(1, 8, 0.5) == 0
        assert ops.tome_merge_count(8, 1, 0.9) == 0
        with pytest.raises(ValueError):
            ops.tome_partition(1, 8, "cpu")


class TestMatch:
    @pytest.mark.parametrize("hw", SHAPES)
    def test_against_oracle(self, hw):
        h, w = hw
        x = T.random_input(h, w)
        s = T.scores(x, h, w)
        node_max, node_idx = ops.tome_match(x, h, w)
        assert node_max.dtype == torch.float32
        assert node_idx.dtype == torch.int32
        e0 = T.e0(T.WIDTH)
        idx = node_idx.long().numpy()
        at = np.take_along_axis(s, idx[..., None], -1)[..., 0]
        assert (s.max(-1) - at).max() <= 2 * e0
        assert np.abs(node_max.double().numpy() - at).max() <= e0
        clear = T.top_two_gap(s) > 2 * e0
        assert np.array_equal(idx[clear], T.match(s)[1][clear])

    def test_lowest_index_on_ties_and_zero_rows(self):
        h, w = 9, 11
        x = T.random_input(h, w, c=32)
        src, dst = T.partition(h, w)
        x[:, dst[7]] = x[:, dst[2]]
        x[:, src[5]] = x[:, dst[2]] * 2
        x[:, src[6]] = 0  # a zero row scores 0 against everything
        node_max, node_idx = ops.tome_match(x, h, w)
        assert node_idx[:, 5].tolist() == [2, 2]
        assert node_max[:, 6].tolist() == [0.0, 0.0]
        assert node_idx[:, 6].tolist() == [0, 0]
        assert torch.isfinite(node_max).all()


class TestPlan:
    @pytest.mark.parametrize("hw", SHAPES)
    def test_invariants_and_oracle(self, hw):
        h, w = hw
        n = h * w
        src, dst = T.partition(h, w)
        ns, nd = len(src), len(dst)
        node_max, node_idx = _synthetic_match(h, w, 3)
        for r in (1, n // 4, n // 2, ns):
            p = ops.tome_plan(node_max, node_idx, h, w, r)
            for t in p.tensors():
                assert t.dtype == torch.int32
            assert p.slot.shape == (T.BATCH, n)
            assert p.unm_tok.shape == (T.BATCH, ns - r)
            assert p.seg_start.shape == (T.BATCH, nd + 1)
            assert p.members.shape == (T.BATCH, r)
            assert int(p.slot.min()) >= 0 and int(p.slot.max()) < n - r
            for b in range(T.BATCH):
                # exactly r merged: the r largest, ties to the lower position
                order = sorted(range(ns),
                               key=lambda i: (-float(node_max[b, i]), i))
                merged = sorted(src[i] for i in order[:r])
                assert sorted(p.members[b].tolist()) == merged
                assert len(set(merged)) == r
                assert p.unm_tok[b].tolist() == sorted(
                    set(src.tolist()) - set(merged))
                seg = p.seg_start[b].tolist()
                assert seg[0] == 0 and seg[-1] == r
                assert all(a <= c for a, c in zip(seg, seg[1:]))
                tok2i = {int(t): i for i, t in enumerate(src)}
                for j in range(nd):
                    part = p.members[b, seg[j]:seg[j + 1]].tolist()
                    assert part == sorted(part)
                    assert all(int(node_idx[b, tok2i[t]]) == j for t in part)
                    assert all(int(p.slot[b, t]) == ns - r + j for t in part)
                    assert int(p.slot[b, dst[j]]) == ns - r + j
                for u, t in enumerate(p.unm_tok[b].tolist()):
                    assert int(p.slot[b, t]) == u
            o = T.plan(node_max.numpy(), node_idx.numpy(), h, w, r)
            for k in ("slot", "unm_tok", "seg_start", "members"):
                assert np.array_equal(getattr(p, k).numpy(), o[k]), k

    def test_bad_r(self):
        node_max, node_idx = _synthetic_match(9, 11, 4)
        with pytest.raises(ValueError):
            ops.tome_plan(node_max, node_idx, 9, 11, 80)
        with pytest.raises(ValueError):
            ops.tome_plan(node_max[:, :5], node_idx[:, :5], 9, 11, 3)


class TestMergeUnmerge:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("hw", SHAPES)
    def test_constant_stays_constant(self, hw, dtype):
        h, w = hw
        node_max, node_idx = _synthetic_match(h, w, 5)
        r = h * w // 2
        p = ops.tome_plan(node_max, node_idx, h, w, r)
        # bf16: the fp32 mean of k copies of c is c (1 + e), |e| <= k 2^-24,
        # far inside half a bf16 ulp of c, so the one rounding returns c.
        # fp32 has no such slack: a dyadic constant keeps the sums exact.
        const = 0.3 if dtype == torch.bfloat16 else 0.375
        x = torch.full((T.BATCH, h * w, 16), const, dtype=dtype)
        m = ops.tome_merge(x, p)
        assert m.shape == (T.BATCH, h * w - r, 16) and m.dtype == dtype
        assert torch.equal(m, torch.full_like(m, const))

    @pytest.mark.parametrize("hw", [(16, 16), (24, 24)])
    def test_round_trip_on_constant_cells(self, hw):
        """Every 2x2 cell constant, the cells different: each src token's
        best match is its own cell's dst at cosine 1, merging averages equal
        rows, and unmerge(merge(x)) is x bit for bit."""
        h, w = hw
        g = torch.Generator().manual_seed(6)
        cells = torch.randn(T.BATCH, h // 2, w // 2, 48, generator=g)
        cells = cells.to(torch.bfloat16)
        x = cells.repeat_interleave(2, 1).repeat_interleave(2, 2)
        x = x.reshape(T.BATCH, h * w, 48)
        node_max, node_idx = ops.tome_match(x, h, w)
        src, dst = T.partition(h, w)
        own = [(t // w // 2) * (w // 2) + (t % w) // 2 for t in src]
        assert node_idx.tolist() == [own, own]
        for ratio in (0.25, 0.5, 0.9):
            r = ops.tome_merge_count(h, w, ratio)
            p = ops.tome_plan(node_max, node_idx, h, w, r)
            assert torch.equal(ops.tome_unmerge(ops.tome_merge(x, p), p), x)

    @pytest.mark.parametrize("hw", SHAPES)
    def test_merge_against_oracle(self, hw):
        h, w = hw
        x = T.random_input(h, w, seed=7, c=24)
        node_max, node_idx = _synthetic_match(h, w, 8)
        r = h * w // 2
        p = ops.tome_plan(node_max, node_idx, h, w, r)
        ref = T.merge(x, h, w, T.plan(node_max.numpy(), node_idx.numpy(),
                                      h, w, r))
        got = ops.tome_merge(x, p).double().numpy()
        bound = (2.0 ** -8 + 2.0 ** -23) * np.abs(ref) \
            + h * w * 2.0 ** -24 * float(x.float().abs().max())
        assert (np.abs(got - ref) <= bound).all()

    def test_gathered_add_layer_norm(self):
        h, w = 9, 11
        n, c = h * w, 40
        g = torch.Generator().manual_seed(9)
        node_max, node_idx = _synthetic_match(h, w, 10)
        r = n // 2
        p = ops.tome_plan(node_max, node_idx, h, w, r)
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn(T.BATCH, n, c, generator=g).to(dtype)
            y = torch.randn(T.BATCH, n - r, c, generator=g).to(dtype)
            wt, bs = torch.randn(c, generator=g), torch.randn(c, generator=g)
            s0, l0 = ops.add_layer_norm(x, ops.tome_unmerge(y, p), wt, bs)
            s1, l1 = ops.add_layer_norm(x, y, wt, bs, gather=p.slot)
            assert torch.equal(s0, s1) and torch.equal(l0, l1)

    def test_rows_independent_of_batch_neighbours(self):
        """What shard parity rests on: a batch row's match, plan and merge
        do not depend on the other rows."""
        h, w = 18, 14
        x = T.random_input(h, w, seed=11, c=64)
        r = h * w // 2

        def run(t):
            node_max, node_idx = ops.tome_match(t, h, w)
            p = ops.tome_plan(node_max, node_idx, h, w, r)
            return (node_max, node_idx, *p.tensors(), ops.tome_merge(t, p))

        whole = run(x)
        for b in range(T.BATCH):
            for a, c in zip(whole, run(x[b:b + 1])):
                assert torch.equal(a[b:b + 1], c)
        swapped = run(x.flip(0))
        for a, c in zip(whole, swapped):
            assert torch.equal(a, c.flip(0))


class TestBlock:
    def test_ratio_zero_is_todays_block(self):
        torch.manual_seed(12)
        blk = BasicTransformerBlock(32, 16, 2).eval()
        assert blk.tome_ratio == 0.0 and BasicTransformerBlock.tome_native
        x = torch.randn(2, 64, 32)
        ctx = torch.randn(2, 5, 16)
        with torch.no_grad():
            base = blk(x, ctx)
            assert torch.equal(blk(x, ctx, (8, 8)), base)
            blk.tome_ratio = 0.01  # r = int(64 * 0.01) = 0
            assert torch.equal(blk(x, ctx, (8, 8)), base)
            blk.tome_ratio = 0.5
            merged = blk(x, ctx, (8, 8))
        assert merged.shape == base.shape
        assert torch.isfinite(merged).all()
        assert not torch.equal(merged, base)

    def test_attention_sees_the_merged_length(self):
        torch.manual_seed(13)
        blk = BasicTransformerBlock(32, 16, 2).eval()
        blk.tome_ratio = 0.5
        seen = []
        attn1, attn2 = blk.attn1.forward, blk.attn2.forward
        blk.attn1.forward = lambda x, c=None: (seen.append(x.shape[1]),
                                               attn1(x, c))[1]
        blk.attn2.forward = lambda x, c=None: (seen.append(x.shape[1]),
                                               attn2(x, c))[1]
        with torch.no_grad():
            blk(torch.randn(1, 80, 32), torch.randn(1, 5, 16), (8, 10))
        assert seen == [40, 80]  # cross-attention and the MLP see all tokens


# ---------------------------------------------------------------------------
# pipeline, engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe():
    return StableDiffusionPipeline(
        load_model("tiny", device="cpu", dtype=torch.float32, cache=False),
        device="cpu", dtype=torch.float32,
    )


REQ = dict(prompt="cows", steps=2, width=64, height=64, seeds=[5, 6])


class TestPipeline:
    def test_ratio_semantics(self, pipe):
        plain = pipe.generate(PipelineRequest(**REQ))
        zero = pipe.generate(PipelineRequest(**REQ, token_merging_ratio=0.0))
        assert torch.equal(plain.images, zero.images)
        assert plain.infotexts == zero.infotexts
        assert "Token merging" not in plain.infotexts[0]
        half = pipe.generate(PipelineRequest(**REQ, token_merging_ratio=0.5))
        assert not torch.equal(half.images, plain.images)
        assert "Token merging ratio: 0.5" in half.infotexts[0]
        again = pipe.generate(PipelineRequest(**REQ, token_merging_ratio=0.5))
        assert torch.equal(half.images, again.images)
        # and back: the switch leaves nothing behind
        assert torch.equal(pipe.generate(PipelineRequest(**REQ)).images,
                           plain.images)

    @pytest.mark.parametrize("ratio", [0.0, 0.5])
    def test_generate_runs_without_autograd(self, pipe, monkeypatch, ratio):
        """generate() is a no_grad region: inside the UNet grad is off and
        neither its input nor its output carries a graph, at any ratio."""
        unet = pipe.model.unet
        assert any(p.requires_grad for p in unet.parameters())
        forward = unet.forward
        seen = []

        def spy(x, *args, **kw):
            out = forward(x, *args, **kw)
            seen.append((torch.is_grad_enabled(), x.requires_grad,
                         out.requires_grad))
            return out

        monkeypatch.setattr(unet, "forward", spy)
        assert torch.is_grad_enabled()
        pipe.generate(PipelineRequest(**REQ, token_merging_ratio=ratio))
        assert len(seen) >= 2
        assert all(s == (False, False, False) for s in seen)
        assert torch.is_grad_enabled()

    def test_only_level0_blocks_of_the_unet(self, pipe):
        pipe.generate(PipelineRequest(**REQ, token_merging_ratio=0.5))
        unet = pipe.model.unet
        level0 = unet.level0_blocks()
        assert level0
        for m in unet.modules():
            if isinstance(m, BasicTransformerBlock):
                want = 0.5 if any(m is b for b in level0) else 0.0
                assert m.tome_ratio == want
        assert len(level0) < sum(
            isinstance(m, BasicTransformerBlock) for m in unet.modules())
        pipe.generate(PipelineRequest(**REQ))
        assert all(b.tome_ratio == 0.0 for b in level0)

    def test_sdxl_has_no_level0_transformer(self):
        from sdwd_amd.models.unet import UNetConfig, UNetModel

        cfg = UNetConfig.tiny()
        cfg.transformer_depth = [0, 1]  # the SDXL layout at tiny scale
        assert UNetModel(cfg).level0_blocks() == []

    def test_change_drops_captured_graphs(self, pipe):
        pipe.generate(PipelineRequest(**REQ))
        from types import SimpleNamespace

        wrapper = SimpleNamespace(cache={"shape": object()})
        pipe._wholestep_cache["sentinel"] = wrapper
        pipe._denoiser.cache["sentinel"] = object()
        pipe.generate(PipelineRequest(**REQ))  # same ratio: caches stay
        assert "sentinel" in pipe._wholestep_cache and wrapper.cache
        pipe.generate(PipelineRequest(**REQ, token_merging_ratio=0.5))
        assert "sentinel" not in pipe._wholestep_cache
        assert "sentinel" not in pipe._denoiser.cache
        assert not wrapper.cache  # a wrapper still held by a pass is emptied

    def test_ratio_per_pass(self):
        r = PipelineRequest(token_merging_ratio=0.5)
        assert token_merging_ratio_for(r) == 0.5
        assert token_merging_ratio_for(r, hr=True) == 0.5  # fallback
        r = replace(r, token_merging_ratio_hr=0.3)
        assert token_merging_ratio_for(r, hr=True) == 0.3
        assert token_merging_ratio_for(r) == 0.5
        lat = torch.zeros(1, 4, 8, 8)
        r = replace(r, init_latents=lat)
        assert token_merging_ratio_for(r) == 0.5  # fallback
        r = replace(r, token_merging_ratio_img2img=0.2)
        assert token_merging_ratio_for(r) == 0.2
        assert token_merging_ratio_for(
            PipelineRequest(token_merging_ratio=3.0)) == 0.9
        assert token_merging_ratio_for(
            PipelineRequest(token_merging_ratio=-1.0)) == 0.0
        assert token_merging_ratio_for(
            PipelineRequest(token_merging_ratio_hr=0.4)) == 0.0

    def test_hires_pass_infotext(self, pipe):
        res = pipe.generate(PipelineRequest(
            **{**REQ, "seeds": [5]}, enable_hr=True, hr_scale=2.0,
            hr_steps=1, token_merging_ratio=0.5,
            token_merging_ratio_hr=0.25))
        info = parse_infotext(res.infotexts[0])
        assert info["Token merging ratio"] == "0.5"
        assert info["Token merging ratio hr"] == "0.25"
        assert info["token_merging_ratio"] == "0.5"
        assert info["token_merging_ratio_hr"] == "0.25"
        assert res.images.shape == (1, 128, 128, 3)
        # only the hires pass merges
        res = pipe.generate(PipelineRequest(
            **{**REQ, "seeds": [5]}, enable_hr=True, hr_scale=2.0,
            hr_steps=1, token_merging_ratio_hr=0.25))
        info = parse_infotext(res.infotexts[0])
        assert "Token merging ratio" not in info
        assert info["Token merging ratio hr"] == "0.25"


class TestEngine:
    def test_two_rank_gallery_equals_one_rank(self, monkeypatch):
        """Exact. The tiny UNet's convolutions and GEMMs round differently at
        different batch sizes (tests/test_pipeline.py::TestTxt2Img::
        test_shard_equals_whole_batch allows 1 LSB for it; here the same
        handful of pixels moves at ratio 0 as at 0.5), which says nothing
        about token merging. So, as in tests/test_noise_source.py, the UNet
        forward is a stand-in whose only library math is the model's own
        level-0 SpatialTransformer (real weights, the real match / plan /
        merge / gathered add+LN); the ratio 0 run shows that the stand-in
        itself shards exactly."""
        from sdwd_amd.parallel import GenerationRequest, LocalEngine

        merges = []
        merge = ops.tome_merge

        def spy(x, plan, native=True):
            merges.append(x.shape[0])
            return merge(x, plan, native)

        monkeypatch.setattr(ops, "tome_merge", spy)

        def stand_in(unet):
            st = unet._level0[0]

            def forward(x, ts, ctx, y=None, control=None):
                h = st(x.repeat(1, 8, 1, 1), ctx)  # 4 -> 32 channels
                return torch.tanh(h.unflatten(1, (8, 4)).mean(1)) * 0.5 \
                    + 0.01 * ts.view(-1, 1, 1, 1) / 1000.0

            monkeypatch.setattr(unet, "forward", forward)

        engines = []
        for devices in (["cpu"], ["cpu", "cpu"]):
            eng = LocalEngine(model="tiny", devices=devices)
            for wk in eng.world.workers:
                wk.eta.avg_ipm = 60.0
            for p in eng.pipes.values():
                stand_in(p.model.unet)
            engines.append(eng)
        gen = GenerationRequest(prompt="a cow", batch_size=4, width=64,
                                height=64, steps=3, seed=21)
        galleries = {}
        for ratio in (0.0, 0.5):
            merges.clear()
            one, two = (e.generate(replace(gen, token_merging_ratio=ratio))
                        for e in engines)
            assert one.images.shape == (4, 64, 64, 3)
            assert torch.equal(one.images, two.images), ratio
            assert one.infotexts == [
                t.replace("gpu1", "gpu0") for t in two.infotexts]
            assert bool(merges) == (ratio > 0)
            galleries[ratio] = one
        # the 2-rank run merged in shards of 2 images (4 rows with CFG)
        assert max(merges) == 8 and min(merges) == 4
        assert not torch.equal(galleries[0.0].images, galleries[0.5].images)
        assert all("Token merging ratio: 0.5" in t
                   for t in galleries[0.5].infotexts)


# ---------------------------------------------------------------------------
# API, infotext, X/Y/Z
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def client(tmp_path_factory):
    from fastapi.testclient import TestClient

    from sdwd_amd.api import create_app
    from sdwd_amd.parallel import LocalEngine

    mp = pytest.MonkeyPatch()
    mp.setenv("SDWD_CONFIG", str(tmp_path_factory.mktemp("cfg") / "c.json"))
    engine = LocalEngine(model="tiny", devices=["cpu", "cpu"])
    for w in engine.world.workers:
        w.eta.avg_ipm = 60.0
    yield TestClient(create_app(engine=engine))
    mp.undo()


BODY = {"prompt": "a cow", "steps": 2, "width": 64, "height": 64,
        "batch_size": 1, "seed": 77}
KEYS = ("token_merging_ratio", "token_merging_ratio_img2img",
        "token_merging_ratio_hr")


def _post(client, route="txt2img", **extra):
    r = client.post(f"/sdapi/v1/{route}", json={**BODY, **extra})
    assert r.status_code == 200, r.text
    body = r.json()
    return body["images"][-1], json.loads(body["info"])["infotexts"][0]


def _set(client, **opts):
    assert client.post("/sdapi/v1/options", json=opts).status_code == 200


class TestApi:
    def test_options_get_and_post(self, client):
        opts = client.get("/sdapi/v1/options").json()
        assert all(opts[k] == 0.0 for k in KEYS)
        try:
            _set(client, token_merging_ratio=0.5, token_merging_ratio_hr=2)
            opts = client.get("/sdapi/v1/options").json()
            assert opts["token_merging_ratio"] == 0.5
            assert opts["token_merging_ratio_hr"] == 0.9  # clamped
            assert opts["token_merging_ratio_img2img"] == 0.0
            img, info = _post(client)
            assert "Token merging ratio: 0.5" in info
        finally:
            _set(client, **{k: 0 for k in KEYS})
        assert "Token merging" not in _post(client)[1]
        r = client.post("/sdapi/v1/options",
                        json={"token_merging_ratio": "much"})
        assert r.status_code == 422

    def test_override_beats_option_and_does_not_stick(self, client):
        plain, info0 = _post(client)
        assert "Token merging" not in info0
        img, info = _post(client,
                          override_settings={"token_merging_ratio": 0.5})
        assert "Token merging ratio: 0.5" in info
        assert base64.b64decode(img) != base64.b64decode(plain)
        assert _post(client)[0] == plain
        try:
            _set(client, token_merging_ratio=0.5)
            assert _post(client)[0] == img
            # an explicit 0 in the request beats the option
            got, info = _post(client,
                              override_settings={"token_merging_ratio": 0})
            assert got == plain and "Token merging" not in info
            assert "Token merging ratio: 0.3" in _post(
                client, override_settings={"token_merging_ratio": 0.3})[1]
        finally:
            _set(client, token_merging_ratio=0)

    def test_infotext_round_trip(self, client):
        img, info = _post(client,
                          override_settings={"token_merging_ratio": 0.5})
        parsed = parse_infotext(info)
        assert parsed["Token merging ratio"] == "0.5"
        again, info2 = _post(client, seed=int(parsed["Seed"]),
                             override_settings={
            "token_merging_ratio": float(parsed["token_merging_ratio"]),
        })
        assert again == img and info2 == info

    def test_hr_and_img2img_fallbacks(self, client):
        hr = dict(enable_hr=True, hr_scale=2.0, hr_second_pass_steps=1,
                  denoising_strength=0.5)
        _, info = _post(client, **hr,
                        override_settings={"token_merging_ratio": 0.5})
        parsed = parse_infotext(info)
        assert parsed["Token merging ratio"] == "0.5"
        assert parsed["Token merging ratio hr"] == "0.5"
        _, info = _post(client, **hr, override_settings={
            "token_merging_ratio": 0.5, "token_merging_ratio_hr": 0.25})
        parsed = parse_infotext(info)
        assert parsed["Token merging ratio"] == "0.5"
        assert parsed["Token merging ratio hr"] == "0.25"
        # img2img: its own ratio, else the general one
        from sdwd_amd.utils.images import encode_png

        png = base64.b64encode(encode_png(
            torch.full((64, 64, 3), 128, dtype=torch.uint8))).decode()
        i2i = dict(init_images=[png], denoising_strength=0.5)
        _, info = _post(client, "img2img", **i2i,
                        override_settings={"token_merging_ratio": 0.5})
        assert parse_infotext(info)["Token merging ratio"] == "0.5"
        _, info = _post(client, "img2img", **i2i, override_settings={
            "token_merging_ratio": 0.5, "token_merging_ratio_img2img": 0.2})
        assert parse_infotext(info)["Token merging ratio"] == "0.2"
        # and txt2img ignores the img2img ratio
        _, info = _post(client, override_settings={
            "token_merging_ratio_img2img": 0.2})
        assert "Token merging" not in info

    def test_ui_has_the_slider(self, client):
        page = client.get("/").text
        assert 'id="tome"' in page and "token_merging_ratio" in page


class TestXYZ:
    def test_token_merging_axis(self):
        from sdwd_amd.parallel import GenerationRequest, LocalEngine
        from sdwd_amd.parallel.xyz import resolve_axis, run_xyz

        assert resolve_axis("Token merging ratio").name \
            == "Token merging ratio"
        assert resolve_axis("token_merging_ratio").name \
            == "Token merging ratio"
        eng = LocalEngine(model="tiny", devices=["cpu"])
        for w in eng.world.workers:
            w.eta.avg_ipm = 60.0
        gen = GenerationRequest(prompt="a cow", batch_size=1, width=64,
                                height=64, steps=2, seed=11)
        out = run_xyz(eng, gen, "Token merging ratio", "0, 0.5", 0, "")
        assert out["labels"]["x_values"] == ["0.0", "0.5"]
        assert not torch.equal(out["grid"][:, :64], out["grid"][:, 64:])
        # the parameter line (the script appends its own "XYZ: ..." line)
        params = [t.split("\n")[2] for t in out["infotexts"]]
        assert ", Token merging ratio: 0.5," in params[1]
        assert "Token merging" not in params[0]
