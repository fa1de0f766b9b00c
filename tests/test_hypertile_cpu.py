"""CPU tests of Hypertile: the window rule, the windowed attention op, the
UNet and pipeline wiring, and the public surface (API options, infotext,
X/Y/Z axes). The GPU kernel is tested in tests/test_hypertile_gpu.py.

The tiny model's VAE halves once, so a 64x64 pixel request has a 32x32
latent grid: with P = 64 the rule gives L = 16 and level 0 (depth 0) is cut
into 2x2 windows of 16x16, level 1 (16x16, depth 1) stays whole.
"""
import base64
import json
import math
from dataclasses import replace

import pytest
import torch

from sdwd_amd import ops
from sdwd_amd.models import load_model
from sdwd_amd.models.unet import (
    BasicTransformerBlock,
    CrossAttention,
    UNetConfig,
    UNetModel,
)
from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline
from sdwd_amd.utils.infotext import parse_infotext


# ---------------------------------------------------------------------------
# the window rule
# ---------------------------------------------------------------------------
class TestRule:
    @pytest.mark.parametrize("width,height,h,w,depth,max_tile,want", [
        (512, 512, 64, 64, 0, 256, (2, 2)),
        (512, 512, 32, 32, 1, 256, (1, 1)),
        (768, 512, 64, 96, 0, 256, (2, 3)),
        (1024, 1024, 128, 128, 0, 256, (4, 4)),
        (1024, 1024, 64, 64, 1, 256, (1, 1)),
        (512, 512, 64, 64, 0, 128, (4, 4)),
        (1024, 1024, 64, 64, 1, 128, (2, 2)),
        (600, 600, 75, 75, 0, 256, (3, 3)),
        (520, 520, 65, 65, 0, 256, (1, 1)),
    ])
    def test_worked_values(self, width, height, h, w, depth, max_tile, want):
        assert ops.hypertile_windows(width, height, h, w, depth,
                                     max_tile) == want

    def test_window_sizes_of_the_worked_values(self):
        assert 64 // 2 == 32 and 96 // 3 == 32 and 75 // 3 == 25  # 32x32, 25x25
        assert ops.hypertile_windows(512, 512, 64, 64, 0) == (2, 2)
        assert ops.hypertile_windows(512, 512, 64, 64, 0, 128) == (4, 4)

    def test_properties(self):
        """th | h, th >= min(L * 2^d, h), no smaller divisor qualifies; the
        same along w. Sizes: multiples of 8 up to 2048 (a stride-5 sample of
        the pairs plus every square), depths 0..3, three tile sizes."""
        sizes = list(range(8, 2049, 8))
        pairs = [(s, s) for s in sizes]
        pairs += [(sizes[i], sizes[(7 * i + 3) % len(sizes)])
                  for i in range(0, len(sizes), 5)]
        for width, height in pairs:
            g = math.gcd(width, height)
            p = g & -g
            h, w = height // 8, width // 8
            for max_tile in (0, 128, 256, 512):
                least = max(128, min(max_tile, p)) // 8
                for d in range(4):
                    nh, nw = ops.hypertile_windows(width, height, h >> d or 1,
                                                   w >> d or 1, d, max_tile)
                    for n, ext in ((nh, h >> d or 1), (nw, w >> d or 1)):
                        assert ext % n == 0
                        t = ext // n
                        m = min(least * 2 ** d, ext)
                        assert t >= m
                        assert not any(ext % c == 0 for c in range(m, t))

    def test_max_depth_cuts_off(self):
        unet = UNetModel(UNetConfig.tiny())
        for max_depth in range(4):
            unet.set_hypertile(True, 64, 64, max_depth=max_depth, max_tile=0)
            for st in unet.spatial_transformers():
                # L * 2^d is at most 64 here: a 256x256 grid is always cut
                if st.hypertile_depth > max_depth:
                    assert st._window(256, 256) is None  # nh * nw == 1
                else:
                    assert st._window(256, 256) is not None

    def test_bad_arguments(self):
        for bad in (dict(width=0), dict(h=-1), dict(depth=-1),
                    dict(max_tile=-8), dict(w=2.5), dict(height=True)):
            kw = dict(width=512, height=512, h=64, w=64, depth=0)
            kw.update(bad)
            with pytest.raises(ValueError, match=next(iter(bad))):
                ops.hypertile_windows(**kw)

    def test_depths(self):
        cfg = UNetConfig.tiny()
        cfg.transformer_depth = [1, 1]
        unet = UNetModel(cfg)
        depths = [st.hypertile_depth for st in unet.spatial_transformers()]
        # down 0, down 1, up 1 (x2), up 0 (x2), middle block
        assert depths == [0, 1, 1, 1, 0, 0, 2]
        cfg = UNetConfig.tiny()
        cfg.transformer_depth = [0, 1]  # the SDXL layout at tiny scale
        unet = UNetModel(cfg)
        depths = [st.hypertile_depth for st in unet.spatial_transformers()]
        assert depths == [0, 0, 0, 1]  # level 1 is depth 0, the middle 1


# ---------------------------------------------------------------------------
# the op
# ---------------------------------------------------------------------------
def _qkv(b, s, h, d, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b, s, 3 * h * d, generator=g)
    c = h * d
    return tuple(qkv[..., i * c:(i + 1) * c].unflatten(-1, (h, d))
                 for i in range(3))


class TestOp:
    @pytest.mark.parametrize("grid,window", [
        ((8, 12), (4, 3)), ((6, 10), (6, 5)), ((9, 4), (3, 4)),
        ((10, 5), (5, 5)),
    ])
    def test_equals_attention_on_hand_sliced_windows(self, grid, window):
        (gh, gw), (th, tw) = grid, window
        b, h, d = 2, 2, 8
        q, k, v = _qkv(b, gh * gw, h, d, seed=gh * gw)
        out = ops.attention_window_bshd(q, k, v, grid=grid, window=window)
        assert out.shape == q.shape
        want = torch.full_like(out, float("nan"))
        grids = [t.reshape(b, gh, gw, h, d) for t in (q, k, v, want)]
        for i in range(gh // th):
            for j in range(gw // tw):
                sl = (slice(None), slice(i * th, (i + 1) * th),
                      slice(j * tw, (j + 1) * tw))
                qs, ks, vs = (t[sl].reshape(b, th * tw, h, d)
                              .permute(0, 2, 1, 3) for t in grids[:3])
                o = ops.attention(qs, ks, vs).permute(0, 2, 1, 3)
                grids[3][sl] = o.reshape(b, th, tw, h, d)
        assert torch.equal(out, want)

    def test_whole_grid_is_attention_bshd(self):
        q, k, v = _qkv(2, 48, 2, 8, seed=3)
        out = ops.attention_window_bshd(q, k, v, grid=(6, 8), window=(6, 8))
        assert torch.equal(out, ops.attention_bshd(q, k, v))
        out = ops.attention_window_bshd(q, k, v, grid=(6, 8), window=(6, 8),
                                        scale=0.3)
        assert torch.equal(out, ops.attention_bshd(q, k, v, scale=0.3))

    def test_split_merge_round_trip(self):
        x = torch.arange(2 * 24 * 3).reshape(2, 24, 3)
        w = ops.window_split(x, (4, 6), (2, 3))
        assert w.shape == (8, 6, 3)
        # window (0, 1) of batch 0: grid rows 0..1, columns 3..5
        assert w[1, :, 0].tolist() == [9, 12, 15, 27, 30, 33]
        assert torch.equal(ops.window_merge(w, (4, 6), (2, 3)), x)

    def test_argument_errors(self):
        q, k, v = _qkv(1, 24, 2, 8, seed=4)
        bad = [
            (dict(grid=(4, 5)), "grid"),
            (dict(window=(3, 3)), "window"),
            (dict(window=(2, 4)), "window"),
            (dict(window=(0, 3)), "window"),
            (dict(grid=(4, 6.0)), "grid"),
            (dict(grid=24), "grid"),
            (dict(window=(True, 3)), "window"),
        ]
        for kw, name in bad:
            args = dict(grid=(4, 6), window=(2, 3))
            args.update(kw)
            with pytest.raises(ValueError, match=name):
                ops.attention_window_bshd(q, k, v, **args)
        with pytest.raises(ValueError, match="one shape"):
            ops.attention_window_bshd(q, k[:, :12], v[:, :12], grid=(4, 6),
                                      window=(2, 3))
        with pytest.raises(ValueError, match=r"\[B, S, H, D\]"):
            ops.attention_window_bshd(q[0], k[0], v[0], grid=(4, 6),
                                      window=(2, 3))


# ---------------------------------------------------------------------------
# UNet
# ---------------------------------------------------------------------------
def _wrap_attn1(unet):
    """The host's way: attn1.forward wrapped by an explicit rearrange, on a
    UNet whose own Hypertile is off. Returns an undo function."""
    undo = []
    for st in unet.spatial_transformers():
        for blk in st.blocks:
            attn, orig = blk.attn1, blk.attn1.forward

            def wrapped(x, context=None, window=None, _st=st, _orig=orig):
                assert window is None
                hw = _st._seen_hw
                nh, nw = ops.hypertile_windows(64, 64, hw[0], hw[1],
                                               _st.hypertile_depth, 256)
                if nh * nw == 1:
                    return _orig(x, context)
                win = (hw[0] // nh, hw[1] // nw)
                out = _orig(ops.window_split(x, hw, win), context)
                return ops.window_merge(out, hw, win)

            attn.forward = wrapped
            undo.append((attn, orig))
        fwd = st.forward

        def spy(x, context, _st=st, _fwd=fwd):
            _st._seen_hw = tuple(x.shape[2:])
            return _fwd(x, context)

        st.forward = spy
        undo.append((st, fwd))
    return lambda: [setattr(m, "forward", f) for m, f in undo]


class TestUNet:
    def test_on_differs_and_equals_explicit_rearrange(self):
        torch.manual_seed(5)
        unet = UNetModel(UNetConfig.tiny()).eval()
        x = torch.randn(2, 4, 32, 32)
        ctx = torch.randn(2, 5, 64)
        t = torch.tensor([500, 20])
        with torch.no_grad():
            off = unet(x, t, ctx)
            unet.set_hypertile(True, 64, 64)
            plan = unet.hypertile_plan(32, 32)
            assert plan == ((32, 32, 16, 16), None, None, None,
                            (32, 32, 16, 16), (32, 32, 16, 16), None)
            on = unet(x, t, ctx)
            unet.set_hypertile(False)
            assert not any(unet.hypertile_plan(32, 32))
            assert torch.equal(unet(x, t, ctx), off)
            undo = _wrap_attn1(unet)
            wrapped = unet(x, t, ctx)
            undo()
        assert not torch.equal(on, off)
        assert torch.equal(on, wrapped)

    def test_only_self_attention_gets_the_window(self):
        torch.manual_seed(6)
        blk = BasicTransformerBlock(32, 16, 2).eval()
        seen = []
        for name in ("attn1", "attn2"):
            attn = getattr(blk, name)

            def spy(x, context=None, window=None, _n=name,
                    _f=attn.forward):
                seen.append((_n, context is None, window))
                return _f(x, context, window)

            attn.forward = spy
        with torch.no_grad():
            blk(torch.randn(1, 64, 32), torch.randn(1, 5, 16), (8, 8),
                (8, 8, 4, 4))
        assert seen == [("attn1", True, (8, 8, 4, 4)), ("attn2", False, None)]
        # a context makes CrossAttention ignore a window it is handed
        attn = CrossAttention(32, 16, 2).eval()
        x, ctx = torch.randn(1, 64, 32), torch.randn(1, 5, 16)
        with torch.no_grad():
            assert torch.equal(attn(x, ctx, window=(8, 8, 4, 4)),
                               attn(x, ctx))

    def test_token_merging_takes_precedence(self):
        torch.manual_seed(7)
        blk = BasicTransformerBlock(32, 16, 2).eval()
        x, ctx = torch.randn(2, 64, 32), torch.randn(2, 5, 16)
        win = (8, 8, 4, 4)
        with torch.no_grad():
            plain = blk(x, ctx, (8, 8))
            windowed = blk(x, ctx, (8, 8), win)
            assert not torch.equal(windowed, plain)
            blk.tome_ratio = 0.5
            merged = blk(x, ctx, (8, 8))
            assert torch.equal(blk(x, ctx, (8, 8), win), merged)
            blk.tome_ratio = 0.01  # r = 0: the block is windowed as usual
            assert torch.equal(blk(x, ctx, (8, 8), win), windowed)


# ---------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe():
    return StableDiffusionPipeline(
        load_model("tiny", device="cpu", dtype=torch.float32, cache=False),
        device="cpu", dtype=torch.float32,
    )


REQ = dict(prompt="cows", steps=2, width=64, height=64, seeds=[5, 6])
HR = dict(enable_hr=True, hr_scale=2.0, hr_steps=1)


class TestPipeline:
    def test_on_off_and_infotext(self, pipe):
        plain = pipe.generate(PipelineRequest(**REQ))
        assert "Hypertile" not in plain.infotexts[0]
        on = pipe.generate(PipelineRequest(**REQ, hypertile_unet=True))
        assert not torch.equal(on.images, plain.images)
        info = parse_infotext(on.infotexts[0])
        assert info["Hypertile U-Net"] == "True"
        assert info["hypertile_unet"] == "True"
        assert "Hypertile U-Net max depth" not in info
        assert "Hypertile U-Net max tile size" not in info
        assert "Hypertile U-Net second pass" not in info
        again = pipe.generate(PipelineRequest(**REQ, hypertile_unet=True))
        assert torch.equal(on.images, again.images)
        # depth 0 only is the same cut here (level 1 is whole anyway), and
        # it reports itself
        d0 = pipe.generate(PipelineRequest(**REQ, hypertile_unet=True,
                                           hypertile_max_depth=0,
                                           hypertile_max_tile=128))
        assert torch.equal(d0.images, on.images)
        info = parse_infotext(d0.infotexts[0])
        assert info["hypertile_max_depth"] == "0"
        assert info["hypertile_max_tile"] == "128"
        # and back: the switch leaves nothing behind
        assert torch.equal(pipe.generate(PipelineRequest(**REQ)).images,
                           plain.images)
        assert pipe._hypertile_plan is None

    def test_graph_caches_follow_the_windows(self, pipe):
        from types import SimpleNamespace

        on = PipelineRequest(**REQ, hypertile_unet=True)
        pipe.generate(on)
        wrapper = SimpleNamespace(cache={"shape": object()})
        pipe._wholestep_cache["sentinel"] = wrapper
        pipe._denoiser.cache["sentinel"] = object()
        pipe.generate(on)  # the same windows: the caches stay
        assert "sentinel" in pipe._wholestep_cache and wrapper.cache
        assert "sentinel" in pipe._denoiser.cache
        # other settings, the same effective windows: they stay too
        pipe.generate(replace(on, hypertile_max_depth=0))
        assert "sentinel" in pipe._wholestep_cache and wrapper.cache
        pipe.generate(PipelineRequest(**REQ))  # off: other launches
        assert "sentinel" not in pipe._wholestep_cache
        assert "sentinel" not in pipe._denoiser.cache
        assert not wrapper.cache  # a wrapper still held by a pass is emptied
        pipe._wholestep_cache["sentinel"] = wrapper
        pipe.generate(on)
        assert "sentinel" not in pipe._wholestep_cache

    def test_hires_pass_gets_windows_from_the_hires_size(self, pipe):
        calls = []
        unet = pipe.model.unet
        set_hypertile = unet.set_hypertile

        def spy(enabled, width=0, height=0, max_depth=3, max_tile=256):
            calls.append((enabled, width, height, max_depth, max_tile))
            return set_hypertile(enabled, width, height, max_depth, max_tile)

        unet.set_hypertile = spy
        # what the attention itself is handed (at 4096 near-uniform tokens
        # the tiny model's images move by less than one uint8 step, so the
        # images cannot show the hires windows)
        grids = []
        windowed = ops.attention_window_bshd

        def attn_spy(q, k, v, grid, window, scale=None, native=True):
            grids.append((tuple(grid), tuple(window)))
            return windowed(q, k, v, grid, window, scale, native)

        mp = pytest.MonkeyPatch()
        mp.setattr(ops, "attention_window_bshd", attn_spy)
        try:
            one = {**REQ, "seeds": [5]}
            res = pipe.generate(PipelineRequest(**one, **HR,
                                                hypertile_unet=True))
            assert calls == [(True, 64, 64, 3, 256), (True, 128, 128, 3, 256)]
            # 128x128 pixels: P = 128, L = 16, the 64x64 latent is cut 4x4
            assert pipe._hypertile_plan[0] == (64, 64, 16, 16)
            assert set(grids) == {((32, 32), (16, 16)), ((64, 64), (16, 16))}
            assert grids[-1] == ((64, 64), (16, 16))
            grids.clear()
            info = parse_infotext(res.infotexts[0])
            assert info["Hypertile U-Net"] == "True"
            assert "Hypertile U-Net second pass" not in info
            calls.clear()
            second = pipe.generate(PipelineRequest(
                **one, **HR, hypertile_unet_secondpass=True))
            assert calls == [(False, 64, 64, 3, 256),
                             (True, 128, 128, 3, 256)]
            info = parse_infotext(second.infotexts[0])
            assert "Hypertile U-Net" not in info
            assert info["Hypertile U-Net second pass"] == "True"
            assert info["hypertile_unet_secondpass"] == "True"
            assert set(grids) == {((64, 64), (16, 16))}  # the hires pass only
            assert not torch.equal(second.images, res.images)
            calls.clear()
            grids.clear()
            pipe.generate(PipelineRequest(**one, **HR))
            assert calls == [(False, 64, 64, 3, 256),
                             (False, 128, 128, 3, 256)]
            assert not grids
        finally:
            mp.undo()
            del unet.set_hypertile

    def test_second_pass_only_leaves_the_first_pass_alone(self, pipe):
        one = {**REQ, "seeds": [5]}
        off = pipe.generate(PipelineRequest(**one))
        only2 = pipe.generate(PipelineRequest(
            **one, hypertile_unet_secondpass=True))
        assert torch.equal(off.images, only2.images)  # no hires pass at all
        assert only2.infotexts == off.infotexts
        # with a hires pass: the first pass's latents are bit-equal to off
        firsts = []
        upscale = pipe_module()._upscale_latent

        def spy(x, *a, **kw):
            firsts.append(x.clone())
            return upscale(x, *a, **kw)

        mp = pytest.MonkeyPatch()
        mp.setattr(pipe_module(), "_upscale_latent", spy)
        try:
            pipe.generate(PipelineRequest(**one, **HR))
            pipe.generate(PipelineRequest(**one, **HR,
                                          hypertile_unet_secondpass=True))
            pipe.generate(PipelineRequest(**one, **HR, hypertile_unet=True))
        finally:
            mp.undo()
        assert len(firsts) == 3
        assert torch.equal(firsts[0], firsts[1])
        assert not torch.equal(firsts[0], firsts[2])


def pipe_module():
    import sdwd_amd.pipeline.pipeline as mod

    return mod


# ---------------------------------------------------------------------------
# engine: a shard of a batch equals the whole batch
# ---------------------------------------------------------------------------
class TestEngine:
    def test_two_rank_gallery_equals_one_rank(self, monkeypatch):
        """Exact, image for image. As in tests/test_tome_cpu.py the UNet
        forward is a stand-in whose only library math is the model's own
        level-0 SpatialTransformer (real weights, the real windowed
        attention): the tiny UNet's convolutions round differently at
        different batch sizes, which says nothing about Hypertile. The off
        run shows that the stand-in itself shards exactly."""
        from sdwd_amd.parallel import GenerationRequest, LocalEngine

        batches = []
        windowed = ops.attention_window_bshd

        def spy(q, k, v, grid, window, scale=None, native=True):
            batches.append((q.shape[0], tuple(grid), tuple(window)))
            return windowed(q, k, v, grid, window, scale, native)

        monkeypatch.setattr(ops, "attention_window_bshd", spy)

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
        for on in (False, True):
            batches.clear()
            one, two = (e.generate(replace(gen, hypertile_unet=on))
                        for e in engines)
            assert one.images.shape == (4, 64, 64, 3)
            assert torch.equal(one.images, two.images), on
            assert one.infotexts == [
                t.replace("gpu1", "gpu0") for t in two.infotexts]
            assert bool(batches) == on
            galleries[on] = one
        # the 2-rank run attended in shards of 2 images (4 rows with CFG)
        assert {b[0] for b in batches} == {8, 4}
        assert all(b[1:] == ((32, 32), (16, 16)) for b in batches)
        assert not torch.equal(galleries[False].images,
                               galleries[True].images)
        assert all("Hypertile U-Net: True" in t
                   for t in galleries[True].infotexts)


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
DEFAULTS = {
    "hypertile_enable_unet": False,
    "hypertile_enable_unet_secondpass": False,
    "hypertile_max_depth_unet": 3,
    "hypertile_max_tile_unet": 256,
    "hypertile_swap_size_unet": 1,
    "hypertile_enable_vae": False,
}


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
        assert {k: opts[k] for k in DEFAULTS} == DEFAULTS
        plain, info0 = _post(client)
        assert "Hypertile" not in info0
        try:
            _set(client, hypertile_enable_unet=True,
                 hypertile_max_tile_unet=128, hypertile_swap_size_unet=4,
                 hypertile_enable_vae=True)
            opts = client.get("/sdapi/v1/options").json()
            assert opts["hypertile_enable_unet"] is True
            assert opts["hypertile_max_tile_unet"] == 128
            assert opts["hypertile_max_depth_unet"] == 3
            img, info = _post(client)
            assert "Hypertile U-Net: True" in info
            assert "Hypertile U-Net max tile size: 128" in info
            assert img != plain
        finally:
            _set(client, **DEFAULTS)
        assert _post(client) == (plain, info0)

    def test_override_beats_option_and_does_not_stick(self, client):
        plain, _ = _post(client)
        img, info = _post(client,
                          override_settings={"hypertile_enable_unet": True})
        assert "Hypertile U-Net: True" in info
        assert base64.b64decode(img) != base64.b64decode(plain)
        assert _post(client)[0] == plain
        try:
            _set(client, hypertile_enable_unet=True)
            assert _post(client)[0] == img
            got, info = _post(
                client, override_settings={"hypertile_enable_unet": False})
            assert got == plain and "Hypertile" not in info
            # the swap size is accepted and changes nothing
            assert _post(client, override_settings={
                "hypertile_swap_size_unet": 3})[0] == img
        finally:
            _set(client, hypertile_enable_unet=False)

    @pytest.mark.parametrize("key,value", [
        ("hypertile_enable_unet", 1),
        ("hypertile_enable_unet", "yes"),
        ("hypertile_enable_unet_secondpass", None),
        ("hypertile_max_depth_unet", 4),
        ("hypertile_max_depth_unet", -1),
        ("hypertile_max_depth_unet", 1.5),
        ("hypertile_max_depth_unet", True),
        ("hypertile_max_depth_unet", "2"),
        ("hypertile_max_tile_unet", 513),
        ("hypertile_max_tile_unet", -8),
        ("hypertile_max_tile_unet", [256]),
        ("hypertile_swap_size_unet", 0),
    ])
    def test_bad_values_are_422_naming_the_key(self, client, key, value):
        r = client.post("/sdapi/v1/options", json={key: value})
        assert r.status_code == 422 and key in r.text
        r = client.post("/sdapi/v1/txt2img",
                        json={**BODY, "override_settings": {key: value}})
        assert r.status_code == 422 and key in r.text
        opts = client.get("/sdapi/v1/options").json()
        assert {k: opts[k] for k in DEFAULTS} == DEFAULTS

    def test_nan_is_422(self, client):
        # JSON itself has no NaN; the Python client's encoder writes the
        # literal that lenient senders use
        for key in ("hypertile_max_depth_unet", "hypertile_max_tile_unet"):
            r = client.post(
                "/sdapi/v1/options", content='{"%s": NaN}' % key,
                headers={"Content-Type": "application/json"})
            assert r.status_code == 422

    def test_infotext_round_trip(self, client):
        ov = {"hypertile_enable_unet": True, "hypertile_max_depth_unet": 1,
              "hypertile_max_tile_unet": 128}
        img, info = _post(client, override_settings=ov)
        parsed = parse_infotext(info)
        assert parsed["Hypertile U-Net"] == "True"
        assert parsed["Hypertile U-Net max depth"] == "1"
        assert parsed["Hypertile U-Net max tile size"] == "128"
        again, info2 = _post(client, seed=int(parsed["Seed"]),
                             override_settings={
            "hypertile_enable_unet": parsed["hypertile_unet"] == "True",
            "hypertile_max_depth_unet": int(parsed["hypertile_max_depth"]),
            "hypertile_max_tile_unet": int(parsed["hypertile_max_tile"]),
        })
        assert again == img and info2 == info

    def test_raw_grammar_round_trip(self):
        line = ("Steps: 2, Sampler: Euler a, CFG scale: 7.0, Seed: 1, "
                "Size: 64x64, Model: tiny, Hypertile U-Net: True, "
                "Hypertile U-Net second pass: True, "
                "Hypertile U-Net max depth: 2, "
                "Hypertile U-Net max tile size: 128")
        parsed = parse_infotext("a cow\nNegative prompt: fence\n" + line)
        assert parsed["prompt"] == "a cow"
        assert parsed["hypertile_unet"] == "True"
        assert parsed["hypertile_unet_secondpass"] == "True"
        assert parsed["hypertile_max_depth"] == "2"
        assert parsed["hypertile_max_tile"] == "128"
        rebuilt = ", ".join(
            f"{k}: {v}" for k, v in parsed.items()
            if k[0].isupper())
        assert rebuilt == line

    def test_second_pass_option(self, client):
        hr = dict(enable_hr=True, hr_scale=2.0, hr_second_pass_steps=1,
                  denoising_strength=0.5)
        _, info = _post(client, **hr, override_settings={
            "hypertile_enable_unet_secondpass": True})
        parsed = parse_infotext(info)
        assert "Hypertile U-Net" not in parsed
        assert parsed["Hypertile U-Net second pass"] == "True"
        # without a hires pass the switch does nothing and says nothing
        _, info = _post(client, override_settings={
            "hypertile_enable_unet_secondpass": True})
        assert "Hypertile" not in info

    def test_ui_has_the_checkbox(self, client):
        page = client.get("/").text
        assert 'id="hypertile"' in page and "hypertile_enable_unet" in page


class TestXYZ:
    def test_axes(self):
        from sdwd_amd.parallel import GenerationRequest, LocalEngine
        from sdwd_amd.parallel.xyz import resolve_axis, run_xyz

        names = ("Hypertile U-Net first pass enabled",
                 "Hypertile U-Net second pass enabled",
                 "Hypertile U-Net max depth",
                 "Hypertile U-Net max tile size")
        for name in names:
            assert resolve_axis(name).name == name
        assert resolve_axis("[Hypertile] Unet First pass Enabled").name \
            == names[0]
        assert resolve_axis("hypertile_max_tile_unet").name == names[3]
        gen = GenerationRequest(prompt="a cow", batch_size=1, width=64,
                                height=64, steps=2, seed=11)
        g = resolve_axis(names[0]).apply(gen, "True")
        assert g.hypertile_unet is True
        assert resolve_axis(names[1]).apply(gen, "false") \
            .hypertile_unet_secondpass is False
        assert resolve_axis(names[2]).apply(gen, 2).hypertile_max_depth == 2
        assert resolve_axis(names[3]).apply(gen, 128).hypertile_max_tile \
            == 128
        with pytest.raises(ValueError):
            resolve_axis(names[0]).apply(gen, "maybe")
        with pytest.raises(ValueError):
            resolve_axis(names[2]).apply(gen, 4)
        with pytest.raises(ValueError):
            resolve_axis(names[3]).apply(gen, 1024)
        eng = LocalEngine(model="tiny", devices=["cpu"])
        for w in eng.world.workers:
            w.eta.avg_ipm = 60.0
        out = run_xyz(eng, gen, names[0], "False, True", 0, "")
        assert out["labels"]["x_values"] == ["False", "True"]
        assert not torch.equal(out["grid"][:, :64], out["grid"][:, 64:])
        params = [t.split("\n")[2] for t in out["infotexts"]]
        assert "Hypertile U-Net: True" in params[1]
        assert "Hypertile" not in params[0]
