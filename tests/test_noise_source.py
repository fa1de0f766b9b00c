"""The noise sources of sdwd_amd/pipeline/noise.py through the CPU pipeline,
the samplers, the engine, the API, the infotext and the X/Y/Z script.

Shard invariance is asserted exactly, tensor for tensor. The tiny UNet's
BLAS reductions depend on the batch size at the last bit (see
tests/test_pipeline.py::TestTxt2Img::test_shard_equals_whole_batch), which
has nothing to do with where the noise comes from, so these runs replace the
UNet's forward with an elementwise function of its input: everything else
(the request plumbing, CFG, the samplers, the noise source, the hires pass)
is the real generation path, and its result must not move by one bit when
the batch is split.
"""
import base64
import json
from unittest import mock

import pytest
import torch

from sdwd_amd import ops
from sdwd_amd.models import load_model
from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline
from sdwd_amd.pipeline import noise as noise_mod
from sdwd_amd.pipeline.noise import CpuNoise, PhiloxNoise
from sdwd_amd.pipeline.samplers import build_sampler
from sdwd_amd.pipeline.schedule import schedule_for
from sdwd_amd.utils.infotext import parse_infotext

SEEDS = [100, 2 ** 32 + 7, 102, 2 ** 63 - 1]


@pytest.fixture(scope="module")
def pipe():
    p = StableDiffusionPipeline(
        load_model("tiny", device="cpu", dtype=torch.float32, cache=False),
        device="cpu", dtype=torch.float32,
    )

    def elementwise_unet(x, ts, ctx, y=None, control=None):
        return torch.tanh(x) * 0.5 + 0.01 * ts.view(-1, 1, 1, 1) / 1000.0

    p.model.unet.forward = elementwise_unet
    return p


def _latents(pipe, seeds, **kw):
    base = dict(prompt="cows", steps=3, width=64, height=64,
                sampler_name="Euler a", randn_source="NV")
    base.update(kw)
    sub = base.pop("subseeds", None)
    req = PipelineRequest(**base, seeds=list(seeds),
                          subseeds=list(sub) if sub else [])
    return pipe.generate(req, decode=False).images


class TestShardInvariance:
    @pytest.mark.parametrize("kw", [
        {},
        {"subseed_strength": 0.4},
        {"eta_noise_seed_delta": 31337},
        {"enable_hr": True, "hr_scale": 2.0, "hr_steps": 2,
         "denoising_strength": 0.6},
    ], ids=["plain", "subseed", "ensd", "hires"])
    def test_four_equals_two_plus_two(self, pipe, kw):
        subs = [7, 8, 9, 10] if "subseed_strength" in kw else None
        whole = _latents(pipe, SEEDS, subseeds=subs, **kw)
        a = _latents(pipe, SEEDS[:2], subseeds=subs and subs[:2], **kw)
        b = _latents(pipe, SEEDS[2:], subseeds=subs and subs[2:], **kw)
        assert whole.shape[0] == 4
        assert torch.isfinite(whole).all()
        assert torch.equal(torch.cat([a, b]), whole)
        # and the variation is live: it changes the result
        if kw:
            assert not torch.equal(whole, _latents(pipe, SEEDS))

    def test_batch_position_does_not_matter(self, pipe):
        fwd = _latents(pipe, SEEDS)
        rev = _latents(pipe, SEEDS[::-1])
        assert torch.equal(fwd, rev.flip(0))


class TestSources:
    def test_nv_differs_from_cpu(self, pipe):
        nv = _latents(pipe, [5])
        cpu = _latents(pipe, [5], randn_source="CPU")
        assert not torch.equal(nv, cpu)
        assert torch.equal(cpu, _latents(pipe, [5], randn_source="cpu"))

    def test_default_is_cpu(self, pipe):
        assert PipelineRequest().randn_source == "CPU"
        base = dict(prompt="cows", steps=3, width=64, height=64, seeds=[5])
        a = pipe.generate(PipelineRequest(**base), decode=False).images
        assert torch.equal(a, _latents(pipe, [5], randn_source="CPU"))

    def test_cpu_source_is_the_old_formulas(self):
        """CpuNoise against the generator recipes written out: seed & M32,
        slerp towards the subseed noise, ((seed + ensd) ^ 0x5EED) & M32 step
        generators, seed ^ 0xF111 fill, (seed ^ 0x12E50) hires noise."""
        seeds, subs, ensd, shape = [3, 2 ** 33 + 1], [9, -1], 17, (4, 8, 8)
        src = CpuNoise(seeds, subs, 0.3, ensd, "cpu", torch.float32)

        def randn(seed):
            g = torch.Generator("cpu").manual_seed(seed & 0xFFFFFFFF)
            return torch.randn(shape, generator=g, dtype=torch.float32)

        init = src.initial(shape)
        want0 = noise_mod._slerp(randn(3), randn(9), 0.3)
        assert torch.equal(init[0], want0)
        assert torch.equal(init[1], randn(2 ** 33 + 1))  # subseed -1: none
        gens = [
            torch.Generator("cpu").manual_seed(((s + ensd) ^ 0x5EED) & 0xFFFFFFFF)
            for s in seeds
        ]
        src.shape = shape
        for _ in range(2):
            want = torch.stack([
                torch.randn(shape, generator=g, dtype=torch.float32)
                for g in gens
            ])
            assert torch.equal(src(), want)
        x = torch.ones(2, *shape)
        want = torch.stack([
            torch.randn(shape, generator=g, dtype=torch.float32) for g in gens
        ])
        assert torch.equal(src.add_to(x, 1.0, 0.5), x + 0.5 * want)
        assert torch.equal(
            src.fill(shape), torch.stack([randn(s ^ 0xF111) for s in seeds])
        )
        assert torch.equal(
            src.hires_initial(shape),
            torch.stack([randn(s ^ 0x12E50) for s in seeds]),
        )

    def test_unknown_source_raises(self, pipe):
        for bad in ("GPU", "philox", ""):
            with pytest.raises(ValueError, match="CPU, NV"):
                pipe.generate(PipelineRequest(
                    prompt="x", steps=1, width=64, height=64, seeds=[1],
                    randn_source=bad,
                ))
        from sdwd_amd.parallel import GenerationRequest

        with pytest.raises(ValueError, match="CPU, NV"):
            GenerationRequest(randn_source="GPU")
        assert GenerationRequest(randn_source="nv").randn_source == "NV"


class TestDrawSchedule:
    """initial = draw 0 of Generator(seed), step k = draw k; with ENSD the
    steps restart at draw 0 of Generator(seed + ensd); the hires pass keeps
    counting. Every expected tensor is recomputed with ops.philox_randn."""

    shape = (4, 8, 8)

    @pytest.mark.parametrize("ensd", [0, 31337])
    def test_generate_follows_the_schedule(self, pipe, ensd):
        seeds = [21, 2 ** 40 + 3]
        f = pipe.model.vae.cfg.downsample_factor
        shape = (pipe.model.latent_channels, 64 // f, 64 // f)
        draws, adds = [], []
        randn, add_to = ops.philox_randn, PhiloxNoise.add_to

        def spy_randn(sd, offset, shp, *a, **k):
            draws.append((list(sd), offset, tuple(shp)))
            return randn(sd, offset, shp, *a, **k)

        def spy_add_to(self, x, a, b):
            out = add_to(self, x, a, b)
            adds.append((x.clone(), a, b, out.clone()))
            return out

        with mock.patch.object(ops, "philox_randn", spy_randn), \
                mock.patch.object(PhiloxNoise, "add_to", spy_add_to):
            got = _latents(pipe, seeds, eta_noise_seed_delta=ensd)
        assert torch.equal(got, _latents(pipe, seeds,
                                         eta_noise_seed_delta=ensd))
        step_seeds = [s + ensd for s in seeds]
        first = 0 if ensd else 1
        # 3 steps, the last lands on sigma 0: the initial draw + 2 noisy steps
        assert draws == [
            (seeds, 0, shape),
            (step_seeds, first, shape),
            (step_seeds, first + 1, shape),
        ]
        assert len(adds) == 2
        for k, (x, a, b, out) in enumerate(adds):
            want = ops.add_noise(
                x, ops.philox_randn(step_seeds, first + k, shape), a, b
            )
            assert torch.equal(out, want), k

    def test_initial_noise_is_draw_zero(self, pipe):
        seeds = [21, 2 ** 40 + 3]
        src = PhiloxNoise(seeds, [-1, -1], 0.0, 0, "cpu", torch.float32)
        assert torch.equal(
            src.initial(self.shape), ops.philox_randn(seeds, 0, self.shape)
        )
        # a one-step run has no step noise: image i depends on seed i alone
        got = _latents(pipe, seeds, steps=1)
        other = _latents(pipe, [22, 2 ** 40 + 3], steps=1)
        assert torch.isfinite(got).all()
        assert not torch.equal(got[0], other[0])
        assert torch.equal(got[1], other[1])

    def test_subseed_is_draw_zero_of_its_own_generator(self):
        src = PhiloxNoise([5, 6], [77, -1], 0.25, 0, "cpu", torch.float32)
        init = src.initial(self.shape)
        a = ops.philox_randn([5], 0, self.shape)[0]
        b = ops.philox_randn([77], 0, self.shape)[0]
        assert torch.equal(init[0], noise_mod._slerp(a, b, 0.25))
        assert torch.equal(init[1], ops.philox_randn([6], 0, self.shape)[0])

    def test_hires_continues_and_fill_is_keyed(self):
        seeds = [5, 6]
        src = PhiloxNoise(seeds, [-1, -1], 0.0, 0, "cpu", torch.float32)
        src.initial(self.shape)
        src.shape = self.shape
        src(), src()
        big = (4, 16, 16)
        assert torch.equal(
            src.hires_initial(big), ops.philox_randn(seeds, 3, big)
        )
        src.shape = big
        assert torch.equal(src(), ops.philox_randn(seeds, 4, big))
        assert torch.equal(
            src.fill(self.shape),
            ops.philox_randn([s ^ 0xF111 for s in seeds], 0, self.shape),
        )
        # ENSD: steps on their own generator, hires noise on the main one
        src = PhiloxNoise(seeds, [-1, -1], 0.0, 9, "cpu", torch.float32)
        src.initial(self.shape)
        src.shape = self.shape
        assert torch.equal(
            src(), ops.philox_randn([14, 15], 0, self.shape)
        )
        assert torch.equal(
            src.hires_initial(big), ops.philox_randn(seeds, 1, big)
        )


class TestSamplerHelper:
    def _run(self, noise_fn, name="Euler a", steps=4):
        if name == "Restart":
            steps = 12  # enough steps for a restart band
        sampler = build_sampler(name, schedule_for(name, steps, "Automatic"))
        x = torch.ones(1, 4, 4, 4) * 10.0
        return sampler.sample(lambda xs, t: xs * 0.1, x, noise_fn=noise_fn)

    def test_plain_callable_still_works(self):
        calls = []

        def noise_fn():
            calls.append(1)
            return torch.full((1, 4, 4, 4), 0.5)

        out = self._run(noise_fn)
        assert torch.isfinite(out).all() and len(calls) == 3

    def test_add_to_is_preferred_and_object_never_called(self):
        class Source:
            def __init__(self):
                self.adds = []

            def __call__(self):
                raise AssertionError("the source must not be called")

            def add_to(self, x, a, b):
                self.adds.append((a, b))
                return ops.add_noise(x, torch.full_like(x, 0.5), a, b)

        src = Source()
        out = self._run(src)
        # 4 steps, the last has sigma_next = 0: three noisy steps
        assert len(src.adds) == 3 and all(a == 1.0 for a, _ in src.adds)
        plain = self._run(lambda: torch.full((1, 4, 4, 4), 0.5))
        assert torch.equal(out, plain)

    @pytest.mark.parametrize(
        "name", ["DPM2 a", "DPM++ 2S a", "DPM++ SDE", "DPM++ 2M SDE", "DDPM",
                 "LCM", "Restart"])
    def test_other_stochastic_samplers_use_add_to(self, name):
        class Source:
            adds = 0

            def __call__(self):
                raise AssertionError("the source must not be called")

            def add_to(self, x, a, b):
                Source.adds += 1
                return ops.add_noise(x, torch.full_like(x, 0.5), a, b)

        Source.adds = 0
        out = self._run(Source(), name=name)
        assert torch.isfinite(out).all() and Source.adds >= 1


# ---------------------------------------------------------------------------
# public surface: API, options, infotext, X/Y/Z
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


def _post(client, **extra):
    r = client.post("/sdapi/v1/txt2img", json={**BODY, **extra})
    assert r.status_code == 200, r.text
    body = r.json()
    return body["images"][-1], json.loads(body["info"])["infotexts"][0]


class TestApi:
    def test_per_request_override(self, client):
        img_cpu, info_cpu = _post(client)
        img_nv, info_nv = _post(
            client, override_settings={"randn_source": "NV"}
        )
        assert base64.b64decode(img_cpu) != base64.b64decode(img_nv)
        assert "RNG: NV" in info_nv and "RNG" not in info_cpu
        # the override did not stick
        assert _post(client)[0] == img_cpu
        assert _post(client, override_settings={"randn_source": "nv"})[0] \
            == img_nv

    def test_gpu_is_422(self, client):
        r = client.post("/sdapi/v1/txt2img", json={
            **BODY, "override_settings": {"randn_source": "GPU"},
        })
        assert r.status_code == 422
        assert "CPU" in r.text and "NV" in r.text
        r = client.post("/sdapi/v1/options", json={"randn_source": "GPU"})
        assert r.status_code == 422

    def test_options_round_trip(self, client):
        assert client.get("/sdapi/v1/options").json()["randn_source"] == "CPU"
        img_nv = _post(client, override_settings={"randn_source": "NV"})[0]
        try:
            r = client.post("/sdapi/v1/options", json={"randn_source": "NV"})
            assert r.status_code == 200
            opts = client.get("/sdapi/v1/options").json()
            assert opts["randn_source"] == "NV"
            assert "eta_noise_seed_delta" in opts
            img, info = _post(client)
            assert img == img_nv and "RNG: NV" in info
        finally:
            client.post("/sdapi/v1/options", json={"randn_source": "CPU"})
        assert client.get("/sdapi/v1/options").json()["randn_source"] == "CPU"

    def test_infotext_round_trip_with_ensd(self, client):
        img, info = _post(client, override_settings={
            "randn_source": "NV", "eta_noise_seed_delta": 31337,
        })
        parsed = parse_infotext(info)
        assert parsed["RNG"] == "NV" and parsed["randn_source"] == "NV"
        assert parsed["eta_noise_seed_delta"] == "31337"
        # feeding the parsed settings back reproduces the image
        again, info2 = _post(client, seed=int(parsed["Seed"]),
                             override_settings={
            "randn_source": parsed["randn_source"],
            "eta_noise_seed_delta": int(parsed["eta_noise_seed_delta"]),
        })
        assert again == img and info2 == info
        # without ENSD the picture is another one
        assert _post(client, override_settings={"randn_source": "NV"})[0] \
            != img

    def test_existing_infotexts_unchanged(self, client):
        _, info = _post(client)
        assert "RNG" not in info and "ENSD" not in info
        assert "randn_source" not in parse_infotext(info)


class TestXYZ:
    def test_rng_source_axis(self):
        from sdwd_amd.parallel import GenerationRequest, LocalEngine
        from sdwd_amd.parallel.xyz import resolve_axis, run_xyz

        assert resolve_axis("RNG source").name == "RNG source"
        assert resolve_axis("rng").name == "RNG source"
        eng = LocalEngine(model="tiny", devices=["cpu"])
        for w in eng.world.workers:
            w.eta.avg_ipm = 60.0
        gen = GenerationRequest(prompt="a cow", batch_size=1, width=64,
                                height=64, steps=2, seed=11)
        out = run_xyz(eng, gen, "RNG source", "CPU, NV", 0, "")
        assert out["labels"]["x_values"] == ["CPU", "NV"]
        assert not torch.equal(out["grid"][:, :64], out["grid"][:, 64:])
        assert "RNG: NV" in out["infotexts"][1]
        assert "RNG: NV" not in out["infotexts"][0]
        with pytest.raises(ValueError, match="CPU, NV"):
            run_xyz(eng, gen, "RNG source", "CPU, GPU", 0, "")
