"""Noise sources of a generation: where every normal the pipeline and the
samplers consume comes from.

Both sources keep the determinism contract of pipeline.py: the noise of image
k depends on (seed_k, subseed_k, request params) alone, never on the batch
position, the shard or the device count.

* ``CpuNoise`` ("CPU", the default): one ``torch.Generator("cpu")`` per image,
  drawn on the host and copied to the device.
* ``PhiloxNoise`` ("NV"): the counter-based Philox4x32-10 + Box-Muller stream
  of ``ops.philox_randn``. Draw k of image i is a pure function of
  (seed_i, k, element), so a noisy sampler step is one fused kernel launch
  (``ops.add_philox_noise``) with no host work, no copy and no sync.

A source is callable (``noise_fn()`` -> [B, *shape] on the pipeline device and
dtype, ``shape`` being the attribute the pipeline sets before each sampling
pass) and has ``add_to(x, a, b)`` = a*x + b*noise, which the samplers prefer.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import torch

from .. import ops

RANDN_SOURCES = ("CPU", "NV")

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
# per-purpose keys xor-ed into the image seed for draws outside the main
# stream (the values predate this module and are part of every stored seed)
KEY_STEP_CPU = 0x5EED    # CpuNoise step generators
KEY_FILL = 0xF111        # inpaint "latent noise" masked content
KEY_HIRES_CPU = 0x12E50  # CpuNoise hires second-pass initial noise
KEY_ENCODE = 0xE4C0DE    # VAE encoder sampling noise


def normalize_randn_source(value) -> str:
    """"CPU" or "NV" (case-insensitive); anything else is a ValueError that
    names the accepted values. The host application's "GPU" source is
    rejected on purpose: it is neither shard- nor device-invariant."""
    name = str(value if value is not None else "CPU").strip().upper()
    if name not in RANDN_SOURCES:
        raise ValueError(
            f"randn_source: unknown value {value!r} "
            f"(accepted: {', '.join(RANDN_SOURCES)})"
        )
    return name


def _slerp(a: torch.Tensor, b: torch.Tensor, t: float) -> torch.Tensor:
    """Spherical interpolation between noise tensors (subseed variation)."""
    af, bf = a.flatten().double(), b.flatten().double()
    dot = torch.dot(af / af.norm(), bf / bf.norm()).clamp(-1, 1)
    omega = torch.acos(dot)
    if omega.abs() < 1e-6:
        out = (1 - t) * af + t * bf
    else:
        so = torch.sin(omega)
        out = (math.sin((1 - t) * omega) / so) * af + (
            math.sin(t * omega) / so
        ) * bf
    return out.reshape(a.shape).to(a.dtype)


def _image_noise(
    seed: int,
    subseed: int,
    subseed_strength: float,
    shape,
) -> torch.Tensor:
    """Per-image deterministic CPU noise (device-independent)."""
    g = torch.Generator("cpu").manual_seed(int(seed) & 0xFFFFFFFF)
    noise = torch.randn(shape, generator=g, dtype=torch.float32)
    if subseed_strength and subseed_strength > 0 and subseed >= 0:
        g2 = torch.Generator("cpu").manual_seed(int(subseed) & 0xFFFFFFFF)
        noise2 = torch.randn(shape, generator=g2, dtype=torch.float32)
        noise = _slerp(noise, noise2, float(subseed_strength))
    return noise


def keyed_noise(
    randn_source: str, seeds: Sequence[int], key: int, shape, device
) -> torch.Tensor:
    """fp32 [B, *shape] on `device`: draw 0 of a fresh generator seeded
    ``seed_i ^ key`` per image (inpaint fill, encoder sampling noise)."""
    if normalize_randn_source(randn_source) == "NV":
        return ops.philox_randn(
            [(int(s) ^ key) & _M64 for s in seeds], 0, shape,
            torch.float32, device,
        )
    return torch.stack([
        torch.randn(
            tuple(shape),
            generator=torch.Generator("cpu").manual_seed(
                (int(s) ^ key) & _M32
            ),
            dtype=torch.float32,
        )
        for s in seeds
    ]).to(device)


class CpuNoise:
    """Host generators, one per image (the default source)."""

    randn_source = "CPU"

    def __init__(self, seeds: Sequence[int], subseeds: Sequence[int],
                 subseed_strength: float, ensd: int, device, dtype) -> None:
        self.seeds = [int(s) for s in seeds]
        self.subseeds = [int(s) for s in subseeds]
        self.subseed_strength = float(subseed_strength)
        self.device = torch.device(device)
        self.dtype = dtype
        self.shape = None  # per-image shape of the step noise
        # ancestral noise: per-image generators stepped identically
        # regardless of shard composition
        self._gens = [
            torch.Generator("cpu").manual_seed(
                ((s + int(ensd)) ^ KEY_STEP_CPU) & _M32
            )
            for s in self.seeds
        ]

    def initial(self, shape) -> torch.Tensor:
        """fp32 initial latent noise [B, *shape] (seed, slerped towards the
        subseed noise by subseed_strength)."""
        return torch.stack([
            _image_noise(sd, sub, self.subseed_strength, tuple(shape))
            for sd, sub in zip(self.seeds, self.subseeds)
        ])

    def hires_initial(self, shape) -> torch.Tensor:
        """fp32 noise the hires second pass adds before it denoises."""
        return keyed_noise("CPU", self.seeds, KEY_HIRES_CPU, shape, "cpu")

    def fill(self, shape) -> torch.Tensor:
        return keyed_noise("CPU", self.seeds, KEY_FILL, shape, self.device)

    def __call__(self) -> torch.Tensor:
        n = torch.stack([
            torch.randn(tuple(self.shape), generator=g, dtype=torch.float32)
            for g in self._gens
        ])
        return n.to(self.device, self.dtype)

    def add_to(self, x: torch.Tensor, a: float, b: float) -> torch.Tensor:
        return ops.add_noise(x, self(), a, b)


class _PhiloxGen:
    """A batch of Philox generators that draw in lockstep: the device seed
    table (uploaded once) and the shared host-side offset."""

    def __init__(self, seeds: List[int], device) -> None:
        table = [s & _M64 for s in seeds]
        if torch.device(device).type != "cpu":
            table = ops._philox_seeds(table, device)  # the one upload
        self.table = table
        self.offset = 0

    def take(self) -> int:
        off = self.offset
        self.offset += 1
        return off


class PhiloxNoise:
    """The "NV" source. Generator(seed_i): draw 0 is the initial noise, the
    step noise continues at draws 1, 2, ... and the hires second pass keeps
    counting on the same generator. With eta_noise_seed_delta != 0 the step
    noise comes from a fresh Generator(seed_i + ensd) instead, from draw 0
    (the host application's rule). Subseed noise is draw 0 of
    Generator(subseed_i)."""

    randn_source = "NV"

    def __init__(self, seeds: Sequence[int], subseeds: Sequence[int],
                 subseed_strength: float, ensd: int, device, dtype) -> None:
        self.seeds = [int(s) for s in seeds]
        self.subseeds = [int(s) for s in subseeds]
        self.subseed_strength = float(subseed_strength)
        self.device = torch.device(device)
        self.dtype = dtype
        self.shape = None
        self._main = _PhiloxGen(self.seeds, self.device)
        self._step = self._main if int(ensd) == 0 else _PhiloxGen(
            [s + int(ensd) for s in self.seeds], self.device
        )

    def _draw(self, gen: _PhiloxGen, shape, dtype) -> torch.Tensor:
        return ops.philox_randn(
            gen.table, gen.take(), tuple(shape), dtype, self.device
        )

    def initial(self, shape) -> torch.Tensor:
        noise = self._draw(self._main, shape, torch.float32)
        if self.subseed_strength > 0:
            for i, sub in enumerate(self.subseeds):
                if sub < 0:
                    continue
                other = ops.philox_randn(
                    [sub & _M64], 0, tuple(shape), torch.float32, self.device
                )[0]
                noise[i] = _slerp(noise[i], other, self.subseed_strength)
        return noise

    def hires_initial(self, shape) -> torch.Tensor:
        return self._draw(self._main, shape, torch.float32)

    def fill(self, shape) -> torch.Tensor:
        return keyed_noise("NV", self.seeds, KEY_FILL, shape, self.device)

    def __call__(self) -> torch.Tensor:
        return self._draw(self._step, self.shape, self.dtype)

    def add_to(self, x: torch.Tensor, a: float, b: float) -> torch.Tensor:
        if x.is_cuda and x.dim() == 4:
            # one launch: the normals never touch memory
            return ops.add_philox_noise(
                x, self._step.table, self._step.take(), a, b
            )
        return ops.add_noise(x, self(), a, b)


def make_noise_source(randn_source: str, seeds, subseeds, subseed_strength,
                      ensd, device, dtype):
    cls = PhiloxNoise if normalize_randn_source(randn_source) == "NV" \
        else CpuNoise
    return cls(seeds, subseeds, subseed_strength, ensd, device, dtype)
