"""GPU tests of the Philox kernels (sdwd_amd/ops/hip/rng.hip) against the CPU
ops, and of the "NV" noise source through the GPU pipeline.

Words are compared bit for bit. Normals: both the CPU op and the kernel are
fp32 implementations of the stream, each within the bound of
tests/philox_oracle.py of the exact value with its own libm's ulp figures,
so

    |gpu - cpu| <= bound(ULP_CPU) + bound(ULP_DEVICE)

per element, with s and r of the bound taken from the fp64 reference. The
ulp figures and where they come from are in philox_oracle's docstring (CPU:
SLEEF logf 1.0 / sinf 3.5, sqrt correctly rounded; device: the OpenCL C
relative-error table the ROCm device library is written to, log 3 / sin 4 /
sqrt 3). Elements with u >= 1 - 2^-20 are left out of the normals
comparison as in tests/test_philox_cpu.py; none of the fixed draws below
has one (asserted).

add_philox_noise: the reference is the CPU op on the same x, and

    |gpu - ref| <= |b| * (normals bound) + 2^-9 |ref|          (bf16)
    |gpu - ref| <= |b| * (normals bound) + 2^-23 (|b r| + |ref|) (fp32)

The bf16 term is the one output rounding; the fp32 term is the rounding of
b*r and of the sum on either side (2 * 2^-24 each).
"""
from unittest import mock

import numpy as np
import pytest
import torch

from philox_oracle import (KNOWN, OFFSETS, SEEDS, ULP_CPU, ULP_DEVICE,
                           Draw)
from sdwd_amd import ops

pytestmark = pytest.mark.gpu

B3_SEEDS = [1, 2 ** 32 + 7, 2 ** 63 - 1]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _normals_bound(seeds, offset, n):
    """[B, n] bound and keep mask of |gpu - cpu| from the fp64 reference."""
    ds = [Draw(s, offset, n) for s in seeds]
    bound = np.stack([d.bound(ULP_CPU) + d.bound(ULP_DEVICE) for d in ds])
    keep = np.stack([d.keep for d in ds])
    r = np.stack([d.r for d in ds])
    return torch.from_numpy(bound), torch.from_numpy(keep), torch.from_numpy(r)


class TestWords:
    def test_known_answers(self, dev):
        c = torch.tensor([k[0] for k in KNOWN], dtype=torch.int64, device=dev)
        k = torch.tensor([k[1] for k in KNOWN], dtype=torch.int64, device=dev)
        want = torch.tensor([k[2] for k in KNOWN], dtype=torch.int64)
        assert torch.equal(ops.philox4x32(c, k).cpu(), want)

    def test_random_pairs_match_cpu(self, dev):
        g = torch.Generator().manual_seed(4096)
        c = torch.randint(0, 1 << 32, (4096, 4), generator=g)
        k = torch.randint(0, 1 << 32, (4096, 2), generator=g)
        got = ops.philox4x32(c.to(dev), k.to(dev)).cpu()
        assert torch.equal(got, ops.philox4x32(c, k))


class TestRandn:
    @pytest.mark.parametrize("offset", OFFSETS)
    def test_matches_cpu_op(self, dev, offset):
        shape = (3, 37, 37)  # n = 4107: odd, vector groups straddle images
        n = 3 * 37 * 37
        for seeds in (B3_SEEDS, [SEEDS[0]] + B3_SEEDS[:2]):
            cpu = ops.philox_randn(seeds, offset, shape)
            gpu = ops.philox_randn(seeds, offset, shape, device=dev)
            assert gpu.shape == cpu.shape and gpu.dtype == torch.float32
            bound, keep, _ = _normals_bound(seeds, offset, n)
            assert bool(keep.all())
            err = (gpu.cpu().double() - cpu.double()).abs().reshape(3, n)
            ratio = (err / bound).max().item()
            print(f"offset {offset}: worst err/bound {ratio:.3f}")
            assert ratio <= 1.0

    def test_device_seed_table_and_bf16(self, dev):
        table = ops._philox_seeds(B3_SEEDS, dev)
        a = ops.philox_randn(table, 2, (4, 5, 7), device=dev)
        b = ops.philox_randn(B3_SEEDS, 2, (4, 5, 7), device=dev)
        assert torch.equal(a, b)
        h = ops.philox_randn(table, 2, (4, 5, 7), torch.bfloat16, dev)
        assert h.dtype == torch.bfloat16
        assert torch.equal(h, a.to(torch.bfloat16))  # one rounding of fp32


CASES = [
    (torch.bfloat16, 3, (4, 5, 7), False),  # n = 140, n % 8 == 4, tail
    (torch.bfloat16, 3, (4, 5, 7), True),   # + channels_last index map
    (torch.bfloat16, 2, (4, 8, 8), False),  # all-vector path
    (torch.float32, 3, (4, 5, 7), False),   # fp32 I/O
]


class TestAddPhiloxNoise:
    @pytest.mark.parametrize("dtype,b,chw,cl", CASES)
    def test_matches_cpu_op(self, dev, dtype, b, chw, cl):
        a_, b_, offset = 1.0, 0.37, 3
        seeds = B3_SEEDS[:b]
        g = torch.Generator().manual_seed(7)
        x = torch.randn(b, *chw, generator=g).to(dtype)
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        ref = ops.add_philox_noise(x, seeds, offset, a_, b_)
        got = ops.add_philox_noise(x.to(dev), seeds, offset, a_, b_)
        assert got.dtype == dtype and got.shape == x.shape
        assert got.stride() == x.stride()  # keeps x's memory format
        n = chw[0] * chw[1] * chw[2]
        nb, keep, r = _normals_bound(seeds, offset, n)
        assert bool(keep.all())
        refd = ref.double().reshape(b, n)
        if dtype == torch.bfloat16:
            bound = abs(b_) * nb + 2.0 ** -9 * refd.abs()
        else:
            bound = abs(b_) * nb + 2.0 ** -23 * (
                abs(b_) * r.abs() + refd.abs()
            )
        err = (got.cpu().double().reshape(b, n) - refd).abs()
        ratio = (err / bound).max().item()
        print(f"{dtype} {chw} cl={cl}: worst err/bound {ratio:.3f}")
        assert ratio <= 1.0

    def test_view_at_odd_offset(self, dev):
        x = torch.randn(3, 4, 5, 7, device=dev, dtype=torch.bfloat16)
        v = x[1:]  # 280 B into the buffer: not 16 B aligned
        got = ops.add_philox_noise(v, B3_SEEDS[1:], 3, 1.0, 0.37)
        want = ops.add_philox_noise(v.clone(), B3_SEEDS[1:], 3, 1.0, 0.37)
        assert torch.equal(got, want)


class TestPipelineGPU:
    BASE = dict(prompt="gpu cow", steps=3, width=64, height=64,
                sampler_name="Euler a", randn_source="NV")

    def test_fused_route_and_no_host_randn(self, dev):
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline
        from sdwd_amd.pipeline.noise import PhiloxNoise

        pipe = StableDiffusionPipeline("tiny", device=dev)
        adds, launches = [], []
        add_to, fused = PhiloxNoise.add_to, ops.add_philox_noise

        def spy_add_to(self, x, a, b):
            adds.append(x.is_cuda)
            return add_to(self, x, a, b)

        def spy_fused(x, seeds, offset, a, b):
            launches.append((offset, torch.is_tensor(seeds) and seeds.is_cuda))
            return fused(x, seeds, offset, a, b)

        with mock.patch.object(PhiloxNoise, "add_to", spy_add_to), \
                mock.patch.object(ops, "add_philox_noise", spy_fused), \
                mock.patch.object(torch, "randn", wraps=torch.randn) as randn:
            res = pipe.generate(PipelineRequest(**self.BASE, seeds=[5, 6]))
        assert res.images.shape == (2, 64, 64, 3)
        assert torch.isfinite(res.images.float()).all()
        assert "RNG: NV" in res.infotexts[0]
        # 3 steps, the last lands on sigma 0: two noisy steps, each one
        # fused launch at draws 1 and 2 from the cached device seed table
        assert adds == [True, True]
        assert launches == [(1, True), (2, True)]
        assert randn.call_count == 0

    def test_two_images_equal_two_single_runs(self, dev):
        """Exact, so with an elementwise stand-in for the UNet: library GEMM
        selection depends on the batch size, the noise must not."""
        from sdwd_amd.models import load_model
        from sdwd_amd.pipeline import PipelineRequest, StableDiffusionPipeline

        pipe = StableDiffusionPipeline(
            load_model("tiny", device=dev, dtype=torch.bfloat16, cache=False),
            device=dev,
        )

        def elementwise_unet(x, ts, ctx, y=None, control=None):
            return torch.tanh(x) * 0.5

        pipe.model.unet.forward = elementwise_unet

        def run(seeds):
            return pipe.generate(
                PipelineRequest(**self.BASE, seeds=seeds), decode=False
            ).images

        both = run([5, 2 ** 40 + 6])
        assert torch.isfinite(both.float()).all()
        assert torch.equal(both[:1], run([5]))
        assert torch.equal(both[1:], run([2 ** 40 + 6]))
        cpu = pipe.generate(
            PipelineRequest(**{**self.BASE, "randn_source": "CPU"},
                            seeds=[5, 2 ** 40 + 6]), decode=False,
        ).images
        assert not torch.equal(both, cpu)
