"""CPU tests of the Philox4x32-10 + Box-Muller ops (the "NV" random source):
the core against the Random123 known answers, the stream against the
independent numpy reference of tests/philox_oracle.py.

Normals are compared element by element within the bound derived in
philox_oracle's docstring,

    |r_hat - r| <= 2^-24 (K1 / s + K2 s + K3 |r|),   s = sqrt(-2 ln u),

with the CPU ulp figures (K2 = 1 + 2*0.5 + 25.5 + 2*3.5 = 34.5). Elements
with u >= 1 - 2^-20 are left out of that comparison alone (never out of the
word comparison); the seeds are fixed and the reference itself shows at most
4 such elements per 2^20.
"""
import math

import numpy as np
import pytest
import torch

from philox_oracle import (KNOWN, OFFSETS, SEEDS, ULP_CPU, Draw,
                           counters_keys, draw_words)
from sdwd_amd import ops


def check_normals(got, draw, ulp, scale=1.0, extra=0.0, what=""):
    """got [n] against the reference draw; returns the worst err/bound."""
    got = got.detach().cpu().double().numpy()
    assert np.isfinite(got).all(), what
    err = np.abs(got - draw.r)
    bound = scale * draw.bound(ulp) + extra
    ratio = np.where(draw.keep, err / bound, 0.0)
    worst = float(ratio.max())
    print(f"{what}: worst err/bound {worst:.3f}, "
          f"left out {int((~draw.keep).sum())} of {got.size}")
    assert worst <= 1.0, what
    return worst


def test_known_answers():
    c = torch.tensor([k[0] for k in KNOWN], dtype=torch.int64)
    k = torch.tensor([k[1] for k in KNOWN], dtype=torch.int64)
    want = torch.tensor([k[2] for k in KNOWN], dtype=torch.int64)
    assert torch.equal(ops.philox4x32(c, k), want)


@pytest.mark.parametrize("offset", OFFSETS)
def test_words_bit_exact(offset):
    """The raw words of every draw the normals tests use, through the op's
    own core, equal the numpy rounds bit for bit."""
    n = 4099
    for seed in SEEDS:
        c, k = counters_keys(seed, offset, n)
        got = ops.philox4x32(torch.from_numpy(c), torch.from_numpy(k))
        x0, x1 = draw_words(seed, offset, n)
        assert torch.equal(got[:, 0], torch.from_numpy(x0.astype(np.int64)))
        assert torch.equal(got[:, 1], torch.from_numpy(x1.astype(np.int64)))


def test_normals_within_bound_2pow20():
    """2^20 normals (4 seeds x 2^18) at offset 0 against the fp64 reference;
    at most 4 elements per 2^20 may sit in the excluded u >= 1 - 2^-20."""
    n = 1 << 18
    got = ops.philox_randn(SEEDS, 0, (n,))
    assert got.shape == (len(SEEDS), n) and got.dtype == torch.float32
    left_out = 0
    for i, seed in enumerate(SEEDS):
        d = Draw(seed, 0, n)
        left_out += int((~d.keep).sum())
        check_normals(got[i], d, ULP_CPU, what=f"seed {seed}")
    assert left_out <= 4


@pytest.mark.parametrize("offset", OFFSETS[1:])
def test_normals_high_offsets(offset):
    shape = (3, 37, 37)  # n = 4107, odd
    n = math.prod(shape)
    got = ops.philox_randn(torch.tensor(SEEDS), offset, shape)
    assert got.shape == (len(SEEDS), *shape)
    for i, seed in enumerate(SEEDS):
        d = Draw(seed, offset, n)
        assert int((~d.keep).sum()) == 0
        check_normals(got[i].reshape(-1), d, ULP_CPU,
                      what=f"seed {seed} offset {offset}")


def test_offset_advances_by_one():
    """Consecutive draws are offsets k, k+1: different from each other, and
    draw k+1 is exactly what asking for offset k+1 gives."""
    from sdwd_amd.pipeline.noise import PhiloxNoise

    src = PhiloxNoise([5, 6], [-1, -1], 0.0, 0, "cpu", torch.float32)
    src.shape = (4, 3, 3)
    first = src.initial((4, 3, 3))
    a, b = src(), src()
    for k, t in enumerate((first, a, b)):
        assert torch.equal(t, ops.philox_randn([5, 6], k, (4, 3, 3))), k
    assert not torch.equal(a, b)


def test_bf16_is_rounded_fp32():
    a = ops.philox_randn([3], 2, (1000,))
    b = ops.philox_randn([3], 2, (1000,), dtype=torch.bfloat16)
    assert b.dtype == torch.bfloat16 and torch.equal(a.to(torch.bfloat16), b)


@pytest.mark.parametrize("bad", [[-1], [1 << 64], [1.5], [True]])
def test_bad_seed_names_argument(bad):
    with pytest.raises(ValueError, match="seeds"):
        ops.philox_randn(bad, 0, (4,))


def test_bad_offset_and_dtype():
    with pytest.raises(ValueError, match="offset"):
        ops.philox_randn([1], -1, (4,))
    with pytest.raises(ValueError, match="offset"):
        ops.philox_randn([1], 1 << 64, (4,))
    with pytest.raises(ValueError, match="dtype"):
        ops.philox_randn([1], 0, (4,), dtype=torch.float16)


def test_largest_seed_and_offset():
    r = ops.philox_randn([(1 << 64) - 1], (1 << 64) - 1, (64,))
    d = Draw((1 << 64) - 1, (1 << 64) - 1, 64)
    check_normals(r[0], d, ULP_CPU, what="max seed/offset")


class TestAddPhiloxNoise:
    B, CHW = 3, (4, 5, 7)
    seeds = [11, 2 ** 32 + 7, 2 ** 63 - 1]

    def _x(self, dtype=torch.float32):
        g = torch.Generator().manual_seed(0)
        return torch.randn(self.B, *self.CHW, generator=g).to(dtype)

    def test_equals_axpby_of_randn(self):
        x = self._x()
        got = ops.add_philox_noise(x, self.seeds, 3, 0.75, 0.37)
        want = 0.75 * x + 0.37 * ops.philox_randn(self.seeds, 3, self.CHW)
        assert torch.equal(got, want)

    def test_channels_last_same_logical_result(self):
        x = self._x()
        xc = x.contiguous(memory_format=torch.channels_last)
        a = ops.add_philox_noise(x, self.seeds, 3, 1.0, 0.37)
        b = ops.add_philox_noise(xc, self.seeds, 3, 1.0, 0.37)
        assert a.is_contiguous()
        assert b.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(a, b)

    def test_other_layout_made_contiguous(self):
        x = self._x()
        xt = x.permute(0, 1, 3, 2)  # neither contiguous nor channels_last
        got = ops.add_philox_noise(xt, self.seeds, 3, 1.0, 0.37)
        want = ops.add_philox_noise(xt.contiguous(), self.seeds, 3, 1.0, 0.37)
        assert got.is_contiguous() and torch.equal(got, want)

    def test_bf16_rounds_once(self):
        x = self._x(torch.bfloat16)
        got = ops.add_philox_noise(x, self.seeds, 3, 1.0, 0.37)
        want = (x.float() + 0.37 * ops.philox_randn(self.seeds, 3, self.CHW))
        assert got.dtype == torch.bfloat16
        assert torch.equal(got, want.to(torch.bfloat16))

    def test_rejects_bad_input(self):
        with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
            ops.add_philox_noise(torch.zeros(3, 4, 5), self.seeds, 0, 1, 1)
        with pytest.raises(ValueError, match="seeds"):
            ops.add_philox_noise(self._x(), [1, 2], 0, 1, 1)


def test_distribution_sanity():
    n = 1 << 20
    r = ops.philox_randn([2024], 0, (n,))[0].double()
    assert torch.isfinite(r).all()
    assert abs(float(r.mean())) < 5.0 / math.sqrt(n)
    assert abs(float(r.var()) - 1.0) < 5.0 * math.sqrt(2.0 / n)
    assert float(r.abs().max()) < math.sqrt(66.0 * math.log(2.0))
