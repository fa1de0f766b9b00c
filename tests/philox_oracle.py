"""Independent reference for the Philox4x32-10 + Box-Muller stream ("NV"
random source) and the derived per-element error bound of its fp32
implementations. Plain helper module (not a conftest) shared by
tests/test_philox_cpu.py and tests/test_philox_gpu.py; nothing here imports
the stream from the package.

Stream (docs/usage.md), element j of draw `offset` of generator `seed`:

    counter (offset & M32, offset >> 32, j, 0), key (seed & M32, seed >> 32)
    (x0, x1, _, _) = philox4x32_10(counter, key)
    u = x0 * 2^-32 + 2^-33,  v = 2 pi u'  with u' = x1 * 2^-32 + 2^-33
    r = s * sin(v),  s = sqrt(-2 ln u)

The reference does the rounds in uint64 numpy arithmetic and Box-Muller in
fp64 from the exact words, so its own error (~1e-16) is far below the bound.

Bound. An fp32 implementation computes, with eps = 2^-24 (unit roundoff):

* u_hat: the uint32 -> float conversion and the add each round once, so
  |u_hat - u| <= 2 eps u (1 + eps). With L = -2 ln u = s^2 this moves L by
  |dL| <= 4 eps, and s by |dL| / (s + s') where s' >= s sqrt(1 - 4 eps / L).
  On the elements compared, u < 1 - 2^-20, so L > 2^-19, 4 eps / L < 2^-3
  and |ds| <= 4 eps / ((1 + sqrt(7/8)) s) < 2.07 eps / s. This 1/s term is
  real: near u = 1 one ulp of u moves r by far more than an ulp. K1 = 2.25.
* logf within E_log ulp (1 ulp <= 2 eps relative) and sqrtf within E_sqrt
  ulp: s_hat = sqrtf(-2 logf(u_hat)) carries another (E_log + 2 E_sqrt) eps
  relative error (the square root halves the logarithm's).
* v_hat: conversion, the rounded constant 2 pi 2^-32, the product and the
  add each contribute at most eps v, v <= 2 pi: |v_hat - v| <= 4 eps 2 pi
  < 25.2 eps, and sin is 1-Lipschitz. sinf within E_sin ulp adds
  2 E_sin eps (|sin| <= 1).
  So |sin_hat - sin v| <= (25.5 + 2 E_sin) eps, multiplied by s.
* the final product rounds once: eps |r|; K3 = 2 leaves the same again for
  the second-order cross terms of everything above.

    |r_hat - r| <= K1 eps / s + (E_log + 2 E_sqrt + 25.5 + 2 E_sin) eps s
                   + K3 eps |r|

Elements with u >= 1 - 2^-20 (about 2^-20 of all draws) are left out of the
normals comparison only: there u_hat may round to exactly 1, s_hat = 0, and
the linearisation above does not hold. Their words are still compared.

ulp figures. CPU (the package's torch path): ATen's vectorised fp32 kernels
call SLEEF's logf at 1.0 ulp and sinf at 3.5 ulp; sqrt is correctly rounded.
Device: the OpenCL C specification's relative-error table (log 3, sin 4,
sqrt 3 ulp), which the ROCm device library the kernel's logf/sinf/sqrtf come
from is written to meet.
"""
import math

import numpy as np

EPS = 2.0 ** -24
M32 = 0xFFFFFFFF
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85

K1 = 2.25
K3 = 2.0
ULP_CPU = dict(log=1.0, sin=3.5, sqrt=0.5)
ULP_DEVICE = dict(log=3.0, sin=4.0, sqrt=3.0)

# the cases the issue fixes: high key word, high counter word
SEEDS = [0, 1, 2 ** 32 + 7, 2 ** 63 - 1]
OFFSETS = [0, 1, 2 ** 32 + 5]
U_CUT = 1.0 - 2.0 ** -20

# Random123 known answers: (counter, key, output)
KNOWN = [
    ([0, 0, 0, 0], [0, 0],
     [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2,
     [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344],
     [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def philox_words_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold uint32 values."""
    c0, c1, c2, c3, k0, k1 = (
        np.asarray(a, dtype=np.uint64) for a in (c0, c1, c2, c3, k0, k1)
    )
    mask, sh = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0   # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (
            (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        )
        k0 = (k0 + np.uint64(W0)) & mask
        k1 = (k1 + np.uint64(W1)) & mask
    return c0, c1, c2, c3


def draw_words(seed, offset, n):
    """(x0, x1) uint64 [n] of draw `offset` of generator `seed`."""
    j = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, dtype=np.uint64)
    x0, x1, _, _ = philox_words_np(
        z + np.uint64(offset & M32), z + np.uint64(offset >> 32), j, z,
        z + np.uint64(seed & M32), z + np.uint64(seed >> 32),
    )
    return x0, x1


def counters_keys(seed, offset, n):
    """int64-valued [n,4] / [n,2] tables of the same draw for
    ops.philox4x32."""
    c = np.zeros((n, 4), dtype=np.int64)
    c[:, 0] = offset & M32
    c[:, 1] = offset >> 32
    c[:, 2] = np.arange(n)
    k = np.zeros((n, 2), dtype=np.int64)
    k[:, 0] = seed & M32
    k[:, 1] = seed >> 32
    return c, k


class Draw:
    """fp64 reference normals of one draw, and what the bound needs."""

    def __init__(self, seed, offset, n):
        self.x0, self.x1 = draw_words(seed, offset, n)
        self.u = self.x0.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33
        v = 2.0 * math.pi * (
            self.x1.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33
        )
        self.s = np.sqrt(-2.0 * np.log(self.u))
        self.r = self.s * np.sin(v)
        self.keep = self.u < U_CUT

    def bound(self, ulp):
        k2 = ulp["log"] + 2.0 * ulp["sqrt"] + 25.5 + 2.0 * ulp["sin"]
        s = np.where(self.keep, self.s, 1.0)
        return EPS * (K1 / s + k2 * s + K3 * np.abs(self.r))
