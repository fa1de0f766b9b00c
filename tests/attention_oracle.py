"""fp64 attention reference, a derived per-element error bound, and the
structured inputs of tests/test_attention_gpu.py.

Plain helper module (not a conftest): the CPU tests in
tests/test_attention_oracle.py prove that the bound rejects wrong results
and that the inputs do what they claim; the GPU tests apply both to the
flash kernels of sdwd_amd/ops/hip/attention.hip.

Reference, from the bf16 inputs in fp64, with c = scale * log2(e):

    s_ij = c * sum_d q_id k_jd,   p = softmax_2(s),   ref = p @ v

Bound, on every output element:

    |out_id - ref_id| <= (2^-7 + delta_i) * sum_j p_ij |v_jd| + 2^-8 |ref_id|

Derivation. P is rounded to bf16 before the PV MFMA, which moves the
numerator by at most 2^-9 * sum p|v| (l is summed from the unrounded fp32
P). The output is rounded to bf16: at most 2^-9 * |ref|. The constants are
4x and 2x those; the slack covers fp32 accumulation order, v_exp_f32 and
second-order terms.

delta_i is 0 when the kernel's Q pre-scale is exact: always for v2 (it
scales fp32 scores after the MFMA), and for v3 when c is a power of two
(exact_scale()). Otherwise v3 rounds q * scale * log2(e) to bf16 once more,
which moves each score by at most 2^-9 * c * sum_d |q_id k_jd| log2 units,
every p_ij by at most a factor 2^(+-2 * that) after normalisation, hence

    delta_i = 2 ln2 * 2^-9 * max_j c * sum_d |q_id k_jd|.
"""
import math

import torch

LOG2E = 1.4426950408889634
KVB = 64     # mirrors attention.hip: keys per staged tile (v2 and v3)
THR = 8.0    # mirrors flash_fwd_bf16_v3: defer-max threshold, log2 units
WROWS = 32   # mirrors both kernels: q rows that share one wave's decisions


def exact_scale(k):
    """A scale whose c = scale * log2(e) is 2^-k: the kernel's fp32 product
    is within 1 ulp of 2^-k, so bf16(q * l2scale) is exactly q * 2^-k."""
    return 2.0 ** -k / LOG2E


def default_scale(d):
    return 1.0 / math.sqrt(d)


class Oracle:
    """ref, sum p|v| and delta for q [.., Sq, D], k/v [.., Sk, D] (bf16 or
    anything exactly representable in fp64); leading dims are batch."""

    def __init__(self, q, k, v, scale):
        q = q.detach().cpu().double()
        k = k.detach().cpu().double()
        v = v.detach().cpu().double()
        c = scale * LOG2E
        self.s = c * (q @ k.transpose(-1, -2))          # log2 units
        w = torch.exp2(self.s - self.s.amax(-1, keepdim=True))
        self.p = w / w.sum(-1, keepdim=True)
        self.ref = self.p @ v
        self.pav = self.p @ v.abs()
        sabs = abs(c) * (q.abs() @ k.abs().transpose(-1, -2))
        self.delta = 2 * math.log(2) * 2.0 ** -9 * sabs.amax(-1, keepdim=True)
        # the composed path stores q.k in bf16: |s| itself, not sum |qk|
        self.delta_composed = (
            2 * math.log(2) * 2.0 ** -9 * self.s.abs().amax(-1, keepdim=True)
        )

    def bound(self, exact=False, composed=False):
        d = 0.0 if exact else (self.delta_composed if composed else self.delta)
        return (2.0 ** -7 + d) * self.pav + 2.0 ** -8 * self.ref.abs()

    def ratio(self, out, exact=False, composed=False):
        """|out - ref| / bound per element (inf where a non-finite output
        or an error over a zero bound appears)."""
        out = out.detach().cpu().double()
        err = (out - self.ref).abs()
        b = self.bound(exact, composed)
        r = torch.where(err == 0, torch.zeros_like(err), err / b)
        return torch.where(torch.isfinite(out), r,
                           torch.full_like(r, float("inf")))

    def worst(self, out, exact=False, composed=False):
        return self.ratio(out, exact, composed).max().item()


# ---------------------------------------------------------------------------
# tile walk: the rescale decisions flash_fwd_bf16_v3 takes on given scores
# ---------------------------------------------------------------------------
def tile_walk(s):
    """s: [Sq, Sk] scores in log2 units. Mirrors the v3 kernel's defer-max
    control flow: KVB-key tiles, a wave of WROWS consecutive q rows rescales
    when ANY of its rows' tile max exceeds the running max by more than THR,
    and then every row of the wave takes m = max(m, tile max) with
    alpha = 2^(m_old - m_new) (so rows whose max did not grow get alpha == 1).

    Returns dict: triggers (wave-tiles that rescale after tile 0),
    mixed (of those, waves holding both alpha < 1 and alpha == 1 rows),
    per_tile (triggers per tile index, tile 0 excluded -> entry 0 is 0),
    deferred (largest growth, in log2 units, that was NOT rescaled)."""
    s = s.detach().cpu().double()
    Sq, Sk = s.shape
    nw = (Sq + WROWS - 1) // WROWS
    m = torch.full((Sq,), -1e30, dtype=torch.float64)
    ntile = (Sk + KVB - 1) // KVB
    per_tile = [0] * ntile
    triggers = mixed = 0
    deferred = 0.0
    for t in range(ntile):
        pmax = s[:, t * KVB:(t + 1) * KVB].amax(-1)
        grow = pmax > m + THR
        for w in range(nw):
            rows = slice(w * WROWS, min(Sq, (w + 1) * WROWS))
            if bool(grow[rows].any()):
                mnew = torch.maximum(m[rows], pmax[rows])
                if t > 0:
                    triggers += 1
                    per_tile[t] += 1
                    lt = mnew > m[rows]
                    if bool(lt.any()) and bool((~lt).any()):
                        mixed += 1
                m[rows] = mnew
            elif t > 0:
                deferred = max(deferred, (pmax[rows] - m[rows]).max().item())
    return {"triggers": triggers, "mixed": mixed, "per_tile": per_tile,
            "deferred": deferred}


def emulate_v3(q, k, v, scale, alpha="ok"):
    """CPU model of flash_fwd_bf16_v3's arithmetic for one head: q [Sq, D],
    k/v [Sk, D] bf16. Q pre-scaled and rounded to bf16, fp32 scores,
    deferred max per 32-row wave, P rounded to bf16 for PV, l from unrounded
    P, bf16 output. alpha selects the factor applied to the O accumulator:
    "ok" the row's own, "neighbour" the next row's (a wrong broadcast row
    map), "none" no rescale at all. l always takes the row's own alpha, as
    in the kernel, where only the O rescale goes through the lane
    broadcast."""
    q, k, v = q.cpu(), k.cpu(), v.cpu()
    l2 = (torch.tensor(scale, dtype=torch.float32)
          * torch.tensor(LOG2E, dtype=torch.float32))
    qs = (q.float() * l2).bfloat16().float()
    kf, vf = k.float(), v.float()
    Sq, Sk = q.shape[0], k.shape[0]
    m = torch.full((Sq,), -1e30)
    l = torch.zeros(Sq)
    o = torch.zeros(Sq, v.shape[1])
    wave = torch.arange(Sq) // WROWS
    nw = (Sq + WROWS - 1) // WROWS
    for t in range(0, Sk, KVB):
        s = qs @ kf[t:t + KVB].T
        pmax = s.amax(-1)
        grow = torch.zeros(nw * WROWS, dtype=torch.bool)
        grow[:Sq] = pmax > m + THR
        trig = grow.view(nw, WROWS).any(-1)[wave]
        mnew = torch.where(trig, torch.maximum(m, pmax), m)
        a = torch.exp2(m - mnew)
        l = l * a
        if alpha == "neighbour":
            ao = torch.roll(a, -1)
        elif alpha == "none":
            ao = torch.ones_like(a)
        else:
            ao = a
        o = o * ao[:, None]
        m = mnew
        p = torch.exp2(s - m[:, None])
        l = l + p.sum(-1)
        o = o + p.bfloat16().float() @ vf[t:t + KVB]
    return (o / l.clamp_min(1e-30)[:, None]).bfloat16()


# ---------------------------------------------------------------------------
# structured inputs (all [H, S, D] bf16 on CPU; the GPU tests add the batch)
# ---------------------------------------------------------------------------
RESCALE_CK = 3  # the rescale family runs with c = 2^-3
RESCALE_KINDS = ("ramp", "creep", "decreasing", "lastkey")


def rescale_inputs(kind, d, sq=260, sk=280, h=2, seed=0):
    """Head dim 0 carries a designed score c*q_i0*k_j0 = a_i * g(j) on top
    of small random scores from the other dims; V is scaled per key so that
    old and new tiles both carry weight in the output.

    ramp:       a cycles {12, 10, 0, -10} by row, g = tile index, V * 2^(-11
                tile): a=12/10 rows rescale at every tile, a=-10 rows need
                alpha == 1 in the same wave.
    creep:      a cycles {6, 5.5, 0, -6}: ~6 log2 units per tile, so the
                rescale fires every other tile and P rises towards 2^8.
    decreasing: a cycles {12, 10, 0, 3}, g = -tile, V * 2^(+11 tile): the max
                sits in tile 0 and nothing rescales afterwards.
    lastkey:    a cycles {12, 10, 0, -10}, g = 4 on the last key of the
                ragged tile only, that key's V * 2^-44.
    Returns q, k, v and the exact scale."""
    g = torch.Generator().manual_seed(seed + d)
    c = 2.0 ** -RESCALE_CK
    q = torch.randn(h, sq, d, generator=g) * 0.5
    k = torch.randn(h, sk, d, generator=g) * 0.5
    v = torch.randn(h, sk, d, generator=g)
    tile = (torch.arange(sk) // KVB).double()
    cyc = {"ramp": (12.0, 10.0, 0.0, -10.0), "creep": (6.0, 5.5, 0.0, -6.0),
           "decreasing": (12.0, 10.0, 0.0, 3.0),
           "lastkey": (12.0, 10.0, 0.0, -10.0)}[kind]
    a = torch.tensor(cyc, dtype=torch.float64)[torch.arange(sq) % 4]
    if kind == "ramp":
        gk, vlog = tile, -11.0 * tile
    elif kind == "creep":
        gk, vlog = tile, -5.0 * tile
    elif kind == "decreasing":
        gk, vlog = -tile, 11.0 * tile
    else:
        gk = torch.zeros(sk, dtype=torch.float64)
        gk[-1] = 4.0
        vlog = torch.zeros(sk, dtype=torch.float64)
        vlog[-1] = -44.0
    q[:, :, 0] = (a / c).float()
    k[:, :, 0] = gk.float()
    v = v * torch.exp2(vlog).float()[None, :, None]
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    # the designed column must have survived the bf16 rounding exactly
    assert torch.equal(q[0, :, 0].double(), a / c)
    assert torch.equal(k[0, :, 0].double(), gk)
    return q, k, v, exact_scale(RESCALE_CK)


def tail_inputs(sq, sk, d, h=2, seed=0):
    """Every real score strongly negative, V centred on 3: a key admitted
    past Sk with score 0 would take most of the softmax mass."""
    g = torch.Generator().manual_seed(seed + 1000 * sq + sk + d)
    q = (torch.randn(h, sq, d, generator=g).abs() * 1.5).bfloat16()
    k = (-torch.randn(h, sk, d, generator=g).abs()).bfloat16()
    v = (torch.randn(h, sk, d, generator=g) + 3).bfloat16()
    return q, k, v


def retrieval_inputs(d, sq=260, sk=280, h=2, beta=64.0, seed=0):
    """Keys are distinct +-1 codes, query i is beta * key pi(i): with the
    default scale the matched score beats every other by c*beta*2*hamming
    log2 units, so the output is v[pi(i)] bit for bit. Returns q, k, v, pi
    ([h, sq] key indices)."""
    g = torch.Generator().manual_seed(seed + d)
    while True:
        k = torch.randint(0, 2, (h, sk, d), generator=g).float() * 2 - 1
        gram = k @ k.transpose(-1, -2)
        gram.diagonal(dim1=-2, dim2=-1).fill_(-d)
        if gram.max() < d:  # no two keys of a head are equal
            break
    pi = torch.randint(0, sk, (h, sq), generator=g)
    q = beta * torch.gather(k, 1, pi[:, :, None].expand(h, sq, d))
    v = torch.randn(h, sk, d, generator=g)
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), pi
