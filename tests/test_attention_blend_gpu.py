"""flash_blend_bf16_kernel (ops.attention_blend_bshd on the GPU) against the
fp64 reference and the derived bound of tests/attention_oracle.py.

Per context c an Oracle(q, K_c[:len_c], V_c[:len_c], scale) gives ref_c and
bound_c; the blend's reference and bound are

    ref = sum_c w_c ref_c,     bound = sum_c |w_c| bound_c(exact=True)

P is rounded to bf16 per context, the blend is fp32, and the single output
rounding 2^-9 |ref| <= 2^-9 sum |w_c| |ref_c| sits inside the per-context
2^-8 terms. exact=True: the kernel scales the fp32 scores after the MFMA, as
v2 does, so there is no extra Q rounding. Each case prints its worst
err/bound as "ATTN blend D=... ...".

All cases: B=2, H=2, [B,S,H,D] layout, K and V strided slices of one buffer
(as the fused K/V projection hands them over).
"""
import functools

import pytest
import torch

from sdwd_amd import ops

from attention_oracle import Oracle, default_scale, tail_inputs

pytestmark = pytest.mark.gpu

B, H, SQ = 2, 2, 260


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def plan(d):
    return tuple(ops.ext().attention_blend_plan(d))


def expected_plan(d):
    dpad = (d + 15) // 16 * 16
    return (dpad, 256 if dpad <= 32 else 128)


def fused_kv(k, v, dev):
    """k, v [Bk, Sk, H, D] CPU -> strided GPU views into one [Bk, Sk, 2HD]
    buffer."""
    bk, sk, h, d = k.shape
    kv = torch.cat([k.flatten(2), v.flatten(2)], dim=-1).to(dev)
    ks = kv[..., :h * d].unflatten(-1, (h, d))
    vs = kv[..., h * d:].unflatten(-1, (h, d))
    assert not ks.is_contiguous() and not vs.is_contiguous()
    return ks, vs


def run(q, k, v, w, index, lens, dev, scale=None, device_tables=False):
    ks, vs = fused_kv(k, v, dev)
    if device_tables:
        index = torch.tensor(index, dtype=torch.int32, device=dev)
        if lens is not None:
            lens = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = ops.attention_blend_bshd(q.to(dev), ks, vs, w.to(dev), index, lens,
                                   scale)
    assert out.shape == q.shape and out.dtype == q.dtype
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _oracle(tag, b, row, n, d):
    """Oracle of (q[b], K[row][:n], V[row][:n]) of the cached case `tag`."""
    q, k, v = _CASES[tag]
    return Oracle(q[b].transpose(0, 1), k[row, :n].transpose(0, 1),
                  v[row, :n].transpose(0, 1), default_scale(d))


_CASES = {}


def worst_ratio(tag, out, w, index, lens):
    """max |out - ref| / bound over the whole output of case `tag`; inf on
    a non-finite output or an error over a zero bound."""
    q, k, v = _CASES[tag]
    d = q.shape[-1]
    worst = 0.0
    for b in range(q.shape[0]):
        ref = torch.zeros(H, q.shape[1], d, dtype=torch.float64)
        bound = torch.zeros_like(ref)
        for c in range(w.shape[1]):
            row = index[b][c]
            n = k.shape[1] if lens is None else lens[row]
            wc = w[b if w.shape[0] > 1 else 0, c].double()[None, :, None]
            if not bool((wc != 0).any()):
                continue  # the bound of the call without this context
            orc = _oracle(tag, b, row, n, d)
            ref += wc * orc.ref
            bound += wc.abs() * orc.bound(exact=True)
        o = out[b].transpose(0, 1).double()
        if not torch.isfinite(o).all():
            return float("inf")
        err = (o - ref).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bound)
        worst = max(worst, r.max().item())
    return worst


def report(d, detail, worst):
    print(f"ATTN blend D={d} {detail} err/bound={worst:.3f}")


def period11_weights(c_n, sq=SQ):
    """w[c, s] = ((7s + 3c) mod 11) / 11: period 11 divides neither 32 nor
    64, so a wrong row in the weight broadcast shows."""
    s = torch.arange(sq)[None, :]
    c = torch.arange(c_n)[:, None]
    return (((7 * s + 3 * c) % 11).float() / 11.0)[None]


def sweep_case(d, sk=77, rows=6):
    """Random q, K; V of row r centred on 3 * (r mod 3), so taking the wrong
    context shows."""
    tag = ("sweep", d, sk, rows)
    if tag not in _CASES:
        g = torch.Generator().manual_seed(100 * d + sk)
        q = torch.randn(B, SQ, H, d, generator=g).bfloat16()
        k = torch.randn(rows, sk, H, d, generator=g).bfloat16()
        v = torch.randn(rows, sk, H, d, generator=g)
        v = (v + 3.0 * (torch.arange(rows) % 3)[:, None, None, None]).bfloat16()
        _CASES[tag] = (q, k, v)
    return tag


SWEEP_INDEX = [[0, 1, 2], [3, 4, 5]]


class TestHeadDimSweep:
    # DPAD 32/48/64/80/80/160: both QS choices (2 at DPAD 32, else 1), every
    # ND of 1..5 but 4, and D=72 with a masked 8-group inside the last chunk
    @pytest.mark.parametrize("d", [32, 40, 64, 72, 80, 160])
    def test_vs_fp64(self, dev, d):
        assert plan(d) == expected_plan(d)
        tag = sweep_case(d)
        q, k, v = _CASES[tag]
        w = period11_weights(3).expand(B, -1, -1).contiguous()
        out = run(q, k, v, w, SWEEP_INDEX, None, dev)
        worst = worst_ratio(tag, out, w, SWEEP_INDEX, None)
        report(d, "sweep Sq=260 Sk=77 C=3", worst)
        assert worst <= 1.0


class TestSelector:
    @pytest.mark.parametrize("d", [32, 40, 160])
    def test_one_hot_weights_pick_one_context(self, dev, d):
        tag = sweep_case(d)
        q, k, v = _CASES[tag]
        sel = torch.arange(SQ) % 3
        w = torch.zeros(1, 3, SQ)
        w[0, sel, torch.arange(SQ)] = 1.0
        out = run(q, k, v, w, SWEEP_INDEX, None, dev)
        # every row is held to the single-context bound of exactly its own
        # context: the other weights are 0 and add nothing to the bound
        worst = worst_ratio(tag, out, w, SWEEP_INDEX, None)
        report(d, "selector c=s%3", worst)
        assert worst <= 1.0


class TestStateReset:
    @pytest.mark.parametrize("d", [32, 40, 160])
    def test_large_offset_in_context_0_does_not_leak(self, dev, d):
        """Context 0 carries a uniform score offset of 8 * 64 * scale *
        log2(e) (about +100 log2 units) that cancels in its own softmax. A
        kernel that keeps m/l/o across contexts returns context 0's output
        for the other three."""
        tag = ("reset", d)
        sk, c_n = 154, 4
        if tag not in _CASES:
            g = torch.Generator().manual_seed(7 * d)
            q = torch.randn(B, SQ, H, d, generator=g)
            k = torch.randn(B * c_n, sk, H, d, generator=g)
            v = torch.randn(B * c_n, sk, H, d, generator=g)
            v = v + 3.0 * (torch.arange(B * c_n) % c_n)[:, None, None, None]
            q[..., 0] = 8.0
            k[..., 0] = 0.0
            k[0::c_n, :, :, 0] = 64.0
            _CASES[tag] = (q.bfloat16(), k.bfloat16(), v.bfloat16())
        q, k, v = _CASES[tag]
        assert 8 * 64 * default_scale(d) * 1.4426950408889634 > 50
        index = [[b * c_n + c for c in range(c_n)] for b in range(B)]
        w = period11_weights(c_n) + 0.25
        out = run(q, k, v, w, index, None, dev)
        worst = worst_ratio(tag, out, w, index, None)
        report(d, "reset Sk=154 C=4", worst)
        assert worst <= 1.0


class TestPerContextLengths:
    @pytest.mark.parametrize("d", [32, 40, 80, 160])
    def test_no_keys_past_each_length(self, dev, d):
        """Every real score strongly negative (tail_inputs): a key admitted
        past its row's length with score 0, or a NaN, would dominate."""
        tag = ("lens", d)
        sk, lens = 154, [77, 154, 100]
        if tag not in _CASES:
            qs, ks, vs = [], [], []
            for i in range(3):
                qi, ki, vi = tail_inputs(SQ, sk, d, h=H, seed=i)
                qs.append(qi.transpose(0, 1))
                ks.append(ki.transpose(0, 1))
                vs.append((vi + 3.0 * i).bfloat16().transpose(0, 1))
            _CASES[tag] = (torch.stack(qs[:B]), torch.stack(ks),
                           torch.stack(vs))
        q, k, v = _CASES[tag]
        kn, vn = k.clone(), v.clone()
        for row, n in enumerate(lens):
            kn[row, n:] = float("nan")
            vn[row, n:] = float("nan")
        index = [[0, 1, 2], [2, 0, 1]]
        w = period11_weights(3)
        for device_tables in (False, True):
            out = run(q, kn, vn, w, index, lens, dev,
                      device_tables=device_tables)
            assert torch.isfinite(out.float()).all()
            worst = worst_ratio(tag, out, w, index, lens)
            report(d, f"lens {lens} device_tables={device_tables}", worst)
            assert worst <= 1.0


class TestIndexTable:
    @pytest.mark.parametrize("d", [40, 160])
    @pytest.mark.parametrize("index", [[[0, 2, 3], [1, 2, 3]],
                                       [[3, 0, 2], [2, 3, 1]]],
                             ids=["shared", "permuted"])
    def test_shared_and_permuted_rows(self, dev, d, index):
        tag = sweep_case(d, rows=4)
        q, k, v = _CASES[tag]
        w1 = period11_weights(3)
        wb = torch.cat([w1, w1.flip(1)], dim=0).contiguous()
        for name, w in (("w[1,C,Sq]", w1), ("w[B,C,Sq]", wb)):
            out = run(q, k, v, w, index, None, dev)
            worst = worst_ratio(tag, out, w, index, None)
            report(d, f"index {index} {name}", worst)
            assert worst <= 1.0


class TestSignedAndZeroWeights:
    @pytest.mark.parametrize("d", [40, 160])
    def test_negative_weights(self, dev, d):
        tag = sweep_case(d)
        q, k, v = _CASES[tag]
        w = (period11_weights(3) - 0.5) * 2.0
        assert (w < 0).any() and (w > 0).any()
        out = run(q, k, v, w, SWEEP_INDEX, None, dev)
        worst = worst_ratio(tag, out, w, SWEEP_INDEX, None)
        report(d, "signed w", worst)
        assert worst <= 1.0

    @pytest.mark.parametrize("d", [40, 160])
    def test_zero_weight_context_adds_nothing(self, dev, d):
        tag = sweep_case(d)
        q, k, v = _CASES[tag]
        w = period11_weights(3).clone()
        w[:, 1] = 0.0
        out = run(q, k, v, w, SWEEP_INDEX, None, dev)
        # worst_ratio leaves an all-zero context out of ref and bound: the
        # bound of the call without it
        worst = worst_ratio(tag, out, w, SWEEP_INDEX, None)
        report(d, "w_1 == 0", worst)
        assert worst <= 1.0


class TestSingleContext:
    @pytest.mark.parametrize("d", [32, 40, 160])
    def test_c1_unit_weight_is_plain_attention(self, dev, d):
        tag = sweep_case(d)
        q, k, v = _CASES[tag]
        w = torch.ones(1, 1, SQ)
        index = [[0], [3]]
        out = run(q, k, v, w, index, None, dev)
        worst = worst_ratio(tag, out, w, index, None)
        report(d, "C=1 w=1", worst)
        assert worst <= 1.0

    @pytest.mark.parametrize("sk", [77, 150])
    @pytest.mark.parametrize("d", [40, 80, 160])
    def test_c1_unit_weight_is_v2_bit_for_bit(self, dev, d, sk):
        """The blend and v2 run the same tile step, so one context of unit
        weight is v2's sequence: w / l with w = 1 is 1 / l, 0 + o * f rounds
        as o * f, and the per-row math does not depend on QS. Sq=70 crosses
        a 32-row subtile inside a ragged block; Sk=77 is one ragged tile
        after a full one, Sk=150 a multi-tile ragged walk."""
        sq = 70
        g = torch.Generator().manual_seed(1000 * d + sk)
        q = torch.randn(B, sq, H, d, generator=g).bfloat16().to(dev)
        k = torch.randn(B, sk, H, d, generator=g).bfloat16().to(dev)
        v = torch.randn(B, sk, H, d, generator=g).bfloat16().to(dev)
        w = torch.ones(1, 1, sq, device=dev)
        blend = ops.attention_blend_bshd(q, k, v, w, [[0], [1]], None)
        plain = ops.attention_bshd(q, k, v, variant="v2")
        assert torch.isfinite(plain.float()).all()
        assert torch.equal(blend, plain)


class TestErrors:
    def _args(self, dev, d, dtype):
        q = torch.randn(B, 64, H, d, device=dev, dtype=dtype)
        k = torch.randn(B, 77, H, d, device=dev, dtype=dtype)
        w = torch.ones(1, 1, 64, device=dev)
        return q, k, k, w, [[0], [1]]

    def test_fp16_raises(self, dev):
        with pytest.raises(RuntimeError):
            ops.attention_blend_bshd(*self._args(dev, 40, torch.float16))

    def test_unsupported_head_dim_raises(self, dev):
        args = self._args(dev, 512, torch.bfloat16)
        assert not ops.attention_blend_supported(*args[:3])
        with pytest.raises(RuntimeError):
            ops.attention_blend_bshd(*args)
        with pytest.raises(RuntimeError):
            ops.ext().attention_blend_plan(512)

    def test_supported_predicate(self, dev):
        q, k, v, _, _ = self._args(dev, 40, torch.bfloat16)
        assert ops.attention_blend_supported(q, k, v)
        assert not ops.attention_blend_supported(q.half(), k.half(), v.half())
        assert not ops.attention_blend_supported(q.cpu(), k.cpu(), v.cpu())
