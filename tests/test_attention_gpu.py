"""Flash attention kernels (v2, v3) and the composed path against the fp64
reference and the derived per-element bound of tests/attention_oracle.py.

Every case names the kernel it is meant to reach and asserts it with
ext().attention_plan, the function the launcher itself decides by. Each
case prints its worst err/bound as "ATTN <family> <kernel> ...".
"""
import functools

import pytest
import torch

from sdwd_amd import ops

from attention_oracle import (Oracle, RESCALE_KINDS, default_scale,
                              rescale_inputs, retrieval_inputs, tail_inputs,
                              tile_walk)

pytestmark = pytest.mark.gpu

FORCE = {"auto": 0, "v2": 2, "v3": 3}
LAYOUTS = ("bhsd", "bshd")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def plan(d, sk, variant="auto"):
    return tuple(ops.ext().attention_plan(d, sk, FORCE[variant]))


def run(q, k, v, layout, dev, scale=None, variant=None):
    """q/k/v: [H, S, D] or [B, H, S, D] CPU tensors. Runs the named entry
    layout on contiguous GPU copies; returns [B, H, Sq, D] on the CPU."""
    if q.dim() == 3:
        q, k, v = q[None], k[None], v[None]
    q, k, v = (t.to(dev) for t in (q, k, v))
    if layout == "bhsd":
        out = ops.attention(q, k, v, scale, variant)
    else:
        q, k, v = (t.transpose(1, 2).contiguous() for t in (q, k, v))
        out = ops.attention_bshd(q, k, v, scale, variant).transpose(1, 2)
    return out.cpu()


def report(family, kernel, d, detail, worst):
    print(f"ATTN {family} {kernel} D={d} {detail} err/bound={worst:.3f}")


# ---------------------------------------------------------------------------
# a. head-dim sweep: every padded instantiation of both kernels
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep_case(d, sk):
    g = torch.Generator().manual_seed(100 * d + sk)
    q = torch.randn(2, 260, d, generator=g).bfloat16()
    k = torch.randn(2, sk, d, generator=g).bfloat16()
    v = torch.randn(2, sk, d, generator=g).bfloat16()
    return q, k, v, Oracle(q, k, v, default_scale(d))


class TestHeadDimSweep:
    @pytest.mark.parametrize("layout", LAYOUTS)
    @pytest.mark.parametrize("sk,variant", [(150, "v2"), (150, "v3"),
                                            (280, "auto")])
    @pytest.mark.parametrize("d", range(24, 193, 8))
    def test_vs_fp64(self, dev, d, sk, variant, layout):
        dpad = (d + 15) // 16 * 16
        kernel = "v3" if variant == "auto" else variant
        rows = 256 if kernel == "v2" or dpad <= 96 else 128
        assert plan(d, sk, variant) == (kernel, dpad, rows)
        q, k, v, orc = _sweep_case(d, sk)
        out = run(q, k, v, layout, dev, variant=variant)
        worst = orc.worst(out[0], exact=(kernel == "v2"))
        report("sweep", kernel, d, f"Sk={sk} {layout}", worst)
        assert worst <= 1.0


# ---------------------------------------------------------------------------
# b. rescale family: the running max moves by design
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rescale_case(kind, d):
    q, k, v, sc = rescale_inputs(kind, d)
    orc = Oracle(q, k, v, sc)
    walks = [tile_walk(orc.s[h]) for h in range(q.shape[0])]
    return q, k, v, sc, orc, walks


class TestRescale:
    @pytest.mark.parametrize("variant", ["v2", "v3"])
    @pytest.mark.parametrize("d", [40, 64, 80, 160])
    @pytest.mark.parametrize("kind", RESCALE_KINDS)
    def test_designed_max_walk(self, dev, kind, d, variant):
        q, k, v, sc, orc, walks = _rescale_case(kind, d)
        # the input does what it claims, before the kernel is looked at
        for w in walks:
            if kind == "ramp":
                assert all(n >= 1 for n in w["per_tile"][1:]), w
                assert w["mixed"] >= 1, w
            elif kind == "creep":
                assert w["triggers"] >= 1 and w["deferred"] > 4.0, w
            elif kind == "decreasing":
                assert w["triggers"] == 0, w
            else:
                assert w["per_tile"][-1] >= 1, w
                assert sum(w["per_tile"][:-1]) == 0 and w["mixed"] >= 1, w
        assert plan(d, k.shape[1], variant)[0] == variant
        # c is a power of two: v3's Q pre-scale is exact, delta = 0
        out = run(q, k, v, "bhsd", dev, scale=sc, variant=variant)
        worst = orc.worst(out[0], exact=True)
        trig = sum(w["triggers"] for w in walks)
        mixed = sum(w["mixed"] for w in walks)
        report("rescale", variant, d,
               f"{kind} triggers={trig} mixed={mixed}", worst)
        assert worst <= 1.0


# ---------------------------------------------------------------------------
# c. tails: ragged Sk/Sq, NaN everywhere the kernel must not look
# ---------------------------------------------------------------------------
def _nan_view(x, dev):
    """x [H, S, D] -> a [1, S, H, D] view into a NaN-filled [1, S+3, H, D+8]
    buffer: NaN rows after S and NaN gaps between the rows."""
    h, s, d = x.shape
    buf = torch.full((1, s + 3, h, d + 8), float("nan"), device=dev,
                     dtype=x.dtype)
    view = buf[:, :s, :, :d]
    view.copy_(x.transpose(0, 1)[None])
    return view


TAIL_PAIRS = [(1, 1), (31, 7), (33, 63), (100, 64), (1, 65), (31, 77),
              (33, 127), (100, 129), (33, 154), (100, 308), (31, 308)]


class TestTails:
    @pytest.mark.parametrize("d,variant", [(40, "v3"), (40, "v2"),
                                           (80, "v2"), (80, "v3"),
                                           (160, "v2"), (160, "v3")])
    @pytest.mark.parametrize("sq,sk", TAIL_PAIRS)
    def test_no_phantom_keys(self, dev, sq, sk, d, variant):
        assert plan(d, sk, variant)[0] == variant
        q, k, v = tail_inputs(sq, sk, d)
        orc = Oracle(q, k, v, default_scale(d))
        qv, kv, vv = (_nan_view(t, dev) for t in (q, k, v))
        for layout in LAYOUTS:
            if layout == "bshd":
                out = ops.attention_bshd(qv, kv, vv, variant=variant)
                out = out.transpose(1, 2)
            else:
                out = ops.attention(qv.transpose(1, 2), kv.transpose(1, 2),
                                    vv.transpose(1, 2), variant=variant)
            out = out.cpu()
            assert torch.isfinite(out.float()).all()
            worst = orc.worst(out[0], exact=(variant == "v2"))
            report("tails", variant, d, f"Sq={sq} Sk={sk} {layout}", worst)
            assert worst <= 1.0
            if sk == 1:
                assert torch.equal(out[0], v.expand(-1, sq, -1))


# ---------------------------------------------------------------------------
# d. retrieval: any key-row, V-row or d-column permutation shows exactly
# ---------------------------------------------------------------------------
class TestRetrieval:
    @pytest.mark.parametrize("variant", ["v2", "v3"])
    @pytest.mark.parametrize("d", [40, 64, 80, 128, 160])
    def test_output_is_the_matched_value_row(self, dev, d, variant):
        q, k, v, pi = retrieval_inputs(d)
        s = Oracle(q, k, v, default_scale(d)).s
        top2 = s.topk(2, dim=-1)
        assert torch.equal(top2.indices[..., 0], pi)
        assert (top2.values[..., 0] - top2.values[..., 1]).min() >= 40
        want = torch.gather(v, 1, pi[:, :, None].expand(-1, -1, d))
        assert plan(d, k.shape[1], variant)[0] == variant
        for layout in LAYOUTS:
            out = run(q, k, v, layout, dev, variant=variant)
            assert torch.equal(out[0], want), (layout, variant, d)


# ---------------------------------------------------------------------------
# e. production strides: slices of fused QKV / KV projections
# ---------------------------------------------------------------------------
def _check_bshd(q, k, v, out, kernel, d, detail):
    """q/k/v/out: [B, S, H, D] GPU views; fp64 reference on the CPU."""
    orc = Oracle(*(t.transpose(1, 2) for t in (q, k, v)), default_scale(d))
    worst = orc.worst(out.transpose(1, 2), exact=(kernel == "v2"))
    report("strides", kernel, d, detail, worst)
    assert worst <= 1.0


class TestProductionStrides:
    @pytest.mark.parametrize("d,s", [(40, 256), (80, 320)])
    def test_fused_qkv_self_attention(self, dev, d, s):
        h, b = 2, 3
        torch.manual_seed(d)
        qkv = torch.randn(b, s, 3 * h * d, device=dev, dtype=torch.bfloat16)
        q, k, v = (qkv[..., i * h * d:(i + 1) * h * d].unflatten(-1, (h, d))
                   for i in range(3))
        assert plan(d, s)[0] == "v3"
        for variant in ("auto", "v2"):
            kernel = plan(d, s, variant)[0]
            out = ops.attention_bshd(q, k, v, variant=variant)
            _check_bshd(q, k, v, out, kernel, d, f"qkv S={s}")
        # the [B,H,S,D] entry on the transposed views of the same slices
        out = ops.attention(q.transpose(1, 2), k.transpose(1, 2),
                            v.transpose(1, 2))
        _check_bshd(q, k, v, out.transpose(1, 2), "v3", d,
                    f"qkv-transposed S={s}")
        # batch-sliced views, as the regional path makes
        nr = 2
        out = ops.attention_bshd(q[:nr], k[:nr], v[:nr])
        _check_bshd(q[:nr], k[:nr], v[:nr], out, "v3", d,
                    f"qkv[:{nr}] S={s}")
        out = ops.attention_bshd(q[1:], k[1:], v[1:])
        _check_bshd(q[1:], k[1:], v[1:], out, "v3", d, f"qkv[1:] S={s}")

    @pytest.mark.parametrize("sk", [77, 154])
    @pytest.mark.parametrize("d,expect", [(40, ("v3", 48, 256)),
                                          (80, ("v2", 80, 256)),
                                          (160, ("v2", 160, 256))])
    def test_fused_kv_cross_attention(self, dev, d, expect, sk):
        h, b, sq = 2, 2, 260
        torch.manual_seed(d + sk)
        q = torch.randn(b, sq, h, d, device=dev, dtype=torch.bfloat16)
        kv = torch.randn(b, sk, 2 * h * d, device=dev, dtype=torch.bfloat16)
        k, v = (kv[..., i * h * d:(i + 1) * h * d].unflatten(-1, (h, d))
                for i in range(2))
        assert plan(d, sk) == expect
        out = ops.attention_bshd(q, k, v)
        _check_bshd(q, k, v, out, expect[0], d, f"kv Sk={sk}")
        out = ops.attention_bshd(q[:1], k[:1], v[:1])
        _check_bshd(q[:1], k[:1], v[:1], out, expect[0], d,
                    f"kv[:1] Sk={sk}")


# ---------------------------------------------------------------------------
# f. dispatch table (host only)
# ---------------------------------------------------------------------------
class TestDispatch:
    def test_auto_table(self):
        for sk in (1, 77, 255, 256, 4096):
            assert plan(40, sk) == ("v3", 48, 256)
        assert plan(80, 77)[0] == "v2"
        assert plan(80, 255)[0] == "v2"
        assert plan(80, 256) == ("v3", 80, 256)
        assert plan(96, 256) == ("v3", 96, 256)
        assert plan(104, 256) == ("v3", 112, 128)
        assert plan(160, 4096) == ("v3", 160, 128)
        assert plan(160, 77) == ("v2", 160, 256)
        for d in (512, 16, 20, 200):
            assert plan(d, 77) == ("composed", 0, 0)

    def test_forced_overrides_the_table(self):
        assert plan(40, 4096, "v2") == ("v2", 48, 256)
        assert plan(80, 77, "v3") == ("v3", 80, 256)
        assert plan(160, 77, "v3") == ("v3", 160, 128)
        assert plan(160, 4096, "v2") == ("v2", 160, 256)

    def test_forced_on_unsupported_head_dim_raises(self, dev):
        for d in (512, 16, 20):
            for force in (2, 3):
                with pytest.raises(RuntimeError):
                    ops.ext().attention_plan(d, 77, force)
        with pytest.raises(RuntimeError):
            ops.ext().attention_plan(40, 77, 4)
        q = torch.randn(1, 1, 64, 512, device=dev, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            ops.attention(q, q, q, variant="v3")
        q = torch.randn(1, 64, 1, 20, device=dev, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            ops.attention_bshd(q, q, q, variant="v2")
        # a flash kernel cannot take fp32 either: forced means forced
        q = torch.randn(1, 1, 64, 40, device=dev)
        with pytest.raises(RuntimeError):
            ops.attention(q, q, q, variant="v3")

    def test_unknown_variant_raises(self, dev):
        q = torch.randn(1, 1, 64, 40, device=dev, dtype=torch.bfloat16)
        with pytest.raises(ValueError):
            ops.attention(q, q, q, variant="v4")
        with pytest.raises(ValueError):
            ops.attention_bshd(q, q, q, variant="v3all")

    @pytest.mark.parametrize("B,H,Sq,Sk,D", [
        (2, 8, 256, 256, 40), (2, 8, 1024, 1024, 80), (1, 8, 256, 256, 160),
        (2, 8, 64, 64, 160), (2, 8, 256, 77, 40), (1, 10, 128, 128, 64),
        (1, 1, 100, 100, 32), (2, 8, 256, 154, 40),
    ])
    def test_auto_is_the_planned_variant_bit_for_bit(self, dev, B, H, Sq,
                                                     Sk, D):
        # the shapes of test_ops_gpu.py's attention classes
        torch.manual_seed(42)
        q = torch.randn(B, H, Sq, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn(B, H, Sk, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(B, H, Sk, D, device=dev, dtype=torch.bfloat16)
        kernel = plan(D, Sk)[0]
        assert torch.equal(ops.attention(q, k, v, variant="auto"),
                           ops.attention(q, k, v, variant=kernel))
        assert torch.equal(ops.attention(q, k, v),
                           ops.attention(q, k, v, variant="auto"))


# ---------------------------------------------------------------------------
# the composed path: row_softmax_ in bf16, and GEMM + softmax + GEMM
# ---------------------------------------------------------------------------
class TestComposed:
    @pytest.mark.parametrize("S", [1, 63, 77, 300])
    def test_row_softmax_bf16(self, dev, S):
        R, scale = 7, 0.37   # 7 rows: the last block of 4 waves is ragged
        g = torch.Generator().manual_seed(S)
        x = (torch.randn(R, S, generator=g) * 3).bfloat16()
        ref = torch.softmax(x.double() * scale, dim=-1)
        y = x.to(dev)
        ops.ext().row_softmax_(y, scale)
        err = (y.cpu().double() - ref).abs()
        # the exponentials are stored in bf16 and rounded again after the
        # normalisation: 2 * 2^-9 relative, plus the same on the row's max
        tol = 2.0 ** -8 * ref + 2.0 ** -8 * ref.amax(-1, keepdim=True)
        worst = (err / tol).max().item()
        print(f"ATTN row_softmax bf16 S={S} err/tol={worst:.3f}")
        assert worst <= 1.0

    @pytest.mark.parametrize("B,H,Sq,Sk,D", [(1, 3, 70, 77, 512),
                                             (1, 2, 50, 77, 20)])
    def test_composed_end_to_end(self, dev, B, H, Sq, Sk, D):
        """Bound for the composed path, same reference. q.k^T leaves the
        GEMM in bf16, so each scaled score moves by at most 2^-9 |s| and
        each p by a factor e^(+-2 max_j 2^-9 |s_ij|): delta_i =
        2 ln2 2^-9 max_j |s_ij| with s in log2 units (Oracle.
        delta_composed). P is rounded to bf16 twice in row_softmax_ (the
        stored exponentials, then the normalised values): 2 * 2^-9 sum
        p|v|, inside the 2^-7 term; the bf16 output adds 2^-9 |ref|."""
        assert plan(D, Sk) == ("composed", 0, 0)
        torch.manual_seed(D)
        q = torch.randn(B, H, Sq, D, device=dev, dtype=torch.bfloat16)
        kbuf = torch.randn(B, H, Sk, D + 8, device=dev, dtype=torch.bfloat16)
        k = kbuf[..., :D]
        assert not k.is_contiguous()
        v = torch.randn(B, H, Sk, D, device=dev, dtype=torch.bfloat16)
        out = ops.attention(q, k, v)
        worst = Oracle(q, k, v, default_scale(D)).worst(out, composed=True)
        report("composed", "composed", D, f"Sq={Sq} Sk={Sk}", worst)
        assert worst <= 1.0
