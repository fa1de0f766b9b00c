"""ops.attention_blend_bshd on the CPU: the fp32 reference path against a
hand-written fp64 per-context sum, the table semantics (kv_len, kv_index,
batch-broadcast w), argument validation, and the model layer's routing (the
CPU always takes the per-region loop)."""
import math

import pytest
import torch

from sdwd_amd import ops
from sdwd_amd.models.unet import CrossAttention, RegionalContext
from sdwd_amd.pipeline.pipeline import _region_masks

B, BK, SQ, SK, H, D, C = 2, 4, 19, 13, 2, 8, 3


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, SQ, H, D, generator=g)
    k = torch.randn(BK, SK, H, D, generator=g)
    v = torch.randn(BK, SK, H, D, generator=g)
    w = torch.randn(B, C, SQ, generator=g)
    return q, k, v, w


def _fp64(q, k, v, w, index, lens, scale):
    """out[b,s,h] = sum_c w[b,c,s] softmax(scale q K_c^T) V_c, in fp64."""
    q, k, v, w = q.double(), k.double(), v.double(), w.double()
    out = torch.zeros_like(q)
    for b in range(q.shape[0]):
        for c in range(w.shape[1]):
            row = index[b][c]
            n = lens[row]
            for h in range(q.shape[2]):
                s = q[b, :, h] @ k[row, :n, h].T * scale
                p = torch.softmax(s, dim=-1)
                wc = w[b if w.shape[0] > 1 else 0, c]
                out[b, :, h] += wc[:, None] * (p @ v[row, :n, h])
    return out


INDEX = [[0, 2, 3], [1, 2, 3]]
FULL = [SK] * BK


class TestReference:
    def test_matches_fp64_per_context_sum(self):
        q, k, v, w = _inputs()
        out = ops.attention_blend_bshd(q, k, v, w, INDEX)
        assert out.shape == q.shape and out.dtype == q.dtype
        want = _fp64(q, k, v, w, INDEX, FULL, 1.0 / math.sqrt(D))
        assert torch.allclose(out.double(), want, rtol=1e-5, atol=1e-5)

    def test_explicit_scale(self):
        q, k, v, w = _inputs(1)
        out = ops.attention_blend_bshd(q, k, v, w, INDEX, scale=0.7)
        want = _fp64(q, k, v, w, INDEX, FULL, 0.7)
        assert torch.allclose(out.double(), want, rtol=1e-5, atol=1e-5)

    def test_kv_len_hides_keys_past_the_length(self):
        q, k, v, w = _inputs(2)
        lens = [5, 13, 1, 7]
        want = _fp64(q, k, v, w, INDEX, lens, 1.0 / math.sqrt(D))
        k, v = k.clone(), v.clone()
        for row, n in enumerate(lens):
            k[row, n:] = float("nan")
            v[row, n:] = float("nan")
        for table in (lens, torch.tensor(lens), torch.tensor(lens).int()):
            out = ops.attention_blend_bshd(q, k, v, w, INDEX, table)
            assert torch.isfinite(out).all()
            assert torch.allclose(out.double(), want, rtol=1e-5, atol=1e-5)

    def test_kv_index_sharing_and_permutation(self):
        q, k, v, w = _inputs(3)
        sc = 1.0 / math.sqrt(D)
        for index in ([[3, 3, 0], [0, 1, 3]], [[2, 1, 0], [3, 2, 1]],
                      torch.tensor([[0, 0, 0], [1, 1, 1]])):
            out = ops.attention_blend_bshd(q, k, v, w, index)
            rows = index.tolist() if torch.is_tensor(index) else index
            want = _fp64(q, k, v, w, rows, FULL, sc)
            assert torch.allclose(out.double(), want, rtol=1e-5, atol=1e-5)
        # permuting K/V rows and the table together changes nothing
        perm = [2, 0, 3, 1]              # new row i holds old row perm[i]
        inv = [perm.index(i) for i in range(BK)]
        a = ops.attention_blend_bshd(q, k, v, w, INDEX)
        b = ops.attention_blend_bshd(
            q, k[perm], v[perm], w, [[inv[i] for i in r] for r in INDEX])
        assert torch.equal(a, b)

    def test_batch_broadcast_weights(self):
        q, k, v, w = _inputs(4)
        w1 = w[:1].contiguous()
        a = ops.attention_blend_bshd(q, k, v, w1, INDEX)
        b = ops.attention_blend_bshd(q, k, v, w1.expand(B, -1, -1).contiguous(),
                                     INDEX)
        assert torch.equal(a, b)
        want = _fp64(q, k, v, w1, INDEX, FULL, 1.0 / math.sqrt(D))
        assert torch.allclose(a.double(), want, rtol=1e-5, atol=1e-5)

    def test_single_context_unit_weight_is_plain_attention(self):
        q, k, v, _ = _inputs(5)
        w = torch.ones(B, 1, SQ)
        out = ops.attention_blend_bshd(q, k, v, w, [[0], [1]])
        want = ops.attention_bshd(q, k[:B], v[:B])
        assert torch.allclose(out, want, rtol=1e-5, atol=1e-6)

    def test_strided_kv_views(self):
        q, k, v, w = _inputs(6)
        kv = torch.cat([k.flatten(2), v.flatten(2)], dim=-1)  # fused K/V GEMM
        ks = kv[..., :H * D].unflatten(-1, (H, D))
        vs = kv[..., H * D:].unflatten(-1, (H, D))
        assert not ks.is_contiguous()
        assert torch.equal(ops.attention_blend_bshd(q, ks, vs, w, INDEX),
                           ops.attention_blend_bshd(q, k, v, w, INDEX))


class TestValidation:
    def _call(self, **over):
        q, k, v, w = _inputs()
        args = dict(q=q, k=k, v=v, w=w, kv_index=INDEX, kv_len=None)
        args.update(over)
        return ops.attention_blend_bshd(**args)

    def test_index_out_of_range(self):
        for bad in ([[0, 2, BK], [1, 2, 3]], [[0, -1, 3], [1, 2, 3]],
                    torch.tensor([[0, 2, 3], [1, 2, 4]])):
            with pytest.raises(ValueError, match="kv_index"):
                self._call(kv_index=bad)

    def test_index_shape(self):
        for bad in ([[0, 2], [1, 2]], [[0, 2, 3]], [0, 1, 2],
                    [[0, 2, 3], [1, 2]]):
            with pytest.raises(ValueError, match="kv_index"):
                self._call(kv_index=bad)

    def test_index_must_hold_integers(self):
        with pytest.raises(ValueError, match="kv_index"):
            self._call(kv_index=torch.zeros(B, C))

    def test_length_out_of_range(self):
        for bad in ([0, 1, 1, 1], [1, 1, 1, SK + 1], [-3, 1, 1, 1]):
            with pytest.raises(ValueError, match="kv_len"):
                self._call(kv_len=bad)

    def test_length_shape(self):
        for bad in ([1, 1, 1], [[1, 1, 1, 1]], torch.ones(BK + 1).long()):
            with pytest.raises(ValueError, match="kv_len"):
                self._call(kv_len=bad)

    def test_no_contexts(self):
        with pytest.raises(ValueError, match="C >= 1"):
            self._call(w=torch.zeros(B, 0, SQ), kv_index=[[], []])

    def test_weight_shape_and_dtype(self):
        for bad in (torch.zeros(B, C, SQ + 1), torch.zeros(B + 1, C, SQ),
                    torch.zeros(C, SQ), torch.zeros(B, C, SQ).double()):
            with pytest.raises(ValueError, match=r"\bw\b"):
                self._call(w=bad)

    def test_kv_shapes(self):
        q, k, v, w = _inputs()
        with pytest.raises(ValueError, match="k and v"):
            self._call(v=v[:, :-1])
        with pytest.raises(ValueError, match=r"\bk\b"):
            self._call(k=k[..., :-1], v=v[..., :-1])
        with pytest.raises(ValueError, match=r"\bq\b"):
            self._call(q=q[0])


class TestModelRoutingOnCPU:
    @pytest.mark.parametrize("switch", [True, False])
    def test_cpu_takes_the_loop(self, monkeypatch, switch):
        def boom(*a, **kw):
            raise AssertionError("fused blend op reached on the CPU")

        monkeypatch.setattr(ops, "attention_blend_bshd", boom)
        monkeypatch.setattr(CrossAttention, "fused_regional", switch)
        torch.manual_seed(0)
        d, heads, s, b = 32, 4, 16, 3
        attn = CrossAttention(d, d, heads).eval()
        x = torch.randn(b, s, d)
        rc = RegionalContext(
            torch.randn(b, 77, d), torch.randn(2, 77, d),
            _region_masks("columns", [1.0, 1.0], 4, 4), rows=2,
            base_ratio=0.25, lat_hw=(4, 4))
        with torch.no_grad():
            out = attn(x, rc)
        assert out.shape == (b, s, d) and torch.isfinite(out).all()

    @pytest.mark.parametrize("mode,base,rtok,rows", [
        ("columns", 0.25, 77, 2), ("rows", 0.0, 77, 2),
        ("columns", 0.25, 154, 2), ("rows", 0.3, 40, 3)])
    def test_fused_route_builds_the_same_blend(self, monkeypatch, mode, base,
                                               rtok, rows):
        """The fused route's contexts, lengths, index table and weights,
        checked where it never runs by itself: with the predicate forced,
        the op's fp32 reference path must reproduce the loop."""
        torch.manual_seed(1)
        d, heads, s, b = 32, 4, 64, 3
        attn = CrossAttention(d, d, heads).eval()
        x = torch.randn(b, s, d)
        rc = RegionalContext(
            torch.randn(b, 77, d), torch.randn(2, rtok, d),
            _region_masks(mode, [1.0, 2.0], 8, 8), rows=rows,
            base_ratio=base, lat_hw=(8, 8))
        with torch.no_grad():
            monkeypatch.setattr(CrossAttention, "fused_regional", False)
            loop = attn(x, rc)
            calls = []
            blend = ops.attention_blend_bshd

            def counted(*a, **kw):
                calls.append(a)
                return blend(*a, **kw)

            monkeypatch.setattr(ops, "attention_blend_bshd", counted)
            monkeypatch.setattr(ops, "attention_blend_supported",
                                lambda q, k, v: True)
            monkeypatch.setattr(CrossAttention, "fused_regional", True)
            fused = attn(x, rc)
        assert len(calls) == 1
        q, k, v, w, index, lens = calls[0]
        assert q.shape[0] == rows and k.shape[:2] == (rows + 2, max(77, rtok))
        assert index.tolist() == [[i, rows, rows + 1] for i in range(rows)]
        assert lens.tolist() == [77] * rows + [rtok] * 2
        assert w.shape == (1, 3, s) and w.dtype == torch.float32
        assert torch.allclose(fused, loop, atol=1e-5), (
            (fused - loop).abs().max())
        assert torch.equal(fused[rows:], loop[rows:])

    def test_switch_defaults_on(self):
        assert CrossAttention.fused_regional is True

    def test_supported_predicate_is_false_on_cpu(self):
        q, k, v, _ = _inputs()
        assert ops.attention_blend_supported(q, k, v) is False
        qb = q.bfloat16()
        assert ops.attention_blend_supported(qb, k.bfloat16(),
                                             v.bfloat16()) is False
