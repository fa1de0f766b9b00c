"""CPU tests of tests/attention_oracle.py: the bound accepts a faithful
model of the v3 kernel's arithmetic and rejects deliberately wrong results,
and the structured inputs of test_attention_gpu.py do what they claim."""
import pytest
import torch

from attention_oracle import (KVB, Oracle, RESCALE_KINDS, default_scale,
                              emulate_v3, exact_scale, rescale_inputs,
                              retrieval_inputs, tail_inputs, tile_walk)


def _emulate(q, k, v, scale, **kw):
    return torch.stack([emulate_v3(q[h], k[h], v[h], scale, **kw)
                        for h in range(q.shape[0])])


class TestTileWalk:
    def test_random_scores_never_trigger(self):
        # what the older attention tests feed the kernel: no rescale after
        # tile 0, so they cannot see a wrong alpha broadcast
        torch.manual_seed(42)
        q = torch.randn(256, 80).bfloat16()
        k = torch.randn(256, 80).bfloat16()
        o = Oracle(q, k, k, default_scale(80))
        assert tile_walk(o.s)["triggers"] == 0

    def test_counts_on_a_hand_made_walk(self):
        # 64 rows = 2 waves, 3 tiles. Wave 0: row 0 jumps by 20 at tile 1,
        # the other rows stay -> one mixed trigger. Wave 1: every row grows
        # 6 per tile -> deferred at tile 1 (6 <= 8), rescaled at tile 2
        # (12 > 8), all rows alike -> not mixed.
        s = torch.zeros(64, 3 * KVB, dtype=torch.float64)
        s[0, KVB:2 * KVB] = 20.0
        s[32:, KVB:2 * KVB] = 6.0
        s[32:, 2 * KVB:] = 12.0
        w = tile_walk(s)
        assert w["triggers"] == 2 and w["mixed"] == 1
        assert w["per_tile"] == [0, 1, 1]
        assert w["deferred"] == 6.0

    def test_threshold_is_strict(self):
        s = torch.zeros(32, 2 * KVB, dtype=torch.float64)
        s[:, KVB:] = 8.0   # pmax <= m + THR: deferred
        assert tile_walk(s)["triggers"] == 0
        s[:, KVB:] = 8.5
        assert tile_walk(s)["triggers"] == 1


class TestExactScale:
    @pytest.mark.parametrize("k", [2, 3, 4])
    def test_prescale_is_exact_in_bf16(self, k):
        l2 = (torch.tensor(exact_scale(k), dtype=torch.float32)
              * torch.tensor(1.4426950408889634, dtype=torch.float32))
        q = torch.randn(4096).bfloat16()
        assert torch.equal((q.float() * l2).bfloat16().float(),
                           q.float() * 2.0 ** -k)


class TestBoundAcceptsTheModel:
    def test_default_scale_randn(self):
        torch.manual_seed(1)
        q = torch.randn(2, 100, 80).bfloat16()
        k = torch.randn(2, 150, 80).bfloat16()
        v = torch.randn(2, 150, 80).bfloat16()
        sc = default_scale(80)
        worst = Oracle(q, k, v, sc).worst(_emulate(q, k, v, sc))
        print(f"emulated v3, randn, default scale: err/bound {worst:.3f}")
        assert worst < 0.5

    @pytest.mark.parametrize("kind", RESCALE_KINDS)
    def test_rescale_family(self, kind):
        q, k, v, sc = rescale_inputs(kind, 40)
        worst = Oracle(q, k, v, sc).worst(_emulate(q, k, v, sc), exact=True)
        print(f"emulated v3, {kind}: err/bound {worst:.3f}")
        assert worst < 0.5


class TestRescaleInputs:
    @pytest.mark.parametrize("d", [40, 160])
    def test_ramp_triggers_every_tile_in_mixed_waves(self, d):
        q, k, v, sc = rescale_inputs("ramp", d)
        for h in range(q.shape[0]):
            w = tile_walk(Oracle(q[h], k[h], v[h], sc).s)
            assert all(n >= 1 for n in w["per_tile"][1:]), w
            assert w["mixed"] >= 1, w

    def test_old_tiles_carry_weight(self):
        # on the a=12 rows the tiles before the last hold most of sum p|v|:
        # a wrong rescale of the accumulator cannot hide
        q, k, v, sc = rescale_inputs("ramp", 40)
        o = Oracle(q[0], k[0], v[0], sc)
        old = o.p[:, :4 * KVB] @ v[0, :4 * KVB].double().abs()
        frac = (old / o.pav)[0::4].mean().item()
        assert 0.5 < frac < 0.9, frac

    def test_creep_defers_then_triggers(self):
        q, k, v, sc = rescale_inputs("creep", 40)
        w = tile_walk(Oracle(q[0], k[0], v[0], sc).s)
        assert w["triggers"] >= 1 and w["deferred"] > 4.0, w

    def test_decreasing_never_triggers(self):
        q, k, v, sc = rescale_inputs("decreasing", 40)
        w = tile_walk(Oracle(q[0], k[0], v[0], sc).s)
        assert w["triggers"] == 0, w

    def test_lastkey_triggers_in_the_ragged_tile_only(self):
        q, k, v, sc = rescale_inputs("lastkey", 40)
        w = tile_walk(Oracle(q[0], k[0], v[0], sc).s)
        assert w["per_tile"][-1] >= 1 and sum(w["per_tile"][:-1]) == 0, w
        assert w["mixed"] >= 1, w


class TestBoundRejectsWrongResults:
    def test_alpha_from_neighbouring_row(self):
        q, k, v, sc = rescale_inputs("ramp", 40)
        r = Oracle(q, k, v, sc).ratio(
            _emulate(q, k, v, sc, alpha="neighbour"), exact=True)
        bad_rows = (r.amax(-1) > 1).float().mean().item()
        assert bad_rows > 0.5, bad_rows

    @pytest.mark.parametrize("kind", ["ramp", "creep", "lastkey"])
    def test_no_rescale_at_all(self, kind):
        q, k, v, sc = rescale_inputs(kind, 40)
        r = Oracle(q, k, v, sc).ratio(
            _emulate(q, k, v, sc, alpha="none"), exact=True)
        assert (r.amax(-1) > 1).float().mean().item() > 0.4

    def test_two_v_rows_swapped(self):
        q, k, v, sc = rescale_inputs("ramp", 40)
        vs = v.clone()
        vs[:, [70, 270]] = v[:, [270, 70]]
        wrong = Oracle(q, k, vs, sc).ref
        assert Oracle(q, k, v, sc).worst(wrong, exact=True) > 1

    def test_last_key_dropped(self):
        # on the lastkey input that key holds the mass of the a=12/10 rows
        # (one of 77 similar keys, as in the tail inputs, would hide)
        q, k, v, sc = rescale_inputs("lastkey", 40)
        wrong = Oracle(q, k[:, :-1], v[:, :-1], sc).ref
        r = Oracle(q, k, v, sc).ratio(wrong, exact=True)
        assert (r.amax(-1) > 1).float().mean().item() >= 0.5

    @pytest.mark.parametrize("sq,sk,d", [(33, 77, 40), (31, 1, 80),
                                         (100, 308, 160), (1, 129, 80)])
    def test_phantom_key_rejected_on_every_element(self, sq, sk, d):
        # one zero key (score 0, value 0) admitted after Sk
        q, k, v = tail_inputs(sq, sk, d)
        sc = default_scale(d)
        z = torch.zeros(q.shape[0], 1, d, dtype=k.dtype)
        wrong = Oracle(q, torch.cat([k, z], 1), torch.cat([v, z], 1), sc).ref
        r = Oracle(q, k, v, sc).ratio(wrong)
        print(f"phantom key Sq={sq} Sk={sk} D={d}: min err/bound "
              f"{r.min().item():.1f}")
        assert r.min().item() > 1

    def test_absent_tail_mask_rejected_on_every_element(self):
        q, k, v = tail_inputs(33, 77, 40)
        sc = default_scale(40)
        z = torch.zeros(q.shape[0], 2 * KVB - 77, 40, dtype=k.dtype)
        wrong = Oracle(q, torch.cat([k, z], 1), torch.cat([v, z], 1), sc).ref
        assert Oracle(q, k, v, sc).ratio(wrong).min().item() > 1

    def test_phantom_key_hides_in_random_data(self):
        # the reason the tail tests are structured: on randn inputs a
        # phantom zero key moves most elements by less than any bound that
        # still admits bf16 rounding
        torch.manual_seed(3)
        q = torch.randn(2, 33, 40).bfloat16()
        k = torch.randn(2, 77, 40).bfloat16()
        v = torch.randn(2, 77, 40).bfloat16()
        sc = default_scale(40)
        z = torch.zeros(2, 1, 40, dtype=k.dtype)
        wrong = Oracle(q, torch.cat([k, z], 1), torch.cat([v, z], 1), sc).ref
        r = Oracle(q, k, v, sc).ratio(wrong)
        assert (r > 1).float().mean().item() < 0.5


class TestRetrievalInputs:
    @pytest.mark.parametrize("d", [40, 64, 80, 128, 160])
    def test_matched_score_wins_by_40(self, d):
        q, k, v, pi = retrieval_inputs(d)
        o = Oracle(q, k, v, default_scale(d))
        top2 = o.s.topk(2, dim=-1)
        assert torch.equal(top2.indices[..., 0], pi)
        assert (top2.values[..., 0] - top2.values[..., 1]).min() >= 40
        want = torch.gather(v, 1, pi[:, :, None].expand(-1, -1, d))
        assert torch.equal(o.ref.bfloat16(), want)


class TestVariantArgument:
    def test_unknown_variant_raises_on_any_device(self):
        from sdwd_amd import ops
        q = torch.randn(1, 1, 8, 40)
        with pytest.raises(ValueError):
            ops.attention(q, q, q, variant="v4")
        with pytest.raises(ValueError):
            ops.attention_bshd(q, q, q, variant="v3all")
        assert ops.attention(q, q, q, variant="v3").shape == q.shape

    @pytest.mark.parametrize("env,force", [("v2", 2), ("v3all", 3),
                                           ("v3", 0), ("", 0), ("auto", 0)])
    def test_none_follows_the_environment(self, monkeypatch, env, force):
        from sdwd_amd import ops
        monkeypatch.setenv("SDWD_ATTN", env)
        monkeypatch.setattr(ops, "_ATTN_ENV_FORCE", None)
        assert ops._attn_force(None) == force
        assert ops._attn_force("v3") == 3 and ops._attn_force("auto") == 0
