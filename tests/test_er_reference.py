"""tests/er_ref.py (the early-reflection rule in float64, over a growing history) and the oracle's ring form, pinned to
each other at both ends of the delay range and of the ring.  CPU only.

The bound is the one test_oracle_primitives.py::test_early_reflections_closed_form already holds the oracle to: relative
RMS < 3e-7 (eight f32 multiply-adds per frame against float64)."""
import numpy as np
import pytest

import er_ref
from helpers import rel_rms

BOUND = 3e-7  # test_early_reflections_closed_form's


def _params(ob, delays, gains):
    p = np.zeros(len(delays), dtype=ob.PARAMS_DTYPE)
    p["er_delay"], p["er_gain"] = delays, gains
    return p


def _clamped(p, F, R):
    q = p.copy()
    q["er_delay"] = er_ref.effective_delays(p["er_delay"], F, R)
    return q


@pytest.mark.parametrize("F,R", er_ref.FRAMES_RINGS)
def test_edge_delays_cover_the_issue_table(F, R):
    """Every entry the table promises is there, none is dropped but those outside 1 .. m, and the drawing helper hands
    every entry out in every draw of 24 sources (and over the three draws of a one-source case)."""
    m = R - F
    inside, outside = er_ref.edge_delays(F, R)
    listed = [1, 2, 63, 64, 65, F - 1, F, F + 1, m - 65, m - 64, m - 63, m - 1, m]
    assert set(inside) == {d for d in listed if 1 <= d <= m}
    assert {d for d in listed if not 1 <= d <= m} <= ({F + 1} if R == 2 * F else set())  # only F + 1 at R = 2F may go
    assert {1, 2, 63, 64, 65, F - 1, F, m - 65, m - 64, m - 63, m - 1, m} <= set(inside)
    assert outside == [0, m + 1, R, R + 1, 0xFFFFFFFF]
    assert all(d == 0 or d > m for d in outside) and all(1 <= d <= m for d in inside)
    big = er_ref.TapDrawer(np.random.default_rng(F + R), F, R)
    for _ in range(3):
        delays, gains = big.draw(24)
        assert set(np.unique(np.abs(gains))) <= set(np.float32(0.7 ** np.arange(1, 9))) | {np.float32(0)}
    big.assert_covered()
    assert 14 <= big.repeats() <= 22  # about a quarter of 72
    one = er_ref.TapDrawer(np.random.default_rng(F), F, R)
    for _ in range(3):
        one.draw(1)
    one.assert_covered(per_draw=False)
    with pytest.raises(AssertionError):
        one.assert_covered()  # eight taps cannot hold the table: the per-draw form must notice


@pytest.mark.parametrize("F,R", er_ref.FRAMES_RINGS)
def test_oracle_matches_the_closed_form_at_the_edges(ob, F, R):
    """The oracle gets min(d, R - F), never 0; er_ref gets the raw values.  24 sources, 2R/F + 3 callbacks, parameters
    redrawn every third; every source and every frame compared, per source."""
    n, T = 24, er_ref.callbacks(F, R)
    rng = np.random.default_rng(R + F)
    inside, outside = er_ref.edge_delays(F, R)
    drawer = er_ref.TapDrawer(rng, F, R, table=inside + [d for d in outside if d != 0])
    ora = [ob.BatchOracle(ob.KIND_EFFECT, 1, F, chain=[ob.FX_EARLY_REFLECTIONS], er_ring_frames=R) for _ in range(n)]
    bank = er_ref.ErBank(n, F, R)
    got, want = [], []
    for b in range(T):
        if b % 3 == 0:
            p = _params(ob, *drawer.draw(n))
            pc = _clamped(p, F, R)
            assert pc["er_delay"].min() >= 1 and pc["er_delay"].max() == R - F
        x = rng.uniform(-0.5, 0.5, (n, F, 2)).astype(np.float32)
        got.append(np.stack([ora[s].block(pc[s : s + 1], x[s : s + 1])[0][0] for s in range(n)]))
        want.append(bank.block(p, x))
    drawer.assert_covered()
    got, want = np.stack(got), np.stack(want)  # [T][n][F][2]
    worst = max(rel_rms(got[:, s], want[:, s]) for s in range(n))
    print(f"F {F} R {R}: worst per-source rel rms {worst:.3e} over {T} callbacks")
    assert worst < BOUND
    assert rel_rms(got[-1], want[-1]) < BOUND  # the last callback alone: after two wraps of the write position


@pytest.mark.parametrize("F,R", [(128, 256), (512, 4096)])
def test_delay_zero_adds_the_frame_itself(ob, F, R):
    """A table of its own: 0 next to a few legal delays.  The oracle writes the block into the ring before it reads, so
    it is a sound reference for 0 too; with all eight taps at 0 the output is x * (1 + sum g) whatever came before."""
    n, T = 6, er_ref.callbacks(F, R)
    rng = np.random.default_rng(3)
    drawer = er_ref.TapDrawer(rng, F, R, table=[0, 0, 1, F, R - F])
    ora = ob.BatchOracle(ob.KIND_EFFECT, n, F, chain=[ob.FX_EARLY_REFLECTIONS], er_ring_frames=R)
    one = [ob.BatchOracle(ob.KIND_EFFECT, 1, F, chain=[ob.FX_EARLY_REFLECTIONS], er_ring_frames=R) for _ in range(n)]
    bank = er_ref.ErBank(n, F, R)
    for b in range(T):
        if b % 3 == 0:
            p = _params(ob, *drawer.draw(n))
            p["er_delay"][0] = 0  # source 0: all eight taps
        x = rng.uniform(-0.5, 0.5, (n, F, 2)).astype(np.float32)
        want = bank.block(p, x)
        _, _, mix64 = ora.block(p, x, want64=True)
        assert rel_rms(mix64[0], want.sum(axis=0)) < BOUND, b
        for s in range(n):
            assert rel_rms(one[s].block(p[s : s + 1], x[s : s + 1])[0][0], want[s]) < BOUND, (b, s)
        scale = 1.0 + p["er_gain"][0].astype(np.float64).sum()
        assert rel_rms(want[0], x[0].astype(np.float64) * scale) < BOUND, b
    drawer.assert_covered()


def test_a_playback_left_out_of_a_callback_keeps_its_history(ob):
    """Three interleaved subsets, each callback takes two of them, rotating: a source's history is the callbacks it
    took part in, nothing else, in er_ref (by construction) and in a per-source oracle (its ring and write position
    only move when it is called)."""
    F, R, n = 128, 256, 12
    rng = np.random.default_rng(17)
    drawer = er_ref.TapDrawer(rng, F, R, table=er_ref.edge_delays(F, R)[0])
    ora = [ob.BatchOracle(ob.KIND_EFFECT, 1, F, chain=[ob.FX_EARLY_REFLECTIONS], er_ring_frames=R) for _ in range(n)]
    bank = er_ref.ErBank(n, F, R)
    took_part = np.zeros(n, int)
    for b in range(3 * R // F + 3):
        if b % 3 == 0:
            p = _params(ob, *drawer.draw(n))
        active = [s for s in range(n) if s % 3 != b % 3]
        x = rng.uniform(-0.5, 0.5, (len(active), F, 2)).astype(np.float32)
        want = bank.block(p[active], x, active)
        for r, s in enumerate(active):
            got = ora[s].block(p[s : s + 1], x[r : r + 1])[0][0]
            assert rel_rms(got, want[r]) < BOUND, (b, s)
            took_part[s] += 1
    assert took_part.min() >= 2 * R // F and len(set(took_part)) == 1
    drawer.assert_covered()
    for s in range(n):
        assert len(bank.sources[s].hist) == took_part[s] * F
