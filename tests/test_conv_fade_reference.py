"""tests/conv_fade_ref.py checked by hand and against conv_ref, without a GPU: the fade rule of include/gas_amd.h, its
state machine, and the float64 model of two IRs' spectra over one ring."""
import numpy as np
import pytest

from conv_fade_ref import ConvFadeRef, DualPartitionModel, fade_s
from conv_ref import ConvRef

F = 128


def noise(rng, blocks, frames=F):
    return [rng.uniform(-1, 1, (frames, 2)) for _ in range(blocks)]


def test_s_is_the_float32_value_the_header_states():
    for n in (1, 3, 4096):
        s = np.concatenate([fade_s(512, n, b) for b in (range(n) if n < 9 else (0, 1, n - 1))])
        assert s[0] == 0.0 and s.max() < 1.0
        if n < 9:  # N F <= 2^21: the products are the exact ratios rounded once
            np.testing.assert_array_equal(s, (np.arange(n * 512, dtype=np.float32) * np.float32(1.0 / (n * 512))).astype(np.float64))
            np.testing.assert_allclose(s, np.arange(n * 512) / (n * 512), rtol=2e-7, atol=0)
    assert fade_s(512, 4096, 4095)[-1] == float(np.float32(4096 * 512 - 1) * (np.float32(1.0) / np.float32(4096 * 512)))


@pytest.mark.parametrize("n", [1, 3])
def test_by_hand_delta_to_twice_delta(n):
    """A = delta, B = 2 delta, dry = 0: y = (1 + s) x."""
    rng = np.random.default_rng(1)
    blocks = noise(rng, n + 2)
    r = ConvFadeRef(F, [1.0])
    np.testing.assert_allclose(r.process(blocks[0]), blocks[0], atol=1e-15)
    r.fade_to([2.0], 0.0, 1.0, n)
    assert r.fade_remaining() == n
    for b in range(n):
        s = (np.arange(F) + b * F) / (n * F)
        np.testing.assert_allclose(r.process(blocks[1 + b]), (1.0 + s)[:, None] * blocks[1 + b], rtol=1e-6, atol=0)
        assert r.fade_remaining() == n - 1 - b
    np.testing.assert_allclose(r.process(blocks[n + 1]), 2.0 * blocks[n + 1], atol=1e-15)


def test_level_only_fade_is_the_lerp_of_the_levels():
    rng = np.random.default_rng(2)
    ir = rng.standard_normal((2, 2 * F + 3)) / 16
    blocks = noise(rng, 5)
    r, wet_only, dry_only = ConvFadeRef(F, ir, 0.75, -0.5), ConvRef(ir, 0.0, 1.0), ConvRef(ir, 1.0, 0.0)
    x0 = blocks[0]
    assert np.abs(r.process(x0) - (0.75 * dry_only.process(x0) - 0.5 * wet_only.process(x0))).max() <= 1e-12
    r.fade_to(ir, 0.0, 1.0, 3)
    for b in range(3):
        s = fade_s(F, 3, b)[:, None]
        dry, wet = (1 - s) * 0.75, (1 - s) * -0.5 + s
        want = dry * dry_only.process(blocks[1 + b]) + wet * wet_only.process(blocks[1 + b])
        assert np.abs(r.process(blocks[1 + b]) - want).max() <= 1e-12
    assert np.abs(r.process(blocks[4]) - wet_only.process(blocks[4])).max() <= 1e-12


def test_zero_blocks_is_the_hard_switch_and_after_the_fade_is_state_b_exactly():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((1, 5)), rng.standard_normal((2, 3 * F)) / 16
    blocks = noise(rng, 8)
    hard, zero, fade = ConvRef(a), ConvFadeRef(F, a), ConvFadeRef(F, a)
    for i, x in enumerate(blocks):
        if i == 2:
            hard.set_ir(b), hard.set_levels(0.25, 0.5)
            zero.fade_to(b, 0.25, 0.5, 0)
            fade.fade_to(b, 0.25, 0.5, 3)
        want = hard.process(x)
        np.testing.assert_array_equal(zero.process(x), want)
        got = fade.process(x)
        if i < 2 or i >= 5:  # before the fade, and from its (N + 1)-th call on
            np.testing.assert_array_equal(got, want)
        else:
            assert np.abs(got - want).max() > 1e-3
    assert zero.fade_remaining() == 0 and fade.fade_remaining() == 0


def test_first_frame_is_all_a_and_the_fade_is_continuous_into_b():
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((2, F + 1)), rng.standard_normal((2, 9))
    blocks = noise(rng, 4)
    r, ra, rb = ConvFadeRef(F, a), ConvRef(a), ConvRef(b)
    r.fade_to(b, 0.0, 1.0, 4)
    ya = np.concatenate([ra.process(x) for x in blocks])
    yb = np.concatenate([rb.process(x) for x in blocks])
    y = np.concatenate([r.process(x) for x in blocks])
    np.testing.assert_array_equal(y[0], ya[0])
    s_last = (4 * F - 1) / (4 * F)
    np.testing.assert_allclose(y[-1], (1 - s_last) * ya[-1] + s_last * yb[-1], rtol=1e-6, atol=1e-12)


def test_pending_target_starts_after_the_fade_and_the_latest_wins():
    rng = np.random.default_rng(5)
    a, b, c, d = (rng.standard_normal((2, t)) / 8 for t in (7, F + 1, 2 * F, 3))
    blocks = noise(rng, 8)
    r = ConvFadeRef(F, a)
    ra, rb, rd = ConvRef(a), ConvRef(b, 0.5, 0.5), ConvRef(d, 0.0, 2.0)
    r.fade_to(b, 0.5, 0.5, 2)
    remaining = []
    for i, x in enumerate(blocks):
        if i == 1:  # both arrive during the first fade: the later one is kept
            r.fade_to(c, 1.0, 1.0, 5)
            assert r.fade_remaining() == 1 + 5
            r.fade_to(d, 0.0, 2.0, 3)
            assert len(r.named()) == 3
        remaining.append(r.fade_remaining())
        ya, yb, yd = ra.process(x), rb.process(x), rd.process(x)
        if i < 2:
            want = (1 - fade_s(F, 2, i)[:, None]) * ya + fade_s(F, 2, i)[:, None] * yb
        elif i < 5:  # the pending fade: from B, over its own three calls
            want = (1 - fade_s(F, 3, i - 2)[:, None]) * yb + fade_s(F, 3, i - 2)[:, None] * yd
        else:
            want = yd
        assert np.abs(r.process(x) - want).max() <= 1e-12, i
    assert remaining == [2, 1 + 3, 3, 2, 1, 0, 0, 0]


def test_a_skipped_call_does_not_advance_the_fade():
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((2, 9)), rng.standard_normal((2, F + 5))
    blocks = noise(rng, 5)
    r, ra, rb = ConvFadeRef(F, a), ConvRef(a), ConvRef(b)
    r.fade_to(b, 0.0, 1.0, 3)
    calls = 0
    for i, x in enumerate(blocks):
        if i == 1:  # this callback does not name the instance: it is not given the block, and nothing moves
            assert r.fade_remaining() == 3 - calls
            continue
        ya, yb = ra.process(x), rb.process(x)
        s = fade_s(F, 3, calls)[:, None] if calls < 3 else 1.0
        assert np.abs(r.process(x) - ((1 - s) * ya + s * yb)).max() <= 1e-12, i
        calls += 1
        assert r.fade_remaining() == max(0, 3 - calls)


def test_set_ir_set_levels_and_reset_end_a_fade():
    rng = np.random.default_rng(7)
    a, b, c = rng.standard_normal((2, 9)), rng.standard_normal((2, F + 5)) / 8, rng.standard_normal((1, 2 * F)) / 8
    blocks = noise(rng, 6)
    # set_levels mid-fade: state B at once, pending dropped, then the levels
    r, want = ConvFadeRef(F, a), ConvRef(a)
    r.fade_to(b, 0.5, 0.5, 4)
    r.process(blocks[0]), want.process(blocks[0])
    r.fade_to(c, 1.0, 1.0, 2)
    r.set_levels(0.25, 2.0)
    want.set_ir(b), want.set_levels(0.25, 2.0)
    assert r.fade_remaining() == 0 and len(r.named()) == 1
    np.testing.assert_array_equal(r.process(blocks[1]), want.process(blocks[1]))
    # set_ir mid-fade: B's levels stay, the IR is the new one
    r.fade_to(a, 0.0, 1.0, 3)
    r.process(blocks[2]), want.process(blocks[2])
    r.set_ir(c)
    want.set_ir(c), want.set_levels(0.0, 1.0)
    np.testing.assert_array_equal(r.process(blocks[3]), want.process(blocks[3]))
    # reset mid-fade with a pending target: a fresh instance in the pending state
    r.fade_to(b, 0.5, 0.5, 3)
    r.process(blocks[4])
    r.fade_to(a, 0.75, -1.0, 2)
    r.reset()
    assert r.fade_remaining() == 0
    np.testing.assert_array_equal(r.process(blocks[5]), ConvRef(a, 0.75, -1.0).process(blocks[5]))
    # reset mid-fade without one: state B
    r.fade_to(c, 0.0, 1.0, 3)
    r.process(blocks[0])
    r.reset()
    np.testing.assert_array_equal(r.process(blocks[1]), ConvRef(c, 0.0, 1.0).process(blocks[1]))


@pytest.mark.parametrize("frames", [128, 384])
def test_dual_partition_model_equals_the_reference_across_a_ring_wrap(frames):
    rng = np.random.default_rng(8)
    blocks = noise(rng, 11, frames)  # a ring of three partitions wraps inside the five-call fade
    a, b = rng.standard_normal((1, 5)), rng.standard_normal((2, 3 * frames - 1)) / 16
    ref, mod = ConvFadeRef(frames, a, 0.5, 0.75), DualPartitionModel(frames, 3 * frames - 1, a, 0.5, 0.75)
    for i, x in enumerate(blocks):
        if i == 2:
            ref.fade_to(b, 0.0, 1.0, 5), mod.fade_to(b, 0.0, 1.0, 5)
        if i == 8:  # and back, to the shorter IR, over one call
            ref.fade_to(a, 1.0, -0.5, 1), mod.fade_to(a, 1.0, -0.5, 1)
        assert np.abs(mod.process(x) - ref.process(x)).max() <= 1e-12, i
    assert mod.n == 0 and ref.fade_remaining() == 0
