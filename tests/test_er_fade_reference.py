"""GAS_FLAG_ER_TAP_FADE: the composed reference (er_fade_ref.py) against hand-worked cases, and the flag's ABI.

The rule (include/gas_amd.h at er_delay): a block whose effective tap row differs from the one the playback last rendered
with is  y[f] = t * Y_new[f] + (1 - t) * Y_old[f],  t = (float)f * (1 / F);  every other block is Y_new."""
import ctypes as C
import os
import re

import numpy as np

import er_fade_ref
import er_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(pairs):
    """Eight taps: the given (gain, delay) pairs, the rest gain 0 at delay 1."""
    g, d = np.zeros(8, np.float32), np.ones(8, np.uint32)
    for k, (gk, dk) in enumerate(pairs):
        g[k], d[k] = gk, dk
    return g, d


def _params(rows):
    p = np.zeros(len(rows), np.dtype([("er_gain", np.float32, 8), ("er_delay", np.uint32, 8)]))
    for i, (g, d) in enumerate(rows):
        p["er_gain"][i], p["er_delay"][i] = g, d
    return p


def _impulse(F, at):
    x = np.zeros((F, 2))
    for f in at:
        x[f] = (1.0, 2.0)
    return x


def test_one_tap_moving_under_a_unit_impulse_frame_by_frame():
    """F = 8, R = 16.  Block 0: impulse at frame 6, tap (0.5, 3), no old row -> y = x (the echo falls into block 1).
    Block 1: impulse at frame 0, tap (0.25, 5).  Over both impulses (history frames 6 and 8):
        Y_old = 1 at f 0, 0.5 at f 1 (6 + 3 = 9), 0.5 at f 3 (8 + 3 = 11)
        Y_new = 1 at f 0, 0.25 at f 3 (6 + 5 = 11), 0.25 at f 5 (8 + 5 = 13)
        y[0] = 1, y[1] = 7/8 * 0.5, y[3] = 3/8 * 0.25 + 5/8 * 0.5, y[5] = 5/8 * 0.25, the rest 0.
    Block 2: silence, the same tap: no fade, and nothing of either impulse is within 5 frames."""
    F, R = 8, 16
    src = er_fade_ref.ErFadeSource(F, R)
    y0 = src.block(*_row([(0.5, 3)]), _impulse(F, [6]))
    np.testing.assert_array_equal(y0, _impulse(F, [6]))
    y1 = src.block(*_row([(0.25, 5)]), _impulse(F, [0]))
    want = np.zeros(F)
    want[0], want[1], want[3], want[5] = 1.0, 0.4375, 0.40625, 0.15625
    np.testing.assert_array_equal(y1[:, 0], want)
    np.testing.assert_array_equal(y1[:, 1], 2.0 * want)
    y2 = src.block(*_row([(0.25, 5)]), _impulse(F, []))
    np.testing.assert_array_equal(y2, np.zeros((F, 2)))
    assert src.faded == 1


def test_unchanged_taps_are_the_unfaded_bank_exactly():
    F, R, n = 128, 256, 3
    rng = np.random.default_rng(1)
    d, g = er_ref.TapDrawer(rng, F, R).draw(n)
    p = _params(list(zip(g, d)))
    fade, plain = er_fade_ref.ErFadeBank(n, F, R), er_ref.ErBank(n, F, R)
    for _ in range(er_ref.callbacks(F, R)):
        x = rng.standard_normal((n, F, 2))
        np.testing.assert_array_equal(fade.block(p, x), plain.block(p, x))
    assert fade.faded() == [0] * n


def test_first_block_and_block_after_reset_do_not_fade():
    """A fresh playback and a reset one render their row alone: what an ErBank that is reset at the same places gives.
    The block in between, with new taps and an old row, fades."""
    F, R = 128, 256
    rng = np.random.default_rng(2)
    drawer = er_ref.TapDrawer(rng, F, R)
    fade, plain = er_fade_ref.ErFadeBank(1, F, R), er_ref.ErBank(1, F, R)
    rows = [drawer.draw(1) for _ in range(3)]
    ps = [_params([(g[0], d[0])]) for d, g in rows]
    x = rng.standard_normal((3, 1, F, 2))
    np.testing.assert_array_equal(fade.block(ps[0], x[0]), plain.block(ps[0], x[0]))
    assert not np.array_equal(fade.block(ps[1], x[1]), plain.block(ps[1], x[1]))
    fade.reset(0)
    plain.reset(0)
    np.testing.assert_array_equal(fade.block(ps[2], x[2]), plain.block(ps[2], x[2]))
    assert fade.faded() == [0]  # a new ErFadeSource: the fade of block 1 went with the old one


def test_raw_out_of_range_delay_is_its_clamped_value():
    """0xffffffff, R + 1 and R - F itself are one effective delay: republishing one for another is not a change."""
    F, R = 128, 256
    rng = np.random.default_rng(3)
    src = er_fade_ref.ErFadeSource(F, R)
    twin = er_ref.ErSource(F, R)
    for raw in (0xFFFFFFFF, R - F, R + 1, 0xFFFFFFFF):
        g, d = _row([(0.5, raw), (-0.25, 7)])
        x = rng.standard_normal((F, 2))
        np.testing.assert_array_equal(src.block(g, d, x), twin.block(g, d, x))
    assert src.faded == 0
    assert er_fade_ref.same_row(er_fade_ref.effective_row(*_row([(0.5, 0xFFFFFFFF)]), F, R), er_fade_ref.effective_row(*_row([(0.5, R - F)]), F, R))
    assert not er_fade_ref.same_row(er_fade_ref.effective_row(*_row([(0.0, 1)]), F, R), er_fade_ref.effective_row(*_row([(-0.0, 1)]), F, R))


def test_dc_is_continuous_across_the_fade():
    """x = 1, all eight gains 0.1 -> 0.5 at delays 1 .. 8.  Faded: no step anywhere, the boundaries included, exceeds
    sum|dg| / F (the lerp's slope; 1e-12 for the float64 sums).  Unfaded: one step of sum|dg| = 3.2 at the boundary."""
    F, R = 128, 256
    lo, hi = np.full(8, 0.1, np.float32), np.full(8, 0.5, np.float32)
    d = np.arange(1, 9, dtype=np.uint32)
    total = float(np.abs(hi.astype(np.float64) - lo.astype(np.float64)).sum())
    assert abs(total - 3.2) < 1e-6
    x = np.ones((1, F, 2))
    plan = [lo, lo, hi, hi]
    fade, plain = er_fade_ref.ErFadeBank(1, F, R), er_ref.ErBank(1, F, R)
    yf = np.concatenate([fade.block(_params([(g, d)]), x)[0] for g in plan])
    yp = np.concatenate([plain.block(_params([(g, d)]), x)[0] for g in plan])
    steps_f, steps_p = np.abs(np.diff(yf[F:, 0])), np.abs(np.diff(yp[F:, 0]))  # from block 1 on: every tap reads ones
    assert steps_f.max() <= total / F + 1e-12
    assert steps_f[F - 1] <= total / F + 1e-12 and steps_f[2 * F - 1] <= total / F + 1e-12  # into and out of the fade block
    assert abs(steps_p[F - 1] - total) < 1e-12 and steps_p.max() == steps_p[F - 1]
    assert fade.faded() == [1]


def test_flag_value_in_capi_and_header():
    import godot_audio_spatializer_amd as gas

    assert gas.capi.FLAG_ER_TAP_FADE == 512
    hdr = open(os.path.join(ROOT, "include", "gas_amd.h")).read()
    assert re.search(r"^#define GAS_FLAG_ER_TAP_FADE 512u$", hdr, re.M)
    assert re.search(r"^#define GAS_ABI_VERSION 2\b", hdr, re.M)


def test_flag_without_a_ring_is_rejected_before_touching_a_device(gas):
    lib = gas.load_library()
    h = C.c_void_p()
    cfg = gas.capi.Config(C.sizeof(gas.capi.Config), 0, 16, 512, 1, 48000.0, 0, gas.capi.FLAG_ER_TAP_FADE)
    assert lib.gas_ctx_create(C.byref(cfg), C.byref(h)) == -1  # GAS_ERR_INVALID_ARGUMENT, with or without a device
    assert not h.value
