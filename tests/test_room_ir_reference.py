"""tests/room_ir_ref.py, the float64 statement of gas_conv_ir_from_room's rule, against cases that can be checked by
hand, against tests/er_rooms_ref.py (the two share levels and times) and against the properties the header promises:
additivity over orders, continuity at the ends of the tap range, what a dead wall removes, the size of the box.  No GPU.

The 1-D case is test_er_rooms_reference.py's: half_extent (5, 5, 5), source (1, 0, 0), listener (-2, 0, 0), d0 = 3,
c = 480 m/s at 48 kHz = 100 frames per metre.  The image m = (1, 0, 0) lies at x = 9: dist 11, pos exactly 800."""
import numpy as np
import pytest

import er_rooms_ref as E
import room_ir_ref as R

RATE = 48000.0


def rel_change(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b**2))


def small_room():
    room = E.unit_room(half_extent=(2.5, 2.0, 1.5))
    room["reflectance"] = [[0.9, 0.85, 0.8, 0.75, 0.7, 0.95]]
    return room


def test_direct_sound_alone_is_the_level_exactly():
    room = small_room()
    room["level"] = 0.7
    d = R.describe(room, (1.0, 0.5, 0.25), (-1.0, 0.25, -0.5))
    out = R.ir(d, 1, 300, RATE, orders=(0, 0))
    assert out.candidates == 1
    assert out.acc[0, 0] == 1 << 32 and not out.acc[0, 1:].any()
    assert out.h[0, 0] == np.float32(0.7) and not out.h[0, 1:].any()


@pytest.mark.parametrize("seed", range(3))
def test_levels_and_times_are_early_reflections(seed):
    """One channel, orders 1 .. 2: the candidates are ER's 24, pos is its fr and v level its g."""
    rng = np.random.default_rng(seed)
    room = E.unit_room(level=0.75)
    room["reflectance"] = rng.uniform(0.3, 0.95, (1, 6))
    h = room["half_extent"][0].astype(np.float64)
    src, lis = (rng.uniform(-0.9, 0.9, 3) * h).astype(np.float32), (rng.uniform(-0.9, 0.9, 3) * h).astype(np.float32)
    er = E.taps(room, [src], lis, RATE, 512, 1 << 16)
    out = R.ir(R.describe(room, src, lis, min_order=1, max_order=2), 1, 4096, RATE)
    assert out.candidates == 24
    by_m = {tuple(m): i for i, m in enumerate(out.m.tolist())}
    checked = 0
    for cand, m in enumerate(E.TRIPLES):
        i = by_m[m]
        if er.g_all[0, cand] <= 0 or E.frac_border(er.fr_all[0, cand]) or er.fr_all[0, cand] < 1.0:
            continue
        assert np.rint(out.pos[0][i]) == er.delay_all[0, cand]
        assert abs(out.v[0][i] * 0.75 - er.g_all[0, cand]) <= E.GAIN_RTOL * er.g_all[0, cand]
        checked += 1
    assert checked >= 20


def test_orders_add_up_exactly():
    """[0, 2] + [3, inf) == [0, inf) in the int64 domain: what ER plays and a tail with min_order = 3 are one room."""
    d = R.describe(small_room(), (1.0, 0.5, 0.25), (-1.0, 0.25, -0.5), ear_spacing=0.18)
    whole = R.ir(d, 2, 3000, RATE)
    early = R.ir(d, 2, 3000, RATE, orders=(0, 2))
    tail = R.ir(d, 2, 3000, RATE, orders=(3, None))
    assert early.candidates == 25 and early.candidates + tail.candidates == whole.candidates
    assert tail.acc.any() and np.array_equal(early.acc + tail.acc, whole.acc)
    d["min_order"] = 3  # the descriptor's own mask is the same thing
    assert np.array_equal(R.ir(d, 2, 3000, RATE).acc, tail.acc)


def one_d(taps, channels=1, **kw):
    room = E.unit_room(half_extent=(5, 5, 5), c=480.0)
    return R.describe(room, (1.0, 0.0, 0.0), (-2.0, 0.0, 0.0), **kw), channels, taps


@pytest.mark.parametrize("taps", [800, 801])
def test_continuous_at_the_last_tap(taps):
    """m = (1, 0, 0) has pos = 800 - 200 dx for a source moved by dx: at 801 taps it crosses from tap 799 / 800 to tap
    800 / (801, dropped), at 800 taps from tap 799 / (800, dropped) to nothing."""
    d, ch, taps = one_d(taps)
    a, b = (R.ir(d, ch, taps, RATE, nudge=(dx, 0, 0)) for dx in (-1e-9, 1e-9))
    i = a.m.tolist().index([1, 0, 0])
    assert a.pos[0][i] > 800.0 > b.pos[0][i]  # the step does cross the border
    assert rel_change(a.h, b.h) < 1e-6
    assert rel_change(a.h, R.ir(d, ch, taps, RATE).h) < 1e-6


def test_continuous_at_tap_zero():
    """Ears 0.25 m apart and the source 0.0625 m to the left of the median plane: the left ear is exactly as far from the
    source as the head's centre, so its direct sound has pos = 0 and a step of the source moves it across k = -1 / k = 0."""
    room = E.unit_room()
    d = R.describe(room, (-0.0625, 2.0, 0.0), (0.0, 0.0, 0.0), ear_spacing=0.25)
    a, b = (R.ir(d, 2, 2000, RATE, nudge=(dx, 0, 0)) for dx in (-1e-9, 1e-9))
    i = a.m.tolist().index([0, 0, 0])
    assert a.pos[0][i] < 0.0 < b.pos[0][i]
    assert a.h[0, 0] > 0.99 and b.h[0, 0] > 0.99  # an image with k = -1 still feeds tap 0
    assert rel_change(a.h, b.h) < 1e-6


def test_a_dead_wall_removes_the_images_that_touch_it():
    """+x with reflectance 0: a path with m_x >= 1 or m_x <= -2 meets it, one with m_x in {-1, 0} does not."""
    room = small_room()
    src, lis = (1.0, 0.5, 0.25), (-1.0, 0.25, -0.5)
    alive = R.ir(R.describe(room, src, lis), 1, 3000, RATE, keep=lambda mx, my, mz: (mx == 0) | (mx == -1))
    room["reflectance"][0, 1] = 0.0
    dead = R.ir(R.describe(room, src, lis), 1, 3000, RATE)
    assert alive.candidates < dead.candidates and alive.acc.any()
    assert np.array_equal(dead.acc, alive.acc)


def test_the_box_and_its_cap():
    """unit_room is 8 x 5 x 6 m; 48 000 taps at 48 kHz and 343 m/s with d0 = 3: reach = 346 m."""
    d = R.describe(E.unit_room(), (1.0, 0.0, 0.0), (-2.0, 0.0, 0.0))
    assert R.box(d, 1, 48000, RATE) == ([44, 70, 58], 89 * 141 * 117)
    d["ear_spacing"] = 8.0  # two channels reach half the ear spacing further: 350 m
    assert R.box(d, 2, 48000, RATE)[0] == [44, 71, 59]
    assert R.box(d, 1, 48000, RATE)[0] == [44, 70, 58]
    d["max_order"] = 50
    assert R.box(d, 1, 48000, RATE) == ([44, 50, 50], 89 * 101 * 101)
    # the cap: a 1 m cube at 2^20 taps has N = 7494 per axis
    cube = R.describe(E.unit_room(half_extent=(0.5, 0.5, 0.5)), (0.25, 0.0, 0.0), (-0.25, 0.0, 0.0))
    n, cells = R.box(cube, 1, 1 << 20, RATE)
    assert n == [7494] * 3 and cells > R.MAX_CELLS
    cube["max_order"] = 322  # 645^3 = 268 336 125 <= 2^28 = 268 435 456 < 647^3
    assert R.box(cube, 1, 1 << 20, RATE)[1] == 645**3 <= R.MAX_CELLS
    cube["max_order"] = 323
    assert R.box(cube, 1, 1 << 20, RATE)[1] > R.MAX_CELLS


def test_the_largest_shape_of_the_gpu_tests():
    d = R.describe(small_room(), (1.0, 0.5, 0.25), (-1.0, 0.25, -0.5), ear_spacing=0.18)
    out = R.ir(d, 2, 16384, RATE)
    assert out.N == [24, 30, 40] and out.cells == 49 * 61 * 81 and out.candidates == out.cells
    assert 100_000 < out.in_range < 140_000
    assert out.acc.max() < 1 << 61 and np.isfinite(out.h).all()
