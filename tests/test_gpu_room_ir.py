"""gas_conv_ir_from_room on the GPU: k_room_ir against tests/room_ir_ref.py (float64, int64 sums), what is bitwise, the
generated IR in the convolver calls, and the refusals.

Tolerance: helpers.TOL (1e-5), as relative RMS per channel and as max-abs relative to max|h|.  Device and reference
quantise the same float64 shares to integers, so the expected error is float32's final rounding or nothing at all; every
comparison prints its figures (and whether the taps are equal to the bit) before it asserts.  Measured on an MI355X:
0 and 0 on every shape, every channel equal to the bit (profiles/room_ir_notes.md).  Each reference is computed once
per shape and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import er_rooms_ref as E
import room_ir_ref as R
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

RATE = 48000.0
F = 128
SRC, LIS = (1.0, 0.5, 0.25), (-1.0, 0.25, -0.5)
WORST = [0.0, 0.0]


def small_room(refl=(0.9, 0.85, 0.8, 0.75, 0.7, 0.95), level=1.0):
    room = E.unit_room(half_extent=(2.5, 2.0, 1.5), level=level)
    room["reflectance"] = [list(refl)]
    return room


def rotated():
    """A rotated room off the origin, a listener turned another way, six different reflectances."""
    rng = np.random.default_rng(7)
    room = small_room(level=0.8)
    B = E.random_basis(rng)
    origin = np.array([3.0, -7.0, 11.0])
    room["basis"], room["origin"] = B, origin
    return R.describe(room, origin + B @ np.array(SRC), origin + B @ np.array(LIS), listener_basis=E.random_basis(rng), ear_spacing=0.18)


CASES = {
    "2000 taps, one channel": lambda: (R.describe(small_room(), SRC, LIS), 1, 2000),
    "2048 taps, two channels": lambda: (R.describe(small_room(), SRC, LIS, ear_spacing=0.18), 2, 2048),
    "16384 taps, two channels, rotated": lambda: (rotated(), 2, 16384),
    "max_order 3 inside a larger box": lambda: (R.describe(small_room(), SRC, LIS, ear_spacing=0.18, max_order=3), 2, 2000),
    "min_order 3": lambda: (R.describe(small_room(), SRC, LIS, ear_spacing=0.18, min_order=3), 2, 2000),
    "rigid room": lambda: (R.describe(small_room(refl=(1,) * 6), SRC, LIS), 1, 2000),
    "one dead wall": lambda: (R.describe(small_room(refl=(0.9, 0.85, 0.0, 0.75, 0.7, 0.95)), SRC, LIS, ear_spacing=0.18), 2, 2000),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    d, channels, taps = CASES[name]()
    out = R.ir(d, channels, taps, RATE)
    out.h.setflags(write=False)
    return d, channels, taps, out


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw(ctx, desc, channels, taps, out_taps, want_ir, sentinel=0xDEADBEEF):
    """The call itself -> (status, *out_ir): out_ir keeps the sentinel where the library does not write it."""
    out = C.c_uint32(sentinel)
    d = None if desc is None else np.ascontiguousarray(desc)
    rc = ctx.lib.gas_conv_ir_from_room(ctx.h, ptr(d), channels, taps, ptr(out_taps), C.byref(out) if want_ir else None)
    return rc, out.value


@pytest.mark.parametrize("name", list(CASES))
def test_parity(gas, name):
    d, channels, taps, ref = reference(name)
    if name.startswith("max_order 3"):
        assert ref.cells == 7**3 > ref.candidates  # the order mask cuts the box's corners
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        h = ctx.conv_ir_from_room(d, channels, taps, want_taps=True, load=False)
    assert h.shape == (channels, taps) and h.dtype == np.float32 and ref.h.any()
    for e in range(channels):
        rms = rel_rms(h[e], ref.h[e])
        mx = np.abs(h[e].astype(np.float64) - ref.h[e]).max() / np.abs(ref.h[e]).max()
        WORST[0], WORST[1] = max(WORST[0], rms), max(WORST[1], mx)
        print(f"{name} ch {e}: rel rms {rms:.3g}, max abs / max|h| {mx:.3g}, bitwise {np.array_equal(h[e], ref.h[e])} (worst so far {WORST[0]:.3g}, {WORST[1]:.3g})")
        assert rms <= TOL and mx <= TOL, (name, e, rms, mx)


def test_direct_sound_is_the_level_exactly(gas):
    """Every wall dead: only m = 0 has R > 0.  h[0] == level to the bit and nothing else."""
    d = R.describe(small_room(refl=(0,) * 6, level=0.7), SRC, LIS)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        h = ctx.conv_ir_from_room(d, 1, 2000, want_taps=True, load=False)
    assert h[0, 0].tobytes() == np.float32(0.7).tobytes()
    assert not h[0, 1:].any()
    assert np.array_equal(h, R.ir(d, 1, 2000, RATE, orders=(0, 0)).h)


def test_two_calls_give_the_same_bits(gas):
    d, channels, taps, _ = reference("2048 taps, two channels")
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        a = ctx.conv_ir_from_room(d, channels, taps, want_taps=True, load=False)
        b = ctx.conv_ir_from_room(d, channels, taps, want_taps=True, load=False)
        d2 = d.copy()
        d2["room"]["max_order"] = 77  # not read here
        c = ctx.conv_ir_from_room(d2, channels, taps, want_taps=True, load=False)
    assert a.any() and a.tobytes() == b.tobytes() == c.tobytes()


def test_registered_ir_is_the_loaded_one_bitwise(gas):
    """3 F + 40 taps: four partitions, the last a partial one; four blocks of noise reach every partition."""
    taps = 3 * F + 40
    d = R.describe(small_room(), SRC, LIS, ear_spacing=0.18)
    rng = np.random.default_rng(11)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 4 * F)
        made, h = ctx.conv_ir_from_room(d, 2, taps, want_taps=True)
        assert ctx.conv_ir_get_info(made) == (2, taps)
        loaded = ctx.conv_ir_load(h)
        assert (made, loaded) == (0, 1)
        convs = [ctx.conv_create(made), ctx.conv_create(loaded)]
        for _ in range(4):
            x = rng.uniform(-1, 1, (1, F, 2)).astype(np.float32)
            y = ctx.conv_process(convs, np.concatenate([x, x]))
            assert y[0].any() and y[0].tobytes() == y[1].tobytes()
        for k in convs:
            ctx.conv_destroy(k)
        ctx.conv_ir_free(made)
        assert ctx.conv_ir_from_room(d, 1, taps) == 0  # the lowest free id, as gas_conv_ir_load gives


def test_generated_ir_as_the_target_of_a_fade(gas):
    """State B of gas_conv_fade_to; once the fade has ended the instance is bitwise a twin that was switched hard.
    The tail (min_order = 3) of this room begins at tap 603 -- the third-order images are that much further than the
    direct sound -- so 5 F + 17 taps hold some of it and the output is the tail's from the fifth block on."""
    taps = 5 * F + 17
    rng = np.random.default_rng(12)
    dry_room = (rng.standard_normal((2, 50)) * 0.1).astype(np.float32)
    d = R.describe(small_room(), SRC, LIS, ear_spacing=0.18, min_order=3)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 6 * F)
        a = ctx.conv_ir_load(dry_room)
        b, tail = ctx.conv_ir_from_room(d, 2, taps, want_taps=True)
        assert ctx.conv_ir_get_info(b) == (2, taps)
        first = [int(np.nonzero(tail[e])[0][0]) for e in range(2)]
        assert 4 * F < min(first) and max(first) < 5 * F, first
        fading, twin = ctx.conv_create(a), ctx.conv_create(a)
        ctx.conv_fade_to(fading, b, 0.0, 1.0, 2)
        for block in range(7):
            if block == 2:
                assert ctx.conv_fade_remaining(fading) == 0
                ctx.conv_set_ir(twin, b)
            x = rng.uniform(-1, 1, (1, F, 2)).astype(np.float32)
            y = ctx.conv_process([fading, twin], np.concatenate([x, x]))
            if block == 1:
                assert y[0].tobytes() != y[1].tobytes()  # half way: A and B mixed against A alone
            if block >= 2:
                assert y[0].tobytes() == y[1].tobytes()
            if block >= 5:  # frames 640 ..: every one of them hears taps 603 .. of both ears
                assert y[0][:, 0].any() and y[0][:, 1].any()


def test_pure_generator_needs_no_reserve(gas):
    d, channels, taps, ref = reference("2000 taps, one channel")
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        h = ctx.conv_ir_from_room(d, channels, taps, want_taps=True, load=False)
        assert rel_rms(h, ref.h) <= TOL
        buf = np.full((channels, taps), np.nan, np.float32)
        assert raw(ctx, d, channels, taps, buf, True) == (-6, 0xDEADBEEF)  # GAS_ERR_UNSUPPORTED_CHAIN
        assert raw(ctx, d, channels, taps, None, True) == (-6, 0xDEADBEEF)
        assert np.isnan(buf).all()


def refusals():
    """(what, descriptor, channels, taps, with out_taps, with out_ir) under a reserve of 4096 taps."""
    ok = R.describe(small_room(), SRC, LIS, ear_spacing=0.18)

    def room(**kw):
        d = ok.copy()
        for k, v in kw.items():
            d["room"][k] = v
        return d

    def desc(**kw):
        d = ok.copy()
        for k, v in kw.items():
            d[k] = v
        return d

    def listener(**kw):
        d = ok.copy()
        for k, v in kw.items():
            d["listener"][k] = v
        return d

    nan_basis = np.eye(3, dtype=np.float32)
    nan_basis[1, 2] = np.nan
    cube = R.describe(E.unit_room(half_extent=(0.5, 0.5, 0.5)), (0.25, 0.0, 0.0), (-0.25, 0.0, 0.0))
    cube323 = cube.copy()
    cube323["max_order"] = 323
    yield "NULL descriptor", None, 2, 256, True, True
    yield "neither output", ok, 2, 256, False, False
    for ch in (0, 3, 4):
        yield f"channels {ch}", ok, ch, 256, True, True
    yield "no taps", ok, 2, 0, True, True
    yield "more taps than the reserve", ok, 1, 4097, True, True
    yield "more taps than 2^20 for the pure generator", ok, 1, (1 << 20) + 1, True, False
    yield "half extent 0", room(half_extent=(2.5, 0.0, 1.5)), 2, 256, True, True
    yield "half extent inf", room(half_extent=(2.5, np.inf, 1.5)), 2, 256, True, True
    yield "speed of sound 0", room(speed_of_sound=0.0), 2, 256, True, True
    yield "level < 0", room(level=-0.5), 2, 256, True, True
    yield "level inf", room(level=np.inf), 2, 256, True, True
    yield "reflectance > 1", room(reflectance=(0.9, 1.5, 0.8, 0.8, 0.8, 0.8)), 2, 256, True, True
    yield "reflectance nan", room(reflectance=(0.9, np.nan, 0.8, 0.8, 0.8, 0.8)), 2, 256, True, True
    yield "min_order > max_order", desc(min_order=4, max_order=3), 2, 256, True, True
    yield "ear spacing < 0", desc(ear_spacing=-0.1), 2, 256, True, True
    yield "ear spacing nan", desc(ear_spacing=np.nan), 1, 256, True, True
    yield "ear spacing inf", desc(ear_spacing=np.inf), 2, 256, True, True
    yield "source nan", desc(source=(1.0, np.nan, 0.25)), 2, 256, True, True
    yield "listener origin inf", listener(origin=(np.inf, 0.0, 0.0)), 2, 256, True, True
    yield "listener basis nan", listener(basis=nan_basis), 2, 256, True, True
    yield "room basis nan", room(basis=nan_basis), 2, 256, True, True
    yield "room origin nan", room(origin=(0.0, 0.0, np.nan)), 2, 256, True, True
    yield "source outside", desc(source=(2.6, 0.5, 0.25)), 2, 256, True, True
    yield "listener outside", listener(origin=(-1.0, 0.25, -1.6)), 2, 256, True, True
    yield "source at the listener", desc(source=LIS), 2, 256, True, True
    yield "d0 below a millimetre", desc(source=(LIS[0] + 5e-4, LIS[1], LIS[2])), 2, 256, True, True
    yield "box over the cap", cube, 1, 1 << 20, True, False
    yield "box over the cap with a max_order", cube323, 1, 1 << 20, True, False


def test_refusals_change_nothing(gas):
    ok = R.describe(small_room(), SRC, LIS, ear_spacing=0.18)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 4096)
        first = ctx.conv_ir_from_room(ok, 2, 256)
        assert first == 0
        for what, d, channels, taps, with_taps, with_ir in refusals():
            buf = np.full((max(channels, 1), max(taps, 1)), np.nan, np.float32) if with_taps else None
            rc, ir = raw(ctx, d, channels, taps, buf, with_ir)
            assert rc == -1, (what, rc)
            assert ir == 0xDEADBEEF, what
            assert buf is None or np.isnan(buf).all(), what
        assert ctx.lib.gas_conv_ir_from_room(None, ptr(np.ascontiguousarray(ok)), 2, 256, None, C.byref(C.c_uint32())) == -1
        assert ctx.conv_ir_load(np.ones((1, 4), np.float32)) == 1  # the id it would have had: the table is as it was
        assert ctx.conv_ir_get_info(first) == (2, 256)
        with pytest.raises(gas.capi.GasError) as ei:
            ctx.conv_ir_get_info(2)
        assert ei.value.status == -3
