"""gas_conv_ir_from_planes on the GPU: k_room_planes against tests/room_planes_ref.py (float64, int64 sums), the box as
six planes against gas_conv_ir_from_room on the same device, reciprocity, what is bitwise, the generated IR in the
convolver calls, and the refusals.

Tolerance: helpers.TOL (1e-5), as relative RMS per channel and as max-abs relative to max|h| -- the bar of every generated
IR.  Device and reference quantise the same float64 shares to integers, so the expected error is float32's final rounding
or nothing at all; what could differ is a face test of step 4 that lands on another side of 0, which drops or doubles a
whole image.  Every case therefore asserts that the reference met no face test nearer than 1e-9 m to a face (float64
carries these coordinates to about 1e-15 m) and that its weakest image has v >= 1e-3, a hundred times the bar, so such a
flip cannot pass.  Every comparison prints its figures (and whether the taps are equal to the bit) before it asserts.
Measured on an MI355X: 0 and 0 on every case, every channel equal to the bit (profiles/room_planes_notes.md).  Each
reference is computed once per case and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import er_rooms_ref as E
import room_ir_ref as R
import room_planes_ref as P
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

RATE = 48000.0
F = 128
SRC, LIS = (1.1, 1.2, 0.5), (-0.9, 1.45, -0.8)
BOX_ORIGIN = np.array([3.0, -7.0, 11.0])
BOX_HALF = (2.5, 2.0, 1.5)
BOX_REFL = (0.9, 0.85, 0.8, 0.75, 0.7, 0.95)
BOX_SRC, BOX_LIS = BOX_ORIGIN + (1.0, 0.5, 0.25), BOX_ORIGIN + (-1.0, 0.25, -0.5)
PARALLEL = [((1, 0, 0), -2.0, 0.9), ((-1, 0, 0), -2.5, 0.8)]
GROUND = [((0, 1, 0), 0.0, 0.6)]


def sixteen_planes():
    """A floor, a ceiling at 3.2 m and fourteen walls at uneven angles and distances of 3.5 to 4.5 m."""
    rng = np.random.default_rng(0)
    rows = [((0, 1, 0), 0.0, 0.8), ((0, -1, 0), -3.2, 0.8)]
    for i in range(14):
        th = 2 * np.pi * (i + rng.uniform(-0.2, 0.2)) / 14
        ap = rng.uniform(3.5, 4.5)
        rows.append(((-np.cos(th), 0.0, -np.sin(th)), -ap, 0.7 + 0.02 * (i % 10)))
    return rows


# name -> (descriptor, channels, taps, candidates)
CASES = {
    "attic, orders <= 3, one channel": lambda: (P.describe(P.attic(), SRC, LIS, max_order=3), 1, 4000, 301),
    "attic, orders <= 4, two channels": lambda: (P.describe(P.attic(), SRC, LIS, ear_spacing=0.18, max_order=4), 2, 4000, 1813),
    "attic, min_order 3": lambda: (P.describe(P.attic(), SRC, LIS, ear_spacing=0.18, min_order=3, max_order=4), 2, 4000, 1764),
    "attic, one reflectance 0": lambda: (P.describe(P.attic(dead=5), SRC, LIS, ear_spacing=0.18, max_order=4), 2, 4000, 1813),
    "two parallel planes, order 8": lambda: (P.describe(PARALLEL, (0.5, 0.2, 0.1), (-0.7, 0.0, 0.3), ear_spacing=0.18, max_order=8), 2, 4000, 16),
    "one plane": lambda: (P.describe(GROUND, (2.0, 1.5, 0.0), (-2.0, 1.7, 0.5), ear_spacing=0.18, max_order=8), 2, 1000, 1),
    "16 planes, orders <= 2": lambda: (P.describe(sixteen_planes(), SRC, LIS, ear_spacing=0.18, max_order=2), 2, 4000, 256),
    "16 planes, orders <= 3": lambda: (P.describe(sixteen_planes(), SRC, LIS, ear_spacing=0.18, max_order=3), 2, 4000, 3856),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    d, channels, taps, candidates = CASES[name]()
    out = P.ir(d, channels, taps, RATE)
    out.h.setflags(write=False)
    assert out.candidates == candidates
    return d, channels, taps, out


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw(ctx, desc, channels, taps, out_taps, want_ir, sentinel=0xDEADBEEF):
    """The call itself -> (status, *out_ir): out_ir keeps the sentinel where the library does not write it."""
    out = C.c_uint32(sentinel)
    d = None if desc is None else np.ascontiguousarray(desc)
    rc = ctx.lib.gas_conv_ir_from_planes(ctx.h, ptr(d), channels, taps, ptr(out_taps), C.byref(out) if want_ir else None)
    return rc, out.value


def compare(what, h, want):
    """Prints the two figures and the bitwise result per channel, then asserts the bar."""
    assert h.shape == want.shape and h.dtype == np.float32 and want.any()
    for e in range(h.shape[0]):
        rms = rel_rms(h[e], want[e])
        mx = np.abs(h[e].astype(np.float64) - want[e]).max() / np.abs(want[e]).max()
        print(f"{what} ch {e}: rel rms {rms:.3g}, max abs / max|h| {mx:.3g}, bitwise {np.array_equal(h[e], want[e])}")
        assert rms <= TOL and mx <= TOL, (what, e, rms, mx)


@pytest.mark.parametrize("name", list(CASES))
def test_parity(gas, name):
    d, channels, taps, ref = reference(name)
    print(f"{name}: {ref.candidates} candidates, {ref.void} void, valid {ref.valid}, margin {ref.margin:.3g} m, smallest v {ref.v_min:.3g}")
    assert ref.margin >= 1e-9 and ref.v_min >= 1e-3
    assert all(v > 0 for v in ref.valid)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        h = ctx.conv_ir_from_planes(d, channels, taps, want_taps=True, load=False)
    compare(name, h, ref.h)


def test_a_box_as_six_planes_is_the_box_call(gas):
    """The same device, both roads: six planes from capi.planes_from_box against gas_conv_ir_from_room."""
    room = E.unit_room(half_extent=BOX_HALF)
    room["reflectance"] = [list(BOX_REFL)]
    room["origin"] = BOX_ORIGIN
    K = gas.capi
    planes = K.planes_from_box(room)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        for channels, max_order in ((1, 3), (2, 4)):
            box = ctx.conv_ir_from_room(R.describe(room, BOX_SRC, BOX_LIS, ear_spacing=0.18, max_order=max_order), channels, 2000, want_taps=True, load=False)
            six = ctx.conv_ir_from_planes(K.default_room_planes(planes=planes, source=BOX_SRC, listener_origin=BOX_LIS, ear_spacing=0.18, max_order=max_order), channels, 2000, want_taps=True, load=False)
            compare(f"box as six planes, max_order {max_order}", six, box)


def test_reciprocity(gas):
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        fwd = ctx.conv_ir_from_planes(P.describe(P.attic(), SRC, LIS, max_order=4), 1, 4000, want_taps=True, load=False)
        back = ctx.conv_ir_from_planes(P.describe(P.attic(), LIS, SRC, max_order=4), 1, 4000, want_taps=True, load=False)
    compare("source and listener swapped", back, fwd)


def test_two_calls_give_the_same_bits(gas):
    d, channels, taps, _ = reference("16 planes, orders <= 3")
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        a = ctx.conv_ir_from_planes(d, channels, taps, want_taps=True, load=False)
        b = ctx.conv_ir_from_planes(d, channels, taps, want_taps=True, load=False)
        d2 = d.copy()
        d2["listener"]["velocity"] = 9.0  # not read
        d2["listener"]["basis"][0][:, 1:] = np.nan  # not read: column 0 alone is
        c = ctx.conv_ir_from_planes(d2, channels, taps, want_taps=True, load=False)
    assert a.any() and a.tobytes() == b.tobytes() == c.tobytes()


def test_planes_beyond_n_planes_are_not_read(gas):
    d, channels, taps, _ = reference("attic, orders <= 3, one channel")
    d2 = d.copy()
    d2["planes"]["normal"][0, 7:] = np.nan
    d2["planes"]["reflectance"][0, 7:] = 5.0
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        a = ctx.conv_ir_from_planes(d, channels, taps, want_taps=True, load=False)
        b = ctx.conv_ir_from_planes(d2, channels, taps, want_taps=True, load=False)
    assert a.any() and a.tobytes() == b.tobytes()


def test_registered_ir_is_the_loaded_one_bitwise(gas):
    """3 F + 40 taps: four partitions, the last a partial one; four blocks of noise reach every partition."""
    taps = 3 * F + 40
    d = P.describe(P.attic(), SRC, LIS, ear_spacing=0.18, max_order=3)
    rng = np.random.default_rng(11)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 4 * F)
        made, h = ctx.conv_ir_from_planes(d, 2, taps, want_taps=True)
        assert ctx.conv_ir_get_info(made) == (2, taps) and np.count_nonzero(h) > 4
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
        assert ctx.conv_ir_from_planes(d, 1, taps) == 0  # the lowest free id, as gas_conv_ir_load gives


def test_generated_ir_as_the_target_of_a_fade(gas):
    """State B of gas_conv_fade_to; once the fade has ended the instance is bitwise a twin that was switched hard."""
    taps = 5 * F + 17
    rng = np.random.default_rng(12)
    dry_room = (rng.standard_normal((2, 50)) * 0.1).astype(np.float32)
    d = P.describe(P.attic(), SRC, LIS, ear_spacing=0.18, max_order=3)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 6 * F)
        a = ctx.conv_ir_load(dry_room)
        b, h = ctx.conv_ir_from_planes(d, 2, taps, want_taps=True)
        assert ctx.conv_ir_get_info(b) == (2, taps) and h[0].any() and h[1].any()
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
                assert y[0].any() and y[0].tobytes() == y[1].tobytes()


def test_pure_generator_needs_no_reserve(gas):
    d, channels, taps, ref = reference("attic, orders <= 3, one channel")
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        h = ctx.conv_ir_from_planes(d, channels, taps, want_taps=True, load=False)
        assert rel_rms(h, ref.h) <= TOL
        buf = np.full((channels, taps), np.nan, np.float32)
        assert raw(ctx, d, channels, taps, buf, True) == (-6, 0xDEADBEEF)  # GAS_ERR_UNSUPPORTED_CHAIN
        assert raw(ctx, d, channels, taps, None, True) == (-6, 0xDEADBEEF)
        assert np.isnan(buf).all()


def refusals():
    """(what, descriptor, channels, taps, with out_taps, with out_ir) under a reserve of 4096 taps."""
    ok = P.describe(P.attic(), SRC, LIS, ear_spacing=0.18, max_order=3)

    def desc(**kw):
        d = ok.copy()
        for k, v in kw.items():
            d[k] = v
        return d

    def plane(j, **kw):
        d = ok.copy()
        for k, v in kw.items():
            d["planes"][k][0, j] = v
        return d

    def listener(**kw):
        d = ok.copy()
        for k, v in kw.items():
            d["listener"][k] = v
        return d

    nan_basis = np.eye(3, dtype=np.float32)
    nan_basis[1, 0] = np.nan
    yield "NULL descriptor", None, 2, 256, True, True
    yield "neither output", ok, 2, 256, False, False
    for ch in (0, 3, 4):
        yield f"channels {ch}", ok, ch, 256, True, True
    yield "no taps", ok, 2, 0, True, True
    yield "more taps than the reserve", ok, 1, 4097, True, True
    yield "more taps than 2^20 for the pure generator", ok, 1, (1 << 20) + 1, True, False
    yield "no planes", desc(n_planes=0), 2, 256, True, True
    yield "17 planes", desc(n_planes=17), 2, 256, True, True
    yield "max_order 0", desc(max_order=0), 2, 256, True, True
    yield "max_order 9", desc(max_order=9), 2, 256, True, True
    yield "min_order > max_order", desc(min_order=4, max_order=3), 2, 256, True, True
    yield "normal nan", plane(2, normal=(np.nan, 0.0, 0.0)), 2, 256, True, True
    yield "normal inf", plane(6, normal=(0.0, np.inf, 0.0)), 2, 256, True, True
    yield "offset nan", plane(0, offset=np.nan), 2, 256, True, True
    yield "offset -inf", plane(0, offset=-np.inf), 2, 256, True, True
    yield "normal too short", plane(1, normal=(0.998, 0.0, 0.0)), 2, 256, True, True
    yield "normal too long", plane(1, normal=(1.002, 0.0, 0.0)), 2, 256, True, True
    yield "normal 0", plane(3, normal=(0.0, 0.0, 0.0)), 2, 256, True, True
    yield "reflectance > 1", plane(4, reflectance=1.5), 2, 256, True, True
    yield "reflectance < 0", plane(4, reflectance=-0.1), 2, 256, True, True
    yield "reflectance nan", plane(6, reflectance=np.nan), 2, 256, True, True
    yield "speed of sound 0", desc(speed_of_sound=0.0), 2, 256, True, True
    yield "speed of sound < 0", desc(speed_of_sound=-343.0), 2, 256, True, True
    yield "speed of sound inf", desc(speed_of_sound=np.inf), 2, 256, True, True
    yield "level < 0", desc(level=-0.5), 2, 256, True, True
    yield "level inf", desc(level=np.inf), 2, 256, True, True
    yield "ear spacing < 0", desc(ear_spacing=-0.1), 2, 256, True, True
    yield "ear spacing nan, one channel", desc(ear_spacing=np.nan), 1, 256, True, True
    yield "ear spacing inf", desc(ear_spacing=np.inf), 2, 256, True, True
    yield "source nan", desc(source=(1.0, np.nan, 0.25)), 2, 256, True, True
    yield "listener origin inf", listener(origin=(np.inf, 0.0, 0.0)), 2, 256, True, True
    yield "listener basis column 0 nan", listener(basis=nan_basis), 2, 256, True, True
    yield "source under the floor", desc(source=(1.1, -0.1, 0.5)), 2, 256, True, True
    yield "source on the floor", desc(source=(1.1, 0.0, 0.5)), 2, 256, True, True
    yield "source above the roof", desc(source=(2.5, 2.2, 0.5)), 2, 256, True, True
    yield "listener outside", listener(origin=(-0.9, 1.45, -4.1)), 2, 256, True, True
    yield "one ear outside", listener(origin=(-2.95, 1.0, -0.8)), 2, 256, True, True
    yield "source at the listener", desc(source=LIS), 2, 256, True, True
    yield "d0 below a millimetre", desc(source=(LIS[0] + 5e-4, LIS[1], LIS[2])), 2, 256, True, True
    yield "more than 2^28 candidates", P.describe(sixteen_planes(), SRC, LIS, ear_spacing=0.18, max_order=8), 1, 256, True, False
    yield "more than 2^28 candidates, the last order alone", P.describe(sixteen_planes(), SRC, LIS, min_order=8, max_order=8), 1, 256, True, True


def test_refusals_change_nothing(gas):
    ok = P.describe(P.attic(), SRC, LIS, ear_spacing=0.18, max_order=3)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 4096)
        first = ctx.conv_ir_from_planes(ok, 2, 256)
        assert first == 0
        one_ear_inside = ok.copy()
        one_ear_inside["listener"]["origin"] = (-2.95, 1.0, -0.8)
        assert raw(ctx, one_ear_inside, 1, 256, np.zeros((1, 256), np.float32), False)[0] == 0  # the listener itself is inside
        for what, d, channels, taps, with_taps, with_ir in refusals():
            buf = np.full((max(channels, 1), max(taps, 1)), np.nan, np.float32) if with_taps else None
            rc, ir = raw(ctx, d, channels, taps, buf, with_ir)
            assert rc == -1, (what, rc)
            assert ir == 0xDEADBEEF, what
            assert buf is None or np.isnan(buf).all(), what
        assert ctx.lib.gas_conv_ir_from_planes(None, ptr(np.ascontiguousarray(ok)), 2, 256, None, C.byref(C.c_uint32())) == -1
        assert ctx.conv_ir_load(np.ones((1, 4), np.float32)) == 1  # the id it would have had: the table is as it was
        assert ctx.conv_ir_get_info(first) == (2, 256)
        with pytest.raises(gas.capi.GasError) as ei:
            ctx.conv_ir_get_info(2)
        assert ei.value.status == -3
