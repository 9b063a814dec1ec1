"""gas_conv_ir_from_room_diffuse and gas_conv_ir_from_room_hrtf_diffuse on the GPU: the lattice passes for K1 taps,
k_room_tail and k_room_bands_combine against tests/room_tail_ref.py (float64), what is bitwise, the generated IR in the
convolver calls, and the refusals.

Tolerance: helpers.TOL (1e-5), as relative RMS per channel and as max-abs relative to max|h|, the bar of
tests/test_gpu_room_bands.py.  Device and reference hold the same specular int64 sums; the diffuse part differs by the
two libraries' exp to an ulp or two, which moves llrint(. 2^32) by one unit (2.3e-10) here and there, then by the order
of the float64 sums of the band filters and float32's last rounding, so the expected error is a few 1e-9 at the most.
Every comparison prints its figures (and whether the taps are equal to the bit) before it asserts.  Measured on an
MI355X: at most 1.3e-17 and 1.4e-17 (every channel but three equal to the bit; profiles/room_tail_notes.md).  Each
reference is computed once per case and shared (tests/room_tail_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import er_rooms_ref as E
import room_bands_cases as BC
import room_brir_cases as CS
import room_ir_ref as R
import room_tail_cases as TC
import room_tail_ref as T
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

RATE = TC.RATE
F = 128
SENTINEL = 0xDEADBEEF
WORST = [0.0, 0.0]


def context(gas):
    return gas.SpatializerContext(max_sources=4, frames=F)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw(ctx, desc, bands, tail, channels, taps, out_taps, want_ir):
    """The call itself -> (status, *out_ir): out_ir keeps the sentinel where the library does not write it."""
    out = C.c_uint32(SENTINEL)
    d, b, t = (None if a is None else np.ascontiguousarray(a) for a in (desc, bands, tail))
    rc = ctx.lib.gas_conv_ir_from_room_diffuse(ctx.h, ptr(d), ptr(b), ptr(t), channels, taps, ptr(out_taps), C.byref(out) if want_ir else None)
    return rc, out.value


def raw_hrtf(ctx, desc, bands, tail, hrir, n_az, n_el, hrir_taps, taps, out_taps, want_ir):
    out = C.c_uint32(SENTINEL)
    d, b, t = (None if a is None else np.ascontiguousarray(a) for a in (desc, bands, tail))
    rc = ctx.lib.gas_conv_ir_from_room_hrtf_diffuse(ctx.h, ptr(d), ptr(b), ptr(t), ptr(hrir), n_az, n_el, hrir_taps, taps, ptr(out_taps), C.byref(out) if want_ir else None)
    return rc, out.value


def compare(what, h, want):
    """Prints and asserts the two figures per channel."""
    assert h.shape == want.shape and h.dtype == np.float32
    for e in range(h.shape[0]):
        assert want[e].any(), (what, e)
        rms = rel_rms(h[e], want[e])
        mx = np.abs(h[e].astype(np.float64) - want[e]).max() / np.abs(want[e]).max()
        WORST[0], WORST[1] = max(WORST[0], rms), max(WORST[1], mx)
        print(f"{what} ch {e}: rel rms {rms:.3g}, max abs / max|h| {mx:.3g}, bitwise {np.array_equal(h[e], want[e])} (worst so far {WORST[0]:.3g}, {WORST[1]:.3g})")
        assert rms <= TOL and mx <= TOL, (what, e, rms, mx)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_parity(gas, name):
    d, bands, t, channels, taps, ref = TC.reference(name)
    with context(gas) as ctx:
        h = ctx.conv_ir_from_room_diffuse(d, bands, t, channels, taps, want_taps=True, load=False)
    compare(name, h, ref.h)


@pytest.mark.parametrize("delta", [False, True])
def test_parity_hrtf(gas, delta):
    d, bands, t, hrir, n_az, n_el, taps, ref = TC.hrtf_reference(delta)
    assert ref.near_edge == 0
    with context(gas) as ctx:
        h = ctx.conv_ir_from_room_hrtf_diffuse(d, bands, t, hrir, n_az, n_el, taps, want_taps=True, load=False)
        if delta:  # the specular part is the one-channel call's in both ears; the diffuse parts differ per ear
            mono = ctx.conv_ir_from_room_diffuse(d, bands, t, 1, taps, want_taps=True, load=False)
            edge = ref.K0 - ref.D
            assert h[0, :edge].any() and h[0, :edge].tobytes() == mono[0, :edge].tobytes() == h[1, :edge].tobytes()
            assert h[0].tobytes() == mono[0].tobytes()  # ear 0 hears the one-channel call's noise stream as well
            assert np.count_nonzero(h[0, ref.K1 :] != h[1, ref.K1 :]) > 0.99 * (taps - ref.K1)
    compare(f"hrtf, B 3, L 255, 8x3, unit-impulse set {delta}", h, ref.h)


@pytest.mark.parametrize("name", ["B 3, L 255, 200 taps, K0 == taps", "B 1, 200 taps, K1 == taps", "B 3, L 255, 6001 taps, fade 0, min_order 3"])
def test_k0_at_taps_is_the_bands_call_bitwise(gas, name):
    d, bands, _, channels, taps, _ = TC.reference(name)
    with context(gas) as ctx:
        want = ctx.conv_ir_from_room_bands(d, bands, channels, taps, want_taps=True, load=False)
        for t in (TC.tail(taps, 0), TC.tail(taps + 1000, 77, seed=99, gain=3.0), T.describe(5, 3.0e38, 3.0e38, 0.0)):
            h = ctx.conv_ir_from_room_diffuse(d, bands, t, channels, taps, want_taps=True, load=False)
            print(f"{name}: K0 == taps bitwise {h.tobytes() == want.tobytes()}")
            assert want.any() and h.tobytes() == want.tobytes()


def test_k0_at_taps_is_the_hrtf_bands_call_bitwise(gas):
    d, bands, _, hrir, n_az, n_el, taps, _ = TC.hrtf_reference()
    with context(gas) as ctx:
        want = ctx.conv_ir_from_room_hrtf_bands(d, bands, hrir, n_az, n_el, taps, want_taps=True, load=False)
        h = ctx.conv_ir_from_room_hrtf_diffuse(d, bands, TC.tail(taps, 5), hrir, n_az, n_el, taps, want_taps=True, load=False)
    assert want.any() and h.tobytes() == want.tobytes()


def test_head_is_the_bands_call_and_gain_0_is_silent(gas):
    """Taps below K0 - D are the *_bands call's whatever the tail; with gain 0 every tap from K1 + D on is 0; another
    seed gives other taps from K0 on."""
    d, bands, t, channels, taps, ref = TC.reference("B 3, L 255, 4096 taps, K1 == taps")
    k0, k1, D = 3000, 3500, ref.D
    with context(gas) as ctx:
        want = ctx.conv_ir_from_room_bands(d, bands, channels, taps, want_taps=True, load=False)
        a = ctx.conv_ir_from_room_diffuse(d, bands, TC.tail(k0, k1 - k0, seed=1), channels, taps, want_taps=True, load=False)
        b = ctx.conv_ir_from_room_diffuse(d, bands, TC.tail(k0, k1 - k0, seed=2), channels, taps, want_taps=True, load=False)
        z = ctx.conv_ir_from_room_diffuse(d, bands, TC.tail(k0, k1 - k0, seed=1, gain=0.0), channels, taps, want_taps=True, load=False)
    assert D == 127 and want[:, : k0 - D].any()
    for h in (a, b, z):
        assert h[:, : k0 - D].tobytes() == want[:, : k0 - D].tobytes()
    assert z[:, k0:k1].any() and not z[:, k1 + D :].any()
    for e in range(channels):
        assert np.count_nonzero(a[e, k0 + 1 :] != b[e, k0 + 1 :]) > 0.99 * (taps - k0 - 1)


def test_two_calls_give_the_same_bits(gas):
    d, bands, t, channels, taps, _ = TC.reference("B 3, L 255, 4096 taps, marks across a tile's and two waves' ends, air on one band")
    dh, bh, th, hrir, n_az, n_el, nh, _ = TC.hrtf_reference()
    with context(gas) as ctx:
        a = ctx.conv_ir_from_room_diffuse(d, bands, t, channels, taps, want_taps=True, load=False)
        b = ctx.conv_ir_from_room_diffuse(d, bands, t, channels, taps, want_taps=True, load=False)
        x = ctx.conv_ir_from_room_hrtf_diffuse(dh, bh, th, hrir, n_az, n_el, nh, want_taps=True, load=False)
        y = ctx.conv_ir_from_room_hrtf_diffuse(dh, bh, th, hrir, n_az, n_el, nh, want_taps=True, load=False)
    print(f"two runs: bitwise {a.tobytes() == b.tobytes()}, hrtf bitwise {x.tobytes() == y.tobytes()}")
    assert a.any() and a.tobytes() == b.tobytes()
    assert x.any() and x.tobytes() == y.tobytes()


def test_registered_ir_is_the_loaded_one_bitwise(gas):
    """3 F + 40 taps: four partitions, the last a partial one; four blocks of noise reach every partition."""
    taps = 3 * F + 40
    d = BC.plain(ear_spacing=0.18)
    bands = TC.three_bands((0.0, 0.05, 0.3))
    t = TC.tail(150, 100, seed=31)
    dh, hrir = CS.describe(), CS.noise_set(23, 24, 32)
    rng = np.random.default_rng(11)
    with context(gas) as ctx:
        ctx.reserve_conv(4, 4 * F)
        made, h = ctx.conv_ir_from_room_diffuse(d, bands, t, 2, taps, want_taps=True)
        assert ctx.conv_ir_get_info(made) == (2, taps)
        pure = ctx.conv_ir_from_room_diffuse(d, bands, t, 2, taps, want_taps=True, load=False)
        assert h.tobytes() == pure.tobytes()
        loaded = ctx.conv_ir_load(h)
        made2, h2 = ctx.conv_ir_from_room_hrtf_diffuse(dh, bands, t, hrir, 8, 3, taps, want_taps=True)
        assert ctx.conv_ir_get_info(made2) == (2, taps)
        loaded2 = ctx.conv_ir_load(h2)
        assert (made, loaded, made2, loaded2) == (0, 1, 2, 3)
        convs = [ctx.conv_create(i) for i in (made, loaded, made2, loaded2)]
        for _ in range(4):
            x = rng.uniform(-1, 1, (1, F, 2)).astype(np.float32)
            y = ctx.conv_process(convs, np.concatenate([x, x, x, x]))
            assert y[0].any() and y[0].tobytes() == y[1].tobytes()
            assert y[2].any() and y[2].tobytes() == y[3].tobytes() and y[2].tobytes() != y[0].tobytes()
        for k in convs:
            ctx.conv_destroy(k)
        ctx.conv_ir_free(made)
        assert ctx.conv_ir_from_room_diffuse(d, bands, t, 1, taps) == 0  # the lowest free id, as gas_conv_ir_load gives


def test_pure_generator_needs_no_reserve(gas):
    d, bands, t, channels, taps, ref = TC.reference("B 1, 200 taps, marks inside a wave")
    dh, bh, th, hrir, n_az, n_el, nh, _ = TC.hrtf_reference()
    with context(gas) as ctx:
        h = ctx.conv_ir_from_room_diffuse(d, bands, t, channels, taps, want_taps=True, load=False)
        assert rel_rms(h, ref.h) <= TOL
        buf = np.full((channels, taps), np.nan, np.float32)
        assert raw(ctx, d, bands, t, channels, taps, buf, True) == (-6, SENTINEL)  # GAS_ERR_UNSUPPORTED_CHAIN
        assert raw(ctx, d, bands, t, channels, taps, None, True) == (-6, SENTINEL)
        assert np.isnan(buf).all()
        buf = np.full((2, nh), np.nan, np.float32)
        assert raw_hrtf(ctx, dh, bh, th, hrir, n_az, n_el, hrir.shape[2], nh, buf, True) == (-6, SENTINEL)
        assert np.isnan(buf).all()


def test_cell_check_is_made_for_k1_taps(gas):
    """A half-metre cube at 2^20 taps is past 2^28 cells for the *_bands call; with the images kept for 4800 taps it is
    generated, and with K1 == 0 not even a lattice as long as the IR would fit is asked for."""
    cube = R.describe(E.unit_room(half_extent=(0.5, 0.5, 0.5)), (0.25, 0.0, 0.0), (-0.25, 0.0, 0.0))
    bands = T.BD.describe([(1.0,) * 6])  # rho = 1: the diffuse part does not decay, so the last taps are not silent
    taps = 1 << 20
    with context(gas) as ctx:
        buf = np.full((1, taps), np.nan, np.float32)
        rc = ctx.lib.gas_conv_ir_from_room_bands(ctx.h, ptr(np.ascontiguousarray(cube)), ptr(bands), 1, taps, ptr(buf), None)
        assert rc == -1 and np.isnan(buf).all()
        assert raw(ctx, cube, bands, TC.tail(taps, 0), 1, taps, buf, False) == (-1, SENTINEL) and np.isnan(buf).all()
        h = ctx.conv_ir_from_room_diffuse(cube, bands, TC.tail(3840, 960, seed=3), 1, taps, want_taps=True, load=False)
        assert np.isfinite(h).all() and h[0, :4800].any() and h[0, -4096:].any()
        z = ctx.conv_ir_from_room_diffuse(cube, bands, TC.tail(3840, 960, seed=3, gain=0.0), 1, taps, want_taps=True, load=False)
        assert z[0, :3840].tobytes() == h[0, :3840].tobytes() and not z[0, 4800:].any()
        p = ctx.conv_ir_from_room_diffuse(cube, bands, TC.tail(0, 0, seed=3), 1, taps, want_taps=True, load=False)
        assert np.isfinite(p).all() and p[0, 0] != 0 and p[0, -4096:].any()
        assert p[0, 4800:].tobytes() == h[0, 4800:].tobytes()  # behind the fade both are the diffuse part alone


def tail_refusals():
    """(what, tail): everything gas_room_tail itself can be refused for."""
    ok = TC.tail(100, 50, seed=3)

    def tail(**kw):
        t = ok.copy()
        for k, v in kw.items():
            t[k] = v
        return t

    yield "NULL tail", None
    for field in ("mix_time_s", "fade_s", "gain"):
        yield field + " negative", tail(**{field: -1e-6})
        yield field + " nan", tail(**{field: np.nan})
        yield field + " inf", tail(**{field: np.inf})
    for i in range(4):
        t = ok.copy()
        t["reserved"][0, i] = 1
        yield f"reserved[{i}] 1", t
    yield "s0 above 1024", tail(gain=1.0e6)
    yield "s0 far above 1024", tail(gain=3.0e38)


def test_refusals_change_nothing(gas):
    ok = BC.plain(ear_spacing=0.18)
    good = TC.three_bands((0.0, 0.05, 0.3))
    fine = TC.tail(100, 50, seed=3)
    n_az, n_el = TC.HRTF_GRID
    hrir = CS.noise_set(24, n_az * n_el, 32)
    with context(gas) as ctx:
        ctx.reserve_conv(2, 4096)
        first = ctx.conv_ir_from_room_diffuse(ok, good, fine, 2, 256)
        assert first == 0
        for what, t in tail_refusals():
            buf = np.full((2, 256), np.nan, np.float32)
            assert raw(ctx, ok, good, t, 2, 256, buf, True) == (-1, SENTINEL), what
            assert np.isnan(buf).all(), what
            assert raw(ctx, ok, good, t, 2, 256, buf, False) == (-1, SENTINEL), what  # the pure generator refuses the same
            assert np.isnan(buf).all(), what
            assert raw_hrtf(ctx, CS.describe(), good, t, hrir, n_az, n_el, 32, 256, buf, True) == (-1, SENTINEL), what
            assert np.isnan(buf).all(), what
        # what the *_bands call of the same name refuses: a sample of every group of tests/test_gpu_room_bands.py's lists
        buf = np.full((2, 256), np.nan, np.float32)
        bad_bands = good.copy()
        bad_bands["reserved"] = 1
        nine = good.copy()
        nine["n_bands"] = 9
        outside = ok.copy()
        outside["source"] = (2.6, 0.5, 0.25)
        at_listener = ok.copy()
        at_listener["source"] = BC.LIS
        orders = ok.copy()
        orders["min_order"], orders["max_order"] = 4, 3
        for what, args in (
            ("NULL descriptor", (None, good, fine, 2, 256)),
            ("NULL bands", (ok, None, fine, 2, 256)),
            ("bands reserved", (ok, bad_bands, fine, 2, 256)),
            ("nine bands", (ok, nine, fine, 2, 256)),
            ("channels 0", (ok, good, fine, 0, 256)),
            ("channels 4", (ok, good, fine, 4, 256)),
            ("no taps", (ok, good, fine, 2, 0)),
            ("more taps than the reserve", (ok, good, fine, 1, 4097)),
            ("source outside", (outside, good, fine, 2, 256)),
            ("source at the listener", (at_listener, good, fine, 2, 256)),
            ("source at the listener, no lattice", (at_listener, good, TC.tail(0, 0), 2, 256)),
            ("source outside, no lattice", (outside, good, TC.tail(0, 0), 2, 256)),
            ("min_order > max_order", (orders, good, fine, 2, 256)),
            ("min_order > max_order, no lattice", (orders, good, TC.tail(0, 0), 2, 256)),
        ):
            assert raw(ctx, *args, buf, True) == (-1, SENTINEL), what
            assert np.isnan(buf).all(), what
        assert raw(ctx, ok, good, fine, 2, 256, None, False) == (-1, SENTINEL)  # neither output
        big_buf = np.full((1, (1 << 20) + 1), np.nan, np.float32)
        assert raw(ctx, ok, good, fine, 1, (1 << 20) + 1, big_buf, False) == (-1, SENTINEL) and np.isnan(big_buf).all()
        for what, args in (
            ("NULL descriptor", (None, good, fine, hrir, n_az, n_el, 32, 256)),
            ("NULL bands", (CS.describe(), None, fine, hrir, n_az, n_el, 32, 256)),
            ("NULL hrir", (CS.describe(), good, fine, None, n_az, n_el, 32, 256)),
            ("n_az 0", (CS.describe(), good, fine, hrir, 0, n_el, 32, 256)),
            ("hrir_taps 257", (CS.describe(), good, fine, hrir, n_az, n_el, 257, 256)),
            ("no taps", (CS.describe(), good, fine, hrir, n_az, n_el, 32, 0)),
            ("more taps than the reserve", (CS.describe(), good, fine, hrir, n_az, n_el, 32, 4097)),
        ):
            assert raw_hrtf(ctx, *args, buf, True) == (-1, SENTINEL), what
            assert np.isnan(buf).all(), what
        bad = hrir.copy()
        bad[3, 1, 7] = 4.5
        assert raw_hrtf(ctx, CS.describe(), good, fine, bad, n_az, n_el, 32, 256, buf, True) == (-1, SENTINEL)
        assert ctx.lib.gas_conv_ir_from_room_diffuse(None, ptr(np.ascontiguousarray(ok)), ptr(good), ptr(fine), 2, 256, None, C.byref(C.c_uint32())) == -1
        # the edges of what is allowed: everything 0, and s0 just below its bound
        assert ctx.conv_ir_from_room_diffuse(ok, good, T.describe(0, 0.0, 0.0, 0.0), 1, 64) == 1
        ctx.conv_ir_free(1)
        s0 = T.decay(ok, good, T.describe(gain=1.0), R.geometry(ok, 2, 256, RATE)[3], float(ok["room"]["speed_of_sound"][0]), RATE)[2]
        assert ctx.conv_ir_from_room_diffuse(ok, good, T.describe(0, 0.001, 0.001, 1000.0 / s0), 2, 256) == 1
        ctx.conv_ir_free(1)
        assert ctx.conv_ir_load(np.ones((1, 4), np.float32)) == 1  # the id it would have had: the table is as it was
        assert ctx.conv_ir_get_info(first) == (2, 256)
        with pytest.raises(gas.capi.GasError) as ei:
            ctx.conv_ir_get_info(2)
        assert ei.value.status == -3
