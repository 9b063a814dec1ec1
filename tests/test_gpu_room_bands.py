"""gas_conv_ir_from_room_bands and gas_conv_ir_from_room_hrtf_bands on the GPU: the band passes and k_room_bands_combine
against tests/room_bands_ref.py (float64), what is bitwise, the generated IR in the convolver calls, and the refusals.

Tolerance: helpers.TOL (1e-5), as relative RMS per channel and as max-abs relative to max|h|.  Device and reference hold
the same int64 band sums (tests/test_gpu_room_ir.py, test_gpu_room_brir.py); what differs is the order of the float64
sums of step 4, the two libraries' exp, sin and cos to an ulp or two, and then float32's last rounding, so the expected
error is a few 1e-9 at the most.  Every comparison prints its figures (and whether the taps are equal to the bit) before
it asserts.  Measured on an MI355X: at most 7e-18 and 9e-18 against the reference (every channel but one equal to the
bit), 3.8e-9 to 9.8e-9 relative RMS for equal bands against the plain device call (profiles/room_bands_notes.md).  Each
reference is computed once per case and shared (tests/room_bands_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import er_rooms_ref as E
import room_bands_cases as BC
import room_bands_ref as BD
import room_brir_cases as CS
import room_brir_ref as BR
import room_ir_ref as R
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

RATE = BC.RATE
F = 128
SENTINEL = 0xDEADBEEF
WORST = [0.0, 0.0]


def context(gas):
    return gas.SpatializerContext(max_sources=4, frames=F)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw(ctx, desc, bands, channels, taps, out_taps, want_ir):
    """The call itself -> (status, *out_ir): out_ir keeps the sentinel where the library does not write it."""
    out = C.c_uint32(SENTINEL)
    d = None if desc is None else np.ascontiguousarray(desc)
    b = None if bands is None else np.ascontiguousarray(bands)
    rc = ctx.lib.gas_conv_ir_from_room_bands(ctx.h, ptr(d), ptr(b), channels, taps, ptr(out_taps), C.byref(out) if want_ir else None)
    return rc, out.value


def raw_hrtf(ctx, desc, bands, hrir, n_az, n_el, hrir_taps, taps, out_taps, want_ir):
    out = C.c_uint32(SENTINEL)
    d = None if desc is None else np.ascontiguousarray(desc)
    b = None if bands is None else np.ascontiguousarray(bands)
    rc = ctx.lib.gas_conv_ir_from_room_hrtf_bands(ctx.h, ptr(d), ptr(b), ptr(hrir), n_az, n_el, hrir_taps, taps, ptr(out_taps), C.byref(out) if want_ir else None)
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


@pytest.mark.parametrize("name", list(BC.CASES))
def test_parity(gas, name):
    d, bands, channels, taps, ref = BC.reference(name)
    with context(gas) as ctx:
        h = ctx.conv_ir_from_room_bands(d, bands, channels, taps, want_taps=True, load=False)
    compare(name, h, ref.h)


def test_parity_hrtf(gas):
    d, bands, hrir, n_az, n_el, taps, ref = BC.hrtf_reference()
    assert ref.near_edge == 0
    with context(gas) as ctx:
        h = ctx.conv_ir_from_room_hrtf_bands(d, bands, hrir, n_az, n_el, taps, want_taps=True, load=False)
    compare("hrtf, B 3, L 255, 8x3, 32 hrir taps", h, ref.h)


ONE_BAND = (0.6, 0.65, 0.7, 0.75, 0.8, 0.85)


def one_band(filter_taps=0):
    """B = 1, no air; filter_taps and the entries beyond the first band are not read, whatever they hold."""
    b = BD.describe([ONE_BAND], filter_taps=filter_taps)
    b["crossover_hz"] = np.nan
    b["reflectance"][0, 1:] = 7.0
    b["air_db_per_m"][0, 1:] = -1.0
    return b


@pytest.mark.parametrize("channels,taps,min_order,filter_taps", [(1, 2000, 0, 0), (2, 2049, 3, 4096), (2, BC.SMALL_TILE + 1, 0, 255)])
def test_one_band_without_air_is_the_plain_call_bitwise(gas, channels, taps, min_order, filter_taps):
    d = BC.plain(ear_spacing=0.18, min_order=min_order)  # its own reflectances are validated, not used
    d1 = d.copy()
    d1["room"]["reflectance"] = ONE_BAND
    with context(gas) as ctx:
        want = ctx.conv_ir_from_room(d1, channels, taps, want_taps=True, load=False)
        other = ctx.conv_ir_from_room(d, channels, taps, want_taps=True, load=False)
        h = ctx.conv_ir_from_room_bands(d, one_band(filter_taps), channels, taps, want_taps=True, load=False)
    print(f"one band, {channels} ch, {taps} taps, min_order {min_order}: bitwise {h.tobytes() == want.tobytes()}")
    assert want.any() and want.tobytes() != other.tobytes()
    assert h.tobytes() == want.tobytes()


@pytest.mark.parametrize("delta", [False, True])
def test_one_band_without_air_is_the_plain_hrtf_call_bitwise(gas, delta):
    n_az, n_el = BC.HRTF_GRID
    hrir = BR.delta_set(n_az * n_el, 4) if delta else CS.noise_set(22, n_az * n_el, 32)
    d = CS.describe()
    d1 = d.copy()
    d1["room"]["reflectance"] = ONE_BAND
    with context(gas) as ctx:
        want = ctx.conv_ir_from_room_hrtf(d1, hrir, n_az, n_el, 2000, want_taps=True, load=False)
        h = ctx.conv_ir_from_room_hrtf_bands(d, one_band(), hrir, n_az, n_el, 2000, want_taps=True, load=False)
        mono = ctx.conv_ir_from_room(d1, 1, 2000, want_taps=True, load=False) if delta else None
    print(f"one band, hrtf, unit-impulse set {delta}: bitwise {h.tobytes() == want.tobytes()}")
    assert want[0].any() and want[1].any() and h.tobytes() == want.tobytes()
    if delta:  # and through the unit-impulse set both ears are the one-channel call
        assert h[0].tobytes() == mono[0].tobytes() and h[1].tobytes() == mono[0].tobytes()


@pytest.mark.parametrize("B,L,xo", [(2, 63, (2000.0,)), (3, 255, (500.0, 4000.0)), (8, 1023, BC.OCTAVES)])
def test_equal_bands_match_the_plain_call(gas, B, L, xo):
    d = BC.plain(ear_spacing=0.18)
    bands = BD.describe([BC.BASE] * B, xo, filter_taps=L)
    with context(gas) as ctx:
        want = ctx.conv_ir_from_room(d, 2, 2000, want_taps=True, load=False)
        h = ctx.conv_ir_from_room_bands(d, bands, 2, 2000, want_taps=True, load=False)
    compare(f"equal bands, B {B}, L {L}", h, want)


def test_equal_bands_match_the_plain_hrtf_call(gas):
    n_az, n_el = BC.HRTF_GRID
    hrir = CS.noise_set(22, n_az * n_el, 32)
    d = CS.describe()
    bands = BD.describe([BC.BASE] * 3, (500.0, 4000.0), filter_taps=255)
    with context(gas) as ctx:
        want = ctx.conv_ir_from_room_hrtf(d, hrir, n_az, n_el, 2000, want_taps=True, load=False)
        h = ctx.conv_ir_from_room_hrtf_bands(d, bands, hrir, n_az, n_el, 2000, want_taps=True, load=False)
    compare("equal bands, hrtf", h, want)


@pytest.mark.parametrize("level", [1.0, 0.7])
def test_direct_sound_is_the_level_exactly(gas, level):
    """Every wall dead in every band, air on every band: only m = 0 is left.  h[0] == level to the bit, and the other taps
    hold what the float64 sum of the band filters leaves of the delta."""
    d = R.describe(BC.small_room(level=level), BC.SRC, BC.LIS)
    with context(gas) as ctx:
        for B, L, xo, air in ((2, 63, (2000.0,), (0.0, 0.5)), (3, 255, (500.0, 4000.0), (0.1, 0.2, 0.3)), (8, 1023, BC.OCTAVES, (0.05,) * 8)):
            h = ctx.conv_ir_from_room_bands(d, BD.describe([(0.0,) * 6] * B, xo, air, L), 1, 2000, want_taps=True, load=False)
            print(f"B {B}, L {L}, level {level}: tap 0 {h[0, 0]!r}, max |other taps| {np.abs(h[0, 1:]).max():.3g}")
            assert h[0, 0].tobytes() == np.float32(level).tobytes(), (B, L)
            assert np.abs(h[0, 1:]).max() <= 1e-15


def test_two_calls_give_the_same_bits(gas):
    d, bands, channels, taps, _ = BC.reference("B 3, L 255, two channels, 2049 taps, air")
    dh, bh, hrir, n_az, n_el, th, _ = BC.hrtf_reference()
    with context(gas) as ctx:
        a = ctx.conv_ir_from_room_bands(d, bands, channels, taps, want_taps=True, load=False)
        b = ctx.conv_ir_from_room_bands(d, bands, channels, taps, want_taps=True, load=False)
        d2 = d.copy()
        d2["room"]["reflectance"] = 0.123  # validated, not used
        c = ctx.conv_ir_from_room_bands(d2, bands, channels, taps, want_taps=True, load=False)
        x = ctx.conv_ir_from_room_hrtf_bands(dh, bh, hrir, n_az, n_el, th, want_taps=True, load=False)
        y = ctx.conv_ir_from_room_hrtf_bands(dh, bh, hrir, n_az, n_el, th, want_taps=True, load=False)
    print(f"two runs: plain bitwise {a.tobytes() == b.tobytes()}, other descriptor reflectances bitwise {a.tobytes() == c.tobytes()}, hrtf bitwise {x.tobytes() == y.tobytes()}")
    assert a.any() and a.tobytes() == b.tobytes() == c.tobytes()
    assert x.any() and x.tobytes() == y.tobytes()


def test_registered_ir_is_the_loaded_one_bitwise(gas):
    """3 F + 40 taps: four partitions, the last a partial one; four blocks of noise reach every partition."""
    taps = 3 * F + 40
    d = BC.plain(ear_spacing=0.18)
    bands = BD.describe(BC.walls(3), (500.0, 4000.0), (0.0, 0.05, 0.3), 255)
    dh, hrir = CS.describe(), CS.noise_set(23, 24, 32)
    rng = np.random.default_rng(11)
    with context(gas) as ctx:
        ctx.reserve_conv(4, 4 * F)
        made, h = ctx.conv_ir_from_room_bands(d, bands, 2, taps, want_taps=True)
        assert ctx.conv_ir_get_info(made) == (2, taps)
        loaded = ctx.conv_ir_load(h)
        made2, h2 = ctx.conv_ir_from_room_hrtf_bands(dh, bands, hrir, 8, 3, taps, want_taps=True)
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
        assert ctx.conv_ir_from_room_bands(d, bands, 1, taps) == 0  # the lowest free id, as gas_conv_ir_load gives


def test_pure_generator_needs_no_reserve(gas):
    d, bands, channels, taps, ref = BC.reference("B 2, L 63, one channel, 2000 taps")
    dh, bh, hrir, n_az, n_el, th, refh = BC.hrtf_reference()
    with context(gas) as ctx:
        h = ctx.conv_ir_from_room_bands(d, bands, channels, taps, want_taps=True, load=False)
        assert rel_rms(h, ref.h) <= TOL
        buf = np.full((channels, taps), np.nan, np.float32)
        assert raw(ctx, d, bands, channels, taps, buf, True) == (-6, SENTINEL)  # GAS_ERR_UNSUPPORTED_CHAIN
        assert raw(ctx, d, bands, channels, taps, None, True) == (-6, SENTINEL)
        assert np.isnan(buf).all()
        buf = np.full((2, th), np.nan, np.float32)
        assert raw_hrtf(ctx, dh, bh, hrir, n_az, n_el, hrir.shape[2], th, buf, True) == (-6, SENTINEL)
        assert np.isnan(buf).all()


def band_refusals():
    """(what, bands): everything gas_room_bands itself can be refused for."""
    ok = BD.describe(BC.walls(3), (500.0, 4000.0), (0.0, 0.05, 0.3), 255)

    def bands(**kw):
        b = ok.copy()
        for k, v in kw.items():
            b[k] = v
        return b

    def at(field, index, v):
        b = ok.copy()
        b[field][(0,) + index] = v
        return b

    yield "NULL bands", None
    yield "no bands", bands(n_bands=0)
    yield "nine bands", bands(n_bands=9)
    yield "filter_taps even", bands(filter_taps=254)
    yield "filter_taps 1", bands(filter_taps=1)
    yield "filter_taps 0", bands(filter_taps=0)
    yield "filter_taps 4097", bands(filter_taps=4097)
    yield "crossover nan", at("crossover_hz", (1,), np.nan)
    yield "crossover inf", at("crossover_hz", (1,), np.inf)
    yield "crossover 0", at("crossover_hz", (0,), 0.0)
    yield "crossover negative", at("crossover_hz", (0,), -500.0)
    yield "crossover at rate / 2", at("crossover_hz", (1,), 24000.0)
    yield "crossovers equal", at("crossover_hz", (1,), 500.0)
    yield "crossovers descending", at("crossover_hz", (1,), 400.0)
    yield "reflectance > 1", at("reflectance", (2, 5), 1.5)
    yield "reflectance < 0", at("reflectance", (0, 0), -0.1)
    yield "reflectance nan", at("reflectance", (1, 3), np.nan)
    yield "air negative", at("air_db_per_m", (2,), -0.1)
    yield "air nan", at("air_db_per_m", (0,), np.nan)
    yield "air inf", at("air_db_per_m", (1,), np.inf)
    yield "reserved 1", bands(reserved=1)


def plain_refusals():
    """(what, descriptor, channels, taps, with out_taps, with out_ir) under a reserve of 4096 taps: what the plain call
    refuses, a sample of every group of tests/test_gpu_room_ir.py's list."""
    ok = BC.plain(ear_spacing=0.18)

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

    cube = R.describe(E.unit_room(half_extent=(0.5, 0.5, 0.5)), (0.25, 0.0, 0.0), (-0.25, 0.0, 0.0))
    yield "NULL descriptor", None, 2, 256, True, True
    yield "neither output", ok, 2, 256, False, False
    yield "channels 0", ok, 0, 256, True, True
    yield "channels 4", ok, 4, 256, True, True
    yield "no taps", ok, 2, 0, True, True
    yield "more taps than the reserve", ok, 1, 4097, True, True
    yield "more taps than 2^20 for the pure generator", ok, 1, (1 << 20) + 1, True, False
    yield "half extent 0", room(half_extent=(2.5, 0.0, 1.5)), 2, 256, True, True
    yield "speed of sound 0", room(speed_of_sound=0.0), 2, 256, True, True
    yield "level inf", room(level=np.inf), 2, 256, True, True
    yield "the descriptor's own reflectance > 1", room(reflectance=(0.9, 1.5, 0.8, 0.8, 0.8, 0.8)), 2, 256, True, True
    yield "the descriptor's own reflectance nan", room(reflectance=(0.9, np.nan, 0.8, 0.8, 0.8, 0.8)), 2, 256, True, True
    yield "min_order > max_order", desc(min_order=4, max_order=3), 2, 256, True, True
    yield "ear spacing nan", desc(ear_spacing=np.nan), 1, 256, True, True
    yield "source nan", desc(source=(1.0, np.nan, 0.25)), 2, 256, True, True
    yield "source outside", desc(source=(2.6, 0.5, 0.25)), 2, 256, True, True
    yield "source at the listener", desc(source=BC.LIS), 2, 256, True, True
    yield "box over the cap", cube, 1, 1 << 20, True, False


def test_refusals_change_nothing(gas):
    ok = BC.plain(ear_spacing=0.18)
    good = BD.describe(BC.walls(3), (500.0, 4000.0), (0.0, 0.05, 0.3), 255)
    n_az, n_el = BC.HRTF_GRID
    hrir = CS.noise_set(24, n_az * n_el, 32)
    with context(gas) as ctx:
        ctx.reserve_conv(2, 4096)
        first = ctx.conv_ir_from_room_bands(ok, good, 2, 256)
        assert first == 0
        for what, b in band_refusals():
            buf = np.full((2, 256), np.nan, np.float32)
            assert raw(ctx, ok, b, 2, 256, buf, True) == (-1, SENTINEL), what
            assert np.isnan(buf).all(), what
            assert raw(ctx, ok, b, 2, 256, buf, False) == (-1, SENTINEL), what  # the pure generator refuses the same
            assert np.isnan(buf).all(), what
            assert raw_hrtf(ctx, CS.describe(), b, hrir, n_az, n_el, 32, 256, buf, True) == (-1, SENTINEL), what
            assert np.isnan(buf).all(), what
        for what, d, channels, taps, with_taps, with_ir in plain_refusals():
            buf = np.full((max(channels, 1), max(taps, 1)), np.nan, np.float32) if with_taps else None
            rc, ir = raw(ctx, d, good, channels, taps, buf, with_ir)
            assert (rc, ir) == (-1, SENTINEL), (what, rc)
            assert buf is None or np.isnan(buf).all(), what
        buf = np.full((2, 256), np.nan, np.float32)
        for what, args in (
            ("NULL descriptor", (None, good, hrir, n_az, n_el, 32, 256)),
            ("NULL hrir", (CS.describe(), good, None, n_az, n_el, 32, 256)),
            ("n_az 0", (CS.describe(), good, hrir, 0, n_el, 32, 256)),
            ("hrir_taps 257", (CS.describe(), good, hrir, n_az, n_el, 257, 256)),
            ("no taps", (CS.describe(), good, hrir, n_az, n_el, 32, 0)),
            ("more taps than the reserve", (CS.describe(), good, hrir, n_az, n_el, 32, 4097)),
        ):
            assert raw_hrtf(ctx, *args, buf, True) == (-1, SENTINEL), what
            assert np.isnan(buf).all(), what
        bad = hrir.copy()
        bad[3, 1, 7] = 4.5
        assert raw_hrtf(ctx, CS.describe(), good, bad, n_az, n_el, 32, 256, buf, True) == (-1, SENTINEL)
        assert ctx.lib.gas_conv_ir_from_room_bands(None, ptr(np.ascontiguousarray(ok)), ptr(good), 2, 256, None, C.byref(C.c_uint32())) == -1
        # the edges of what is allowed: eight bands, the largest filter, reflectances 0 and 1, entries beyond B not read
        edge = BD.describe([[0.0, 1.0, 0.5, 0.5, 0.5, 0.5]] * 2, (23999.0,), (0.0, 0.0), 4095)
        edge["crossover_hz"][0, 1:] = np.nan
        edge["reflectance"][0, 2:] = -3.0
        edge["air_db_per_m"][0, 2:] = np.nan
        assert ctx.conv_ir_from_room_bands(ok, edge, 1, 64) == 1
        ctx.conv_ir_free(1)
        assert ctx.conv_ir_load(np.ones((1, 4), np.float32)) == 1  # the id it would have had: the table is as it was
        assert ctx.conv_ir_get_info(first) == (2, 256)
        with pytest.raises(gas.capi.GasError) as ei:
            ctx.conv_ir_get_info(2)
        assert ei.value.status == -3
