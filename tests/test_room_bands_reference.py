"""tests/room_bands_ref.py on its own, without a GPU: the properties the rule of gas_conv_ir_from_room_bands promises,
checked on the float64 reference with test_gpu_room_ir.py's small room at 48 kHz, and the conditions on the cases
tests/test_gpu_room_bands.py uses.

Bars.  The filters sum to delta_D up to the roundings of B - 1 differences of values below 1: 1e-15 absolute.  Equal
bands against the plain reference: helpers.TOL (measured 3.5e-9 to 7.2e-9, float32's last rounding).  A dead high band:
the spectrum's mean energy above twice the crossover lies at least 40 dB below that between 200 Hz and half the
crossover (the window's design stopband is 74 dB; the reference gives about 65 dB)."""
import numpy as np
import pytest

import room_bands_cases as BC
import room_bands_ref as BD
import room_ir_ref as R
from helpers import TOL, rel_rms

RATE = BC.RATE


def plain(**kw):
    return BC.plain(**kw)


@pytest.mark.parametrize("B,L,xo", [(2, 3, (2000.0,)), (2, 63, (2000.0,)), (3, 255, (500.0, 4000.0)), (8, 1023, BC.OCTAVES), (2, 4095, (1000.0,))])
def test_filters_sum_to_the_delta(B, L, xo):
    F, l, D = BD.filters(B, L, xo, RATE)
    assert (l, D, len(F)) == (L, (L - 1) // 2, B) and all(f.shape == (L,) for f in F)
    delta = np.zeros(L)
    delta[D] = 1.0
    err = np.abs(np.sum(F, axis=0) - delta).max()
    print(f"B {B}, L {L}: max |sum F - delta| {err:.3g}")
    assert err <= 1e-15
    assert abs(F[0].sum() - 1.0) <= 1e-14  # a low pass of unit gain at 0 Hz


def test_one_band_has_a_one_tap_filter_whatever_filter_taps_says():
    F, L, D = BD.filters(1, 12345, (), RATE)
    assert (L, D) == (1, 0) and F[0].tolist() == [1.0]


@pytest.mark.parametrize("channels,min_order", [(1, 0), (2, 3)])
def test_one_band_without_air_is_the_plain_reference_bitwise(channels, min_order):
    refl = (0.6, 0.65, 0.7, 0.75, 0.8, 0.85)
    d = plain(ear_spacing=0.18, min_order=min_order)  # its own reflectances are not used
    bands = BD.describe([refl], filter_taps=0)
    got = BD.ir(d, bands, channels, 2000, RATE)
    d1 = d.copy()
    d1["room"]["reflectance"] = refl
    want = R.ir(d1, channels, 2000, RATE)
    assert want.h.any() and got.h.tobytes() == want.h.tobytes()
    assert not np.array_equal(want.h, R.ir(d, channels, 2000, RATE).h)


@pytest.mark.parametrize("B,L,xo", [(2, 63, (2000.0,)), (3, 255, (500.0, 4000.0)), (8, 1023, BC.OCTAVES)])
def test_equal_bands_without_air_match_the_plain_reference(B, L, xo):
    d = plain(ear_spacing=0.18)
    want = R.ir(d, 2, 2000, RATE)
    got = BD.ir(d, BD.describe([BC.BASE] * B, xo, filter_taps=L), 2, 2000, RATE)
    for e in range(2):
        rms = rel_rms(got.h[e], want.h[e])
        mx = np.abs(got.h[e].astype(np.float64) - want.h[e]).max() / np.abs(want.h[e]).max()
        print(f"B {B}, L {L}, ch {e}: rel rms {rms:.3g}, max abs / max|h| {mx:.3g}")
        assert rms <= TOL and mx <= TOL


@pytest.mark.parametrize("L,xo", [(255, 2000.0), (127, 3000.0)])
def test_a_dead_high_band_is_suppressed(L, xo):
    d = plain(min_order=1)
    got = BD.ir(d, BD.describe([BC.BASE, (0.0,) * 6], (xo,), filter_taps=L), 1, 4096, RATE)
    S = np.abs(np.fft.rfft(got.y[0])) ** 2
    f = np.fft.rfftfreq(4096, 1.0 / RATE)
    low = S[(f > 200.0) & (f < xo / 2)].mean()
    high = S[f > 2 * xo].mean()
    db = 10.0 * np.log10(high / low)
    print(f"L {L}, crossover {xo}: above twice the crossover {db:.1f} dB relative to 200 Hz .. half the crossover")
    assert db <= -40.0


def test_air_leaves_tap_0_and_lowers_the_tail():
    d = plain()
    dry = BD.ir(d, BD.describe([BC.BASE] * 2, (2000.0,), (0.0, 0.0), 255), 1, 4096, RATE)
    wet = BD.ir(d, BD.describe([BC.BASE] * 2, (2000.0,), (0.0, 0.5), 255), 1, 4096, RATE)
    assert wet.lam[0] == 0.0 and wet.lam[1] > 0.0
    assert wet.y[0, 0] == dry.y[0, 0] and wet.h[0, 0] == np.float32(1.0)
    ratio = float((wet.y[0, 2000:] ** 2).sum() / (dry.y[0, 2000:] ** 2).sum())
    print(f"energy of taps 2000 .. 4095 with 0.5 dB/m on the high band over without: {ratio:.3f}")
    assert 0.3 < ratio < 0.7  # the low band, untouched, holds about half of the tail's energy


@pytest.mark.parametrize("level", [1.0, 0.7])
def test_direct_sound_is_the_level_exactly(level):
    """min_order = 0: tap 0 is `level` to the bit whatever the bands and the air (R = 1 in every band, g[0] = 1, and the
    filters sum to the delta)."""
    d = R.describe(BC.small_room(level=level), BC.SRC, BC.LIS)
    for B, L, xo, air in ((2, 63, (2000.0,), (0.0, 0.5)), (3, 255, (500.0, 4000.0), (0.1, 0.2, 0.3)), (8, 1023, BC.OCTAVES, (0.05,) * 8)):
        got = BD.ir(d, BD.describe([(0.0,) * 6] * B, xo, air, L), 1, 600, RATE)
        assert got.h[0, 0].tobytes() == np.float32(level).tobytes(), (B, L)
        assert np.abs(got.h[0, 1:]).max() <= 1e-15  # every wall dead: nothing but what the filters' sum leaves of the delta


@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_gpu_cases_are_what_they_say(name):
    d, bands, channels, taps, ref = BC.reference(name)
    b = bands[0]
    B = int(b["n_bands"])
    assert ref.h.shape == (channels, taps) and all(ref.h[e].any() for e in range(channels))
    assert len({tuple(b["reflectance"][i]) for i in range(B)}) == B  # distinct per band
    assert all(ref.acc[i].any() for i in range(B))
    if "taps < D" in name:
        assert taps < ref.D and np.count_nonzero(ref.acc[0]) >= 12


def test_the_hrtf_case_has_no_image_near_a_cells_edge():
    _, _, hrir, n_az, n_el, taps, ref = BC.hrtf_reference()
    assert ref.near_edge == 0 and ref.h[0].any() and ref.h[1].any()
    assert hrir.shape == (n_az * n_el, 2, 32) and (n_az, n_el, taps) == (8, 3, 2000)
