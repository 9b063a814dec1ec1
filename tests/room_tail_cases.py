"""The inputs tests/test_gpu_room_tail.py compares against tests/room_tail_ref.py, kept apart from it so that
tests/test_room_tail_reference.py can check the conditions on them (the marks each case is named for, near_edge == 0,
results that are not silent) without a GPU.

A case is name -> (descriptor, bands, tail, channels, taps); reference(name) computes room_tail_ref.ir once per process
and shares it read-only.  The room is test_gpu_room_ir.py's 5 x 4 x 3 m box at 48 kHz.  The tail kernel gives a tap to a
lane, 64 to a wave and 256 to a workgroup (a tile); the marks K0 and K1 stand inside a tile, across the ends of a wave
and of a tile, below the band filters' delay D, at the last tap and on top of each other.  Every lattice is walked for
K1 taps only, so the references cost a few short convolutions."""
import functools

import room_bands_cases as BC
import room_bands_ref as BD
import room_brir_cases as CS
import room_tail_ref as T

RATE = BC.RATE
WAVE, TILE = 64, 256
XO3 = (500.0, 4000.0)


def tail(k0, kf, seed=1, gain=1.0):
    """Marks in taps: the cross-fade begins at tap k0 and is kf taps long."""
    return T.describe(seed, k0 / RATE, kf / RATE, gain)


def one_band(air=0.0):
    return BD.describe([BC.BASE], air_db_per_m=(air,))


def three_bands(air=(0.0, 0.0, 0.0), dead=None):
    w = BC.walls(3)
    if dead is not None:
        w[dead] = [0.0] * 6
    return BD.describe(w, XO3, air, 255)


# name -> (descriptor, bands, tail, channels, taps), (K0, K1) as the name says
CASES = {
    "B 1, one tap, pure diffuse": (lambda: (BC.plain(), one_band(), tail(0, 0), 1, 1), (0, 0)),
    "B 1, one tap, specular": (lambda: (BC.plain(), one_band(), tail(5, 5), 1, 1), (1, 1)),
    "B 1, 200 taps, marks inside a wave": (lambda: (BC.plain(ear_spacing=0.18), one_band(), tail(70, 50, seed=2), 2, 200), (70, 120)),
    "B 1, 200 taps, fade 0 at a wave's end": (lambda: (BC.plain(), one_band(), tail(WAVE, 0, seed=3), 1, 200), (WAVE, WAVE)),
    "B 1, 200 taps, K1 == taps": (lambda: (BC.plain(), one_band(0.05), tail(100, 100, seed=4), 1, 200), (100, 200)),
    "B 3, L 255, 200 taps, K0 == taps": (lambda: (BC.plain(ear_spacing=0.18), three_bands((0.0, 0.05, 0.3)), tail(200, 10, seed=5), 2, 200), (200, 200)),
    "B 3, L 255, 4096 taps, marks across a tile's and two waves' ends, air on one band": (lambda: (BC.plain(ear_spacing=0.18), three_bands((0.0, 0.0, 0.3)), tail(250, 80, seed=6), 2, 4096), (250, 330)),
    "B 3, L 255, 4096 taps, K1 == taps": (lambda: (BC.plain(ear_spacing=0.18), three_bands(), tail(3000, 5000, seed=7), 2, 4096), (3000, 4096)),
    "B 3, L 255, 4096 taps, pure diffuse, a dead band": (lambda: (BC.plain(ear_spacing=0.18), three_bands((0.0, 0.01, 0.05), dead=2), tail(0, 0, seed=8), 2, 4096), (0, 0)),
    "B 3, L 255, 6001 taps, K0 < D": (lambda: (BC.plain(), three_bands(), tail(50, 950, seed=9), 1, 6001), (50, 1000)),
    "B 3, L 255, 6001 taps, fade 0, min_order 3": (lambda: (BC.plain(ear_spacing=0.18, min_order=3), three_bands((0.0, 0.05, 0.3)), tail(1500, 0, seed=0xFFFFFFFF), 2, 6001), (1500, 1500)),
    "B 1, 6001 taps, fade from tap 0, gain 0.5, rotated": (lambda: (BC.rotated(), one_band(), tail(0, 777, seed=10, gain=0.5), 2, 6001), (0, 777)),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    d, bands, t, channels, taps = CASES[name][0]()
    out = T.ir(d, bands, t, channels, taps, RATE)
    out.h.setflags(write=False)
    return d, bands, t, channels, taps, out


# The HRTF call: 8 x 3 cells of 32 taps at 2048 taps, B = 3, L = 255; `delta`: unit-impulse HRIRs of 4 taps.
HRTF_GRID = BC.HRTF_GRID
HRTF_TAPS = 2048
HRTF_MARKS = (600, 1000)


@functools.lru_cache(maxsize=None)
def hrtf_reference(delta=False):
    n_az, n_el = HRTF_GRID
    d = CS.describe()
    bands = three_bands((0.0, 0.05, 0.3))
    t = tail(HRTF_MARKS[0], HRTF_MARKS[1] - HRTF_MARKS[0], seed=21)
    hrir = T.BR.delta_set(n_az * n_el, 4) if delta else CS.noise_set(21, n_az * n_el, 32)
    out = T.brir(d, bands, t, hrir, n_az, n_el, HRTF_TAPS, RATE)
    out.h.setflags(write=False)
    hrir.setflags(write=False)
    return d, bands, t, hrir, n_az, n_el, HRTF_TAPS, out
