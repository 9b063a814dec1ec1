"""The inputs tests/test_gpu_room_bands.py compares against tests/room_bands_ref.py, kept apart from it so that
tests/test_room_bands_reference.py can check the conditions on them (near_edge == 0, results that are not silent)
without a GPU.

A case is name -> (descriptor, bands, channels, taps); reference(name) computes room_bands_ref.ir once per process and
shares it read-only.  The room is test_gpu_room_ir.py's 5 x 4 x 3 m box; every band has six reflectances of its own
(band b's are the base values times 1 - 0.09 b).  The combine kernel has two forms: below WIDE_FROM outputs (channels
times taps) a workgroup owns SMALL_TILE taps, from there on TILE taps.  The tile cases stand one below, at and one above
a tile's end in each form and on both sides of WIDE_FROM; the long ones keep max_order = 2 (25 images), so that their
references cost a convolution and no lattice."""
import functools

import numpy as np

import er_rooms_ref as E
import room_bands_ref as BD
import room_brir_cases as CS
import room_ir_ref as R

RATE = 48000.0
SRC, LIS = CS.SRC, CS.LIS
TILE, SMALL_TILE, WIDE_FROM = 1792, 256, 1 << 19
BASE = (0.9, 0.85, 0.8, 0.75, 0.7, 0.95)
OCTAVES = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0)


def walls(n):
    """[n][6], all different."""
    return [[v * (1.0 - 0.09 * b) for v in BASE] for b in range(n)]


def small_room(level=1.0):
    return CS.small_room(level=level)


def rotated():
    """test_gpu_room_ir.py's rotated room off the origin, a listener turned another way."""
    rng = np.random.default_rng(7)
    room = small_room(level=0.8)
    B = E.random_basis(rng)
    origin = np.array([3.0, -7.0, 11.0])
    room["basis"], room["origin"] = B, origin
    return R.describe(room, origin + B @ np.array(SRC), origin + B @ np.array(LIS), listener_basis=E.random_basis(rng), ear_spacing=0.18)


def plain(**kw):
    return R.describe(small_room(), SRC, LIS, **kw)


CASES = {
    "B 2, L 63, one channel, 2000 taps": lambda: (plain(), BD.describe(walls(2), (2000.0,), filter_taps=63), 1, 2000),
    "B 3, L 255, two channels, 2049 taps, air": lambda: (plain(ear_spacing=0.18), BD.describe(walls(3), (500.0, 4000.0), (0.0, 0.05, 0.3), 255), 2, 2049),
    "B 8, L 1023, octaves, min_order 3": lambda: (plain(ear_spacing=0.18, min_order=3), BD.describe(walls(8), OCTAVES, filter_taps=1023), 2, 2000),
    "B 2, L 4095, 100 taps (taps < D)": lambda: (CS.closet(), BD.describe(walls(2), (1000.0,), (0.0, 0.1), 4095), 1, 100),
    "B 2, L 3, one tap": lambda: (plain(), BD.describe(walls(2), (2000.0,), filter_taps=3), 1, 1),
    "B 3, L 255, 16384 taps, rotated": lambda: (rotated(), BD.describe(walls(3), (500.0, 4000.0), (0.0, 0.01, 0.05), 255), 2, 16384),
    "narrow form, one below a tile": lambda: (plain(), BD.describe(walls(2), (2000.0,), filter_taps=63), 1, 8 * SMALL_TILE - 1),
    "narrow form, the tile": lambda: (plain(ear_spacing=0.18), BD.describe(walls(2), (2000.0,), filter_taps=63), 2, 8 * SMALL_TILE),
    "narrow form, one above a tile": lambda: (plain(), BD.describe(walls(2), (2000.0,), filter_taps=63), 1, 8 * SMALL_TILE + 1),
    "narrow form, the last size": lambda: (plain(max_order=2), BD.describe(walls(2), (2000.0,), (0.0, 0.001), 15), 1, WIDE_FROM - 1),
    "wide form, the first size": lambda: (plain(max_order=2), BD.describe(walls(2), (2000.0,), (0.0, 0.001), 15), 1, WIDE_FROM),
    "wide form, two channels, the first size": lambda: (plain(ear_spacing=0.18, max_order=2), BD.describe(walls(2), (2000.0,), (0.0, 0.001), 15), 2, WIDE_FROM // 2),
    "wide form, one below a tile": lambda: (plain(max_order=2), BD.describe(walls(2), (2000.0,), filter_taps=63), 1, 293 * TILE - 1),
    "wide form, the tile": lambda: (plain(max_order=2), BD.describe(walls(2), (2000.0,), filter_taps=63), 1, 293 * TILE),
    "wide form, one above a tile": lambda: (plain(max_order=2), BD.describe(walls(2), (2000.0,), filter_taps=63), 1, 293 * TILE + 1),
    "wide form, B 3, L 1023, air": lambda: (plain(max_order=2), BD.describe(walls(3), (500.0, 4000.0), (0.0, 0.002, 0.01), 1023), 1, WIDE_FROM + 5),
    "wide form, B 2, L 4095": lambda: (plain(ear_spacing=0.18, max_order=2), BD.describe(walls(2), (1000.0,), (0.0, 0.002), 4095), 2, WIDE_FROM // 2 + 3),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    d, bands, channels, taps = CASES[name]()
    out = BD.ir(d, bands, channels, taps, RATE)
    out.h.setflags(write=False)
    return d, bands, channels, taps, out


# The HRTF call: B = 3, L = 255, 2000 taps, 8 x 3 cells of 32 taps.
HRTF_GRID = (8, 3)


@functools.lru_cache(maxsize=None)
def hrtf_reference():
    n_az, n_el = HRTF_GRID
    d = CS.describe()
    bands = BD.describe(walls(3), (500.0, 4000.0), (0.0, 0.05, 0.3), 255)
    hrir = CS.noise_set(21, n_az * n_el, 32)
    out = BD.brir(d, bands, hrir, n_az, n_el, 2000, RATE)
    out.h.setflags(write=False)
    hrir.setflags(write=False)
    return d, bands, hrir, n_az, n_el, 2000, out
