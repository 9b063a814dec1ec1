"""The inputs tests/test_gpu_room_brir.py compares against tests/room_brir_ref.py, kept apart from it so that
tests/test_room_brir_reference.py can require near_edge == 0 of every one of them without a GPU.

A case is name -> (descriptor, hrir float32 [n_az * n_el][2][hrir_taps], n_az, n_el, taps); reference(name) computes
room_brir_ref.brir once per process and shares it read-only.  The room is test_gpu_room_ir.py's 5 x 4 x 3 m box: a few
hundred images at 2048 taps, a few thousand at 4096.  The listener stands at (-1, 0.25, -0.5) with its axes a little off
the room's (TURN), so that no image lies on the listener's vertical axis or on a cell's edge by symmetry."""
import functools

import numpy as np

import er_rooms_ref as E
import room_brir_ref as BR
import room_ir_ref as R

RATE = 48000.0
SRC, LIS = (1.0, 0.5, 0.25), (-1.0, 0.25, -0.5)


def rotation(yaw, pitch, roll):
    """An orthonormal basis (float64) from three angles, columns = the local axes in the global frame."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Y = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    P = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Z = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Y @ P @ Z


TURN = rotation(0.31, -0.17, 0.11)


def small_room(refl=(0.9, 0.85, 0.8, 0.75, 0.7, 0.95), level=1.0):
    room = E.unit_room(half_extent=(2.5, 2.0, 1.5), level=level)
    room["reflectance"] = [list(refl)]
    return room


def describe(room=None, listener_basis=TURN, **kw):
    return R.describe(small_room() if room is None else room, SRC, LIS, listener_basis=listener_basis, **kw)


def rotated():
    """A rotated room off the origin and a listener turned another way."""
    rng = np.random.default_rng(7)
    room = small_room(level=0.8)
    B = E.random_basis(rng)
    origin = np.array([3.0, -7.0, 11.0])
    room["basis"], room["origin"] = B, origin
    return R.describe(room, origin + B @ np.array(SRC), origin + B @ np.array(LIS), listener_basis=E.random_basis(rng))


def closet():
    """0.7 x 0.6 x 0.5 m: a hundred taps (0.71 m of extra path) still hold a dozen images and more."""
    room = E.unit_room(half_extent=(0.35, 0.3, 0.25))
    room["reflectance"] = [[0.9, 0.85, 0.8, 0.75, 0.7, 0.95]]
    return R.describe(room, (0.15, 0.1, 0.05), (-0.15, 0.05, -0.1), listener_basis=TURN)


def noise_set(seed, n_dirs, taps, negative=False):
    """Decaying noise below 4 in magnitude, a different row for every direction and ear."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n_dirs, 2, taps)) * np.exp(-np.arange(taps) / 32.0)
    if negative:
        h = -np.abs(h) - 0.01
    return np.clip(h, -4.0, 4.0).astype(np.float32)


CASES = {
    "2048 taps, 12x5, 32 hrir taps": lambda: (describe(), noise_set(1, 60, 32), 12, 5, 2048),
    "1 hrir tap": lambda: (describe(), noise_set(2, 60, 1), 12, 5, 2048),
    "7 hrir taps": lambda: (describe(), noise_set(3, 60, 7), 12, 5, 2048),
    "256 hrir taps": lambda: (describe(), noise_set(4, 60, 256), 12, 5, 2048),
    "100 taps under 256 hrir taps": lambda: (closet(), noise_set(5, 60, 256), 12, 5, 100),
    "4096 taps, rotated, 16x7, 256 hrir taps": lambda: (rotated(), noise_set(6, 112, 256), 16, 7, 4096),
    "one elevation": lambda: (describe(), noise_set(7, 12, 32), 12, 1, 2048),
    "one azimuth": lambda: (describe(), noise_set(8, 5, 32), 1, 5, 2048),
    "min_order 3": lambda: (describe(min_order=3), noise_set(9, 60, 32), 12, 5, 2048),
    "max_order 3": lambda: (describe(max_order=3), noise_set(10, 60, 32), 12, 5, 2048),
    "one dead wall": lambda: (describe(small_room(refl=(0.9, 0.85, 0.0, 0.75, 0.7, 0.95))), noise_set(11, 60, 32), 12, 5, 2048),
    "64x16": lambda: (describe(), noise_set(12, 1024, 32), 64, 16, 2048),
    "negative throughout": lambda: (describe(), noise_set(13, 60, 32, negative=True), 12, 5, 2048),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    d, hrir, n_az, n_el, taps = CASES[name]()
    out = BR.brir(d, hrir, n_az, n_el, taps, RATE)
    out.h.setflags(write=False)
    out.acc.setflags(write=False)
    hrir.setflags(write=False)
    return d, hrir, n_az, n_el, taps, out


# The direct sound's cell against gas_calc_spatialization's hrtf_dir: listener orientations (yaw, pitch, roll).
ORIENTATIONS = [(0.0, 0.0, 0.0), (0.31, -0.17, 0.11), (2.4, 0.5, -0.3), (-1.9, -0.8, 0.2), (3.0, 0.05, 1.2), (-0.6, 1.1, 2.5)]
DIRECT_GRID = (12, 5)


def calc_spatialization_cell(source, listener_origin, basis, n_az, n_el):
    """The cell k_calc_spatialization picks: the local position in float32 (rel, then basis^T rel, sums in row order), the
    angles in float64 -> (dir, near an edge)."""
    b = np.asarray(basis, np.float32)
    rel = np.asarray(source, np.float32) - np.asarray(listener_origin, np.float32)
    p = [np.float32(np.float32(np.float32(b[0][a] * rel[0]) + np.float32(b[1][a] * rel[1])) + np.float32(b[2][a] * rel[2])) for a in range(3)]
    dirs, near = BR.cells([np.array([float(v)]) for v in p], n_az, n_el)
    return int(dirs[0]), bool(near[0])
