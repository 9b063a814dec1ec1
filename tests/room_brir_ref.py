"""gas_conv_ir_from_room_hrtf: the rule of include/gas_amd.h in numpy float64 on top of tests/room_ir_ref.py (its
geometry, its candidates and their v and pos for one receiver), with np.add.at on int64 per HRIR tap.

It shares nothing with the kernel but the rule.  Every operation is float64 in the order the header states, so the
int64 sums can be expected to agree with the device's to the bit wherever the two libraries' atan2 pick the same cell.
They may legitimately differ where an image's direction lies on the edge between two cells or on the vertical axis,
where the azimuth is ill-conditioned.  brir() counts such images as near_edge, and the tests require near_edge == 0 of
every case they compare: a condition on the inputs, not a tolerance.

brir() returns a Brir: acc int64 [2][taps], h float32 [2][taps], mono (the room_ir_ref.Ir of the same descriptor with
one channel), dirs (the cell of every candidate, in mono's candidate order), in_range (candidates that reach a tap) and
near_edge (in-range candidates for which az / 2 pi n_az or (el + pi / 2) / pi (n_el - 1) lies within EDGE of a
half-integer, or flat < EDGE |p|)."""
import numpy as np

import room_ir_ref as R

ONE = R.ONE
EDGE = 1e-6
TWO_PI = 6.2831853071795864769252867666
MAX_DIRS = 65536
MAX_HRIR_TAPS = 256
MAX_HRIR_ABS = 4.0


class Brir:
    pass


def llround(x):
    """C's llround: halves away from zero."""
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int64)


def cells(p, n_az, n_el):
    """Step 3 from the direction p = (p_x, p_y, p_z) [n] each in the listener's frame -> (dir int64 [n], near bool [n])."""
    px, py, pz = (np.asarray(v, np.float64) for v in p)
    az = np.arctan2(px, -pz)
    flat = np.sqrt(px * px + pz * pz)
    el = np.arctan2(py, flat)
    x = az / TWO_PI * float(n_az)
    y = (el + TWO_PI / 4) / (TWO_PI / 2) * float(n_el - 1)
    ai = llround(x)
    ai = ((ai % n_az) + n_az) % n_az
    ei = llround(y) if n_el > 1 else np.zeros(len(px), np.int64)
    ei = np.clip(ei, 0, n_el - 1)
    norm = np.sqrt(px * px + py * py + pz * pz)
    near = (np.abs(x - np.floor(x) - 0.5) < EDGE) | (np.abs(y - np.floor(y) - 0.5) < EDGE) | (flat < EDGE * norm)
    return ei * n_az + ai, near


def directions(desc, mono, taps, mix_rate):
    """w = img - l per candidate of `mono`, taken through room.basis and the listener's basis transposed -> (p_x, p_y, p_z)."""
    d = np.asarray(desc).reshape(-1)[0]
    s, l, _, _, h, _, _, _ = R.geometry(desc, 1, taps, mix_rate)
    m = mono.m
    w = [2.0 * m[:, a].astype(np.float64) * h[a] + np.where(np.abs(m[:, a]) & 1, -s[a], s[a]) - l[a] for a in range(3)]
    B = d["room"]["basis"].astype(np.float64)
    L = d["listener"]["basis"].astype(np.float64)
    g = [B[a][0] * w[0] + B[a][1] * w[1] + B[a][2] * w[2] for a in range(3)]
    return [L[0][a] * g[0] + L[1][a] * g[1] + L[2][a] * g[2] for a in range(3)]


def brir(desc, hrir, n_az, n_el, taps, mix_rate, orders=None):
    """hrir float32 [n_az * n_el][2][hrir_taps]; orders as room_ir_ref.ir's."""
    hrir = np.asarray(hrir)
    assert hrir.dtype == np.float32 and hrir.ndim == 3 and hrir.shape[:2] == (n_az * n_el, 2)
    assert 1 <= n_az * n_el <= MAX_DIRS and 1 <= hrir.shape[2] <= MAX_HRIR_TAPS
    assert np.isfinite(hrir).all() and np.abs(hrir).max() <= MAX_HRIR_ABS
    T = hrir.shape[2]
    d = np.asarray(desc).reshape(-1)[0]
    mono = R.ir(desc, 1, taps, mix_rate, orders=orders)
    # step 2
    v, pos = mono.v[0], mono.pos[0]
    kf = np.floor(pos)
    f = pos - kf
    k = kf.astype(np.int64)
    a0, a1 = v * (1.0 - f), v * f
    # step 3
    dirs, near = cells(directions(desc, mono, taps, mix_rate), n_az, n_el)
    reaches = (k >= -1) & (k < taps)
    # step 4
    H = np.zeros((hrir.shape[0], 2, T + 2))
    H[:, :, 1 : T + 1] = hrir.astype(np.float64)  # H[.., j + 1] is tap j; taps -1 and T are 0
    out = Brir()
    out.acc = np.zeros((2, taps), np.int64)
    for e in range(2):
        He = H[dirs, e]
        for j in range(T + 1):
            g = a0 * He[:, j + 1] + a1 * He[:, j]
            t = k + j
            ok = (t >= 0) & (t < taps)
            np.add.at(out.acc[e], t[ok], np.rint(g[ok] * ONE).astype(np.int64))
    # step 5
    out.h = (float(d["room"]["level"]) * out.acc.astype(np.float64) * (1.0 / ONE)).astype(np.float32)
    out.mono, out.dirs = mono, dirs
    out.in_range = int(np.count_nonzero(reaches))
    out.near_edge = int(np.count_nonzero(near & reaches))
    return out


def delta_set(n_dirs, taps=1):
    """H[d][e][0] = 1 and nothing else: every image arrives as the one-channel rule places it."""
    h = np.zeros((n_dirs, 2, taps), np.float32)
    h[:, :, 0] = 1.0
    return h
