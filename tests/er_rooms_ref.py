"""gas_calc_early_reflections: the rule of include/gas_amd.h in numpy float64, vectorised over the sources, and the
scenes the tests feed it.

It shares nothing with the kernel but the rule: the candidates come out of itertools and a sort, the selection is a plain
stable argsort of -g (so ties go to the lower candidate number), there are no ranks and no lanes.  Inputs are the float32
values the device is given, widened; every operation after that is float64.

Besides the taps it returns what a comparison with a float32 implementation needs to know about each source:
  fr        of the selected candidates (frames, before rounding): a delay may differ by one where fr is within
            BORDER of k + 0.5;
  gap       the relative gaps between consecutive gains among the nine largest: where one is below NEAR_TIE, float32
            may order (or, at the eighth / ninth, select) the candidates differently;
  drop_edge a candidate with a non-zero gain whose fr is within BORDER of M + 0.5: float32 may drop it where float64
            keeps it, or the other way round.  Such a source is treated like a near tie.
BORDER = 0.01 frames is about six times the error float32 makes in fr at these coordinates (0.0016 frames in a numpy
float32 restatement over 4000 sources of scene()); the gains of that restatement differed by 5e-7 relative, far below
NEAR_TIE = 1e-4."""
import itertools

import numpy as np

ER_TAPS = 8
ROOM_NONE = 0xFFFFFFFF
BORDER = 0.01
NEAR_TIE = 1e-4
GAIN_RTOL = 3e-5  # the band of test_gpu_calc_spatialization.py

ROOM_DTYPE = np.dtype([("basis", np.float32, (3, 3)), ("origin", np.float32, (3,)), ("half_extent", np.float32, (3,)), ("reflectance", np.float32, (6,)), ("speed_of_sound", np.float32), ("level", np.float32), ("max_order", np.uint32)])

# rule 4: the 24 triples with 1 <= |m|_1 <= 2, ascending in (|m|_1, m_x, m_y, m_z)
TRIPLES = sorted((m for m in itertools.product(range(-2, 3), repeat=3) if 1 <= sum(abs(a) for a in m) <= 2), key=lambda m: (sum(abs(a) for a in m),) + m)
assert len(TRIPLES) == 24


class Taps:
    """gain float64 [n][8], delay int64 [n][8], cand int64 [n][8] (candidate numbers, by rank), fr float64 [n][8], gap
    float64 [n][8], border bool [n][8], near_tie bool [n]; g_all / delay_all / fr_all / dist_all [n][24] by candidate,
    d0 [n], outside bool [n]."""

    def params_like(self, dtype):
        out = np.zeros(len(self.gain), dtype)
        out["gain"], out["delay"] = self.gain, self.delay
        return out


def frac_border(fr):
    """|frac(fr) - 0.5| < BORDER: fr lies next to a rounding border of rint."""
    return np.abs(fr - np.floor(fr) - 0.5) < BORDER


def taps(rooms, positions, listener_origin, mix_rate, frames, ring_frames, room_index=None):
    rooms = np.asarray(rooms).reshape(-1)
    pos = np.asarray(positions, np.float32).astype(np.float64).reshape(-1, 3)
    lis = np.asarray(listener_origin, np.float32).astype(np.float64).reshape(3)
    n = len(pos)
    ri = np.zeros(n, np.int64) if room_index is None else np.asarray(room_index).astype(np.uint32).astype(np.int64)
    none = ri == ROOM_NONE
    assert np.all(none | (ri < len(rooms)))
    r = rooms[np.where(none, 0, ri)]
    B = r["basis"].astype(np.float64)
    o, h = r["origin"].astype(np.float64), r["half_extent"].astype(np.float64)
    refl = r["reflectance"].astype(np.float64)
    c, level = r["speed_of_sound"].astype(np.float64), r["level"].astype(np.float64)
    M = ring_frames - frames
    # 1: basis^T v
    s = np.einsum("nra,nr->na", B, pos - o)
    l = np.einsum("nra,nr->na", B, lis[None, :] - o)
    # 2
    outside = none | (np.abs(s) > h).any(axis=1) | (np.abs(l) > h).any(axis=1)
    # 3
    d0 = np.sqrt(((s - l) ** 2).sum(axis=1))
    # 4, 5
    m = np.array(TRIPLES, np.int64)[None, :, :]  # [1][24][3]
    am = np.abs(m)
    img = 2.0 * m * h[:, None, :] + np.where(am % 2 == 1, -s[:, None, :], s[:, None, :])
    dist = np.sqrt(((img - l[:, None, :]) ** 2).sum(axis=2))
    hi, lo = (am + 1) // 2, am // 2
    p, q = np.where(m > 0, hi, lo), np.where(m > 0, lo, hi)
    R = np.prod(refl[:, None, 1::2] ** p * refl[:, None, 0::2] ** q, axis=2)  # 0 ** 0 == 1
    with np.errstate(divide="ignore", invalid="ignore"):
        g = level[:, None] * R * d0[:, None] / dist
        fr = (dist - d0[:, None]) / c[:, None] * float(np.float32(mix_rate))
    delay_raw = np.rint(fr)  # ties to even
    # 6
    order = am.sum(axis=2)
    drop = outside[:, None] | (order > r["max_order"].astype(np.int64)[:, None]) | ~(dist > 0) | ~np.isfinite(g) | (delay_raw > M)
    kept_edge = ~drop & (g > 0) & (np.abs(fr - (M + 0.5)) < BORDER)
    lost_edge = ~outside[:, None] & (order <= r["max_order"].astype(np.int64)[:, None]) & (delay_raw > M) & (np.abs(fr - (M + 0.5)) < BORDER) & (R > 0) & (level[:, None] > 0)
    g = np.where(drop, 0.0, g)
    delay = np.where(g > 0, np.maximum(np.nan_to_num(delay_raw, nan=1.0, posinf=1.0, neginf=1.0), 1.0), 1.0).astype(np.int64)
    # 7
    idx = np.argsort(-g, axis=1, kind="stable")
    first9 = np.take_along_axis(g, idx[:, : ER_TAPS + 1], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(first9[:, :-1] > 0, (first9[:, :-1] - first9[:, 1:]) / first9[:, :-1], np.inf)
    sel = idx[:, :ER_TAPS]
    t = Taps()
    t.cand = sel
    t.gain = np.take_along_axis(g, sel, axis=1)
    t.delay = np.take_along_axis(delay, sel, axis=1)
    t.fr = np.take_along_axis(fr, sel, axis=1)
    t.border = frac_border(t.fr) & (t.gain > 0)
    t.gap = gap
    t.drop_edge = (kept_edge | lost_edge).any(axis=1)
    t.near_tie = (gap < NEAR_TIE).any(axis=1) | t.drop_edge
    t.g_all, t.delay_all, t.fr_all, t.dist_all = g, delay, fr, dist
    t.d0, t.outside = d0, outside
    return t


def random_basis(rng):
    """A random rotation (orthonormal, determinant +1), float64."""
    q, rr = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(rr))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def scene(rng, n, n_rooms=8, max_order=2, with_none=0.0):
    """(rooms ROOM_DTYPE [n_rooms], room_index uint32 [n], positions float32 [n][3], listener_origin float32 [3]).
    Half-extents uniform in 1.5 .. 12 m, reflectances 0.3 .. 0.95, c = 343, level 0.5 .. 1, random orthonormal bases,
    origins within +-20 m.  The rooms overlap at the listener, which lies uniformly inside 0.98 of every box, so that
    one listener gives every room's sources reflections; each source lies uniformly inside 0.98 of its room's box.
    with_none: the share of sources with GAS_ROOM_NONE."""
    lis = rng.uniform(-6.0, 6.0, 3)
    rooms = np.zeros(n_rooms, ROOM_DTYPE)
    bases = []
    for k in range(n_rooms):
        while True:
            h = rng.uniform(1.5, 12.0, 3)
            b = random_basis(rng)
            origin = lis - b @ (rng.uniform(-0.98, 0.98, 3) * h)
            if np.all(np.abs(origin) <= 20.0):
                break
        bases.append(b)
        rooms[k]["basis"], rooms[k]["origin"], rooms[k]["half_extent"] = b, origin, h
        rooms[k]["reflectance"] = rng.uniform(0.3, 0.95, 6)
        rooms[k]["speed_of_sound"] = 343.0
        rooms[k]["level"] = rng.uniform(0.5, 1.0)
        rooms[k]["max_order"] = max_order
    ri = rng.integers(0, n_rooms, n).astype(np.uint32)
    local = rng.uniform(-0.98, 0.98, (n, 3)) * rooms["half_extent"][ri].astype(np.float64)
    B = rooms["basis"][ri].astype(np.float64)
    pos = np.einsum("nra,na->nr", B, local) + rooms["origin"][ri].astype(np.float64)
    if with_none > 0:
        ri[rng.random(n) < with_none] = ROOM_NONE
    return rooms, ri, pos.astype(np.float32), lis.astype(np.float32)


def unit_room(half_extent=(4.0, 2.5, 3.0), reflectance=0.8, level=1.0, max_order=2, c=343.0):
    """One room with the identity basis at the origin."""
    r = np.zeros(1, ROOM_DTYPE)
    r["basis"] = np.eye(3)
    r["half_extent"] = half_extent
    r["reflectance"] = reflectance
    r["speed_of_sound"] = c
    r["level"] = level
    r["max_order"] = max_order
    return r
