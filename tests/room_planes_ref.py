"""gas_conv_ir_from_planes: the rule of include/gas_amd.h in numpy float64, vectorised over the sequences of one order,
with np.add.at on int64.

It shares nothing with the kernel but the rule.  Inputs are the float32 values the device is given, widened; every
operation after that is float64, written out in the order the header states (dot(n, x) = (n_x x_x + n_y x_y) + n_z x_z,
products left to right), so that the int64 sums can be expected to agree with the device's to the bit -- the tests only
ask for helpers.TOL.  Sequences are grown order by order: every sequence of order K - 1 followed by each of the P - 1
other planes.

ir() returns an Ir: acc int64 [channels][taps] (the sums), h float32 [channels][taps], and what the tests and the timing
tool want to know about the case:
  candidates   sequences of every order asked for, P (P - 1)^(K - 1) each (the direct sound is not one of them)
  per_order    {K: candidates of order K}
  void         sequences with some t <= 0 in step 3
  valid        per receiver, the sequences whose path passed step 4
  margin       the smallest |dot(n_j, hit) - d_j|, j != q_i, met in step 4 by a path that was still valid when it got there
  v_min        the smallest v of a valid path that reached a tap (a path over a plane of reflectance 0 has v == 0, adds
               nothing to any tap and is not counted)
  left_early   sequences a lane may drop before step 4: void, R == 0, or some prefix image further from every receiver
               than c (taps + 1) / rate + d0"""
import numpy as np

LISTENER_DTYPE = np.dtype([("basis", np.float32, (3, 3)), ("origin", np.float32, (3,)), ("velocity", np.float32, (3,)), ("pad", np.float32)])
ROOM_PLANE_DTYPE = np.dtype([("normal", np.float32, (3,)), ("offset", np.float32), ("reflectance", np.float32)])
MAX_PLANES = 16
MAX_ORDER = 8
ROOM_PLANES_DTYPE = np.dtype([("planes", ROOM_PLANE_DTYPE, (MAX_PLANES,)), ("n_planes", np.uint32), ("speed_of_sound", np.float32), ("level", np.float32), ("source", np.float32, (3,)), ("listener", LISTENER_DTYPE), ("ear_spacing", np.float32), ("min_order", np.uint32), ("max_order", np.uint32)])
MAX_CANDIDATES = 1 << 28
MIN_D0 = 1e-3
ONE = float(1 << 32)


class Ir:
    pass


def describe(planes, source, listener_origin, listener_basis=None, ear_spacing=0.0, min_order=0, max_order=3, speed_of_sound=343.0, level=1.0):
    """A ROOM_PLANES_DTYPE array ([1]) from rows of (normal, offset, reflectance)."""
    d = np.zeros(1, ROOM_PLANES_DTYPE)
    d["n_planes"] = len(planes)
    for j, (n, off, refl) in enumerate(planes):
        d["planes"][0, j] = (n, off, refl)
    d["speed_of_sound"], d["level"] = speed_of_sound, level
    d["source"] = source
    d["listener"]["basis"] = np.eye(3) if listener_basis is None else listener_basis
    d["listener"]["origin"] = listener_origin
    d["ear_spacing"] = ear_spacing
    d["min_order"], d["max_order"] = min_order, max_order
    return d


def box_planes(origin, half_extent, reflectance):
    """An axis-aligned box as six rows for describe(), in gas_room's wall order -x, +x, -y, +y, -z, +z."""
    rows = []
    for a in range(3):
        for side, sign in ((0, 1.0), (1, -1.0)):
            n = [0.0, 0.0, 0.0]
            n[a] = sign
            rows.append((tuple(n), sign * origin[a] - half_extent[a], reflectance[2 * a + side]))
    return rows


def attic(reflectance=0.8, dead=None):
    """Seven planes: a floor at y = 0, walls at x = -+3 and z = -+4, two roof slopes from the eaves at y = 1.5 to a ridge
    at y = 3.5 above x = 0.  reflectance: one value or seven; dead: the index of one plane whose reflectance is 0."""
    k = 13.0**-0.5
    r = [reflectance] * 7 if np.isscalar(reflectance) else list(reflectance)
    if dead is not None:
        r[dead] = 0.0
    geo = [((0, 1, 0), 0.0), ((1, 0, 0), -3.0), ((-1, 0, 0), -3.0), ((0, 0, 1), -4.0), ((0, 0, -1), -4.0), ((-2 * k, -3 * k, 0), -10.5 * k), ((2 * k, -3 * k, 0), -10.5 * k)]
    return [(n, off, r[j]) for j, (n, off) in enumerate(geo)]


def _dot(n, x):
    return (n[..., 0] * x[..., 0] + n[..., 1] * x[..., 1]) + n[..., 2] * x[..., 2]


def geometry(desc, channels):
    """Step 1 -> (N [P][3], D [P], refl [P], s, [e_0 (, e_1)], d0)."""
    d = np.asarray(desc).reshape(-1)[0]
    P = int(d["n_planes"])
    raw = d["planes"]["normal"][:P].astype(np.float64)
    length = np.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])
    N = raw / length[:, None]
    D = d["planes"]["offset"][:P].astype(np.float64)
    refl = d["planes"]["reflectance"][:P].astype(np.float64)
    s = d["source"].astype(np.float64)
    l = d["listener"]["origin"].astype(np.float64)
    r = d["listener"]["basis"].astype(np.float64)[:, 0]
    dx, dy, dz = s - l
    d0 = float(np.sqrt((dx * dx + dy * dy) + dz * dz))
    half = float(d["ear_spacing"]) / 2.0
    ears = [l] if channels == 1 else [l - half * r, l + half * r]
    return N, D, refl, s, ears, d0


def count(P, lo, hi):
    """{K: P (P - 1)^(K - 1)} for max(lo, 1) <= K <= hi."""
    return {K: P * (P - 1) ** (K - 1) for K in range(max(lo, 1), hi + 1)}


def sequences(P, K):
    """int64 [P (P - 1)^(K - 1)][K]: every q with q_i != q_{i+1}."""
    seq = np.arange(P, dtype=np.int64)[:, None]
    for _ in range(K - 1):
        nxt = np.arange(P, dtype=np.int64)[None, :].repeat(len(seq), 0)
        keep = nxt != seq[:, -1:]
        seq = np.concatenate([seq.repeat(P, 0), nxt.reshape(-1, 1)], axis=1)[keep.reshape(-1)]
    return seq


def _add(acc_row, taps, img, ear, R, d0, c, rate, ok):
    """Step 5 for the rows of `ok` -> the v of those that added to a tap."""
    dx, dy, dz = img[:, 0] - ear[0], img[:, 1] - ear[1], img[:, 2] - ear[2]
    dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
    v = R * d0 / np.maximum(dist, d0)
    pos = (dist - d0) / c * rate
    k = np.floor(pos)
    f = pos - k
    k = k.astype(np.int64)
    for kk, share in ((k, v * (1.0 - f)), (k + 1, v * f)):
        hit = ok & (kk >= 0) & (kk < taps)
        np.add.at(acc_row, kk[hit], np.rint(share[hit] * ONE).astype(np.int64))
    return v[ok & (k + 1 >= 0) & (k < taps) & (v > 0)]


def ir(desc, channels, taps, mix_rate):
    d = np.asarray(desc).reshape(-1)[0]
    N, D, refl, s, ears, d0 = geometry(desc, channels)
    P = len(D)
    c, rate, level = float(d["speed_of_sound"]), float(np.float32(mix_rate)), float(d["level"])
    lo, hi = int(d["min_order"]), int(d["max_order"])
    reach = c * (float(taps) + 1.0) / rate + d0
    out = Ir()
    out.acc = np.zeros((channels, taps), np.int64)
    out.per_order = count(P, lo, hi)
    out.candidates = sum(out.per_order.values())
    out.void, out.left_early, out.valid = 0, 0, [0] * channels
    out.margin, out.v_min = np.inf, np.inf
    out.d0 = d0
    if lo == 0:  # the direct sound
        for e, ear in enumerate(ears):
            v = _add(out.acc[e], taps, s[None, :], ear, np.ones(1), d0, c, rate, np.ones(1, bool))
            out.v_min = min([out.v_min] + list(v))
    for K, n_seq in out.per_order.items():
        if n_seq == 0:
            continue
        seq = sequences(P, K)
        assert seq.shape == (n_seq, K)
        # step 3
        at = np.repeat(s[None, :], n_seq, 0)
        R = np.ones(n_seq)
        alive = np.ones(n_seq, bool)
        near = np.ones(n_seq, bool)
        imgs = []
        for i in range(K):
            q = seq[:, i]
            t = _dot(N[q], at) - D[q]
            alive &= t > 0
            at = at - (2.0 * t)[:, None] * N[q]
            R = R * refl[q]
            imgs.append(at)
            far = np.ones(n_seq, bool)
            for ear in ears:
                far &= np.sqrt(((at - ear) ** 2).sum(1)) > reach
            near &= ~far
        out.void += int(np.count_nonzero(~alive))
        out.left_early += int(np.count_nonzero(~alive | ~(R > 0) | ~near))
        # step 4
        for e, ear in enumerate(ears):
            p = np.repeat(ear[None, :], n_seq, 0)
            ok = alive.copy()
            for i in range(K - 1, -1, -1):
                q = seq[:, i]
                a = _dot(N[q], p) - D[q]
                b = _dot(N[q], imgs[i]) - D[q]
                ok &= a > 0
                with np.errstate(all="ignore"):
                    u = a / (a - b)
                    hit = p + u[:, None] * (imgs[i] - p)
                    inside = np.ones(n_seq, bool)
                    for j in range(P):
                        g = _dot(N[j][None, :], hit) - D[j]
                        other = ok & (q != j)
                        if other.any():
                            out.margin = min(out.margin, float(np.abs(g[other]).min()))
                        inside &= (g >= 0) | (q == j)
                ok &= inside
                p = hit
            out.valid[e] += int(np.count_nonzero(ok))
            v = _add(out.acc[e], taps, imgs[K - 1], ear, R, d0, c, rate, ok)
            if len(v):
                out.v_min = min(out.v_min, float(v.min()))
    out.h = (level * out.acc.astype(np.float64) * (1.0 / ONE)).astype(np.float32)
    return out
