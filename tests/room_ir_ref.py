"""gas_conv_ir_from_room: the rule of include/gas_amd.h in numpy float64, vectorised over the candidate box, with
np.add.at on int64.

It shares nothing with the kernel but the rule.  Inputs are the float32 values the device is given, widened; every
operation after that is float64, written out in the order the header states (sums in x, y, z order, products left to
right), so that the int64 sums can be expected to agree with the device's to the bit -- the tests only ask for
helpers.TOL.  A reflectance's power is a running product (R_a[m] = R_a[m -+ 1] * the wall that step meets), never pow().

ir() returns an Ir: acc int64 [channels][taps] (the sums of step 5), h float32 [channels][taps] (step 6), N (the box of
step 2, clamped), cells = (2 N_x + 1)(2 N_y + 1)(2 N_z + 1), candidates (triples that pass the masks), in_range
(candidates that reach a tap of channel 0), and per candidate m [n][3] and, per channel, pos and v of step 4."""
import numpy as np

from er_rooms_ref import ROOM_DTYPE  # noqa: F401  (one layout for gas_room)

LISTENER_DTYPE = np.dtype([("basis", np.float32, (3, 3)), ("origin", np.float32, (3,)), ("velocity", np.float32, (3,)), ("pad", np.float32)])
ROOM_IR_DTYPE = np.dtype([("room", ROOM_DTYPE), ("source", np.float32, (3,)), ("listener", LISTENER_DTYPE), ("ear_spacing", np.float32), ("min_order", np.uint32), ("max_order", np.uint32)])
MAX_CELLS = 1 << 28
MIN_D0 = 1e-3
ONE = float(1 << 32)


class Ir:
    pass


def describe(room, source, listener_origin, listener_basis=None, ear_spacing=0.0, min_order=0, max_order=0):
    """A ROOM_IR_DTYPE scalar array ([1]) from a ROOM_DTYPE room ([1] or scalar)."""
    d = np.zeros(1, ROOM_IR_DTYPE)
    d["room"] = np.asarray(room).reshape(-1)[0]
    d["source"] = source
    d["listener"]["basis"] = np.eye(3) if listener_basis is None else listener_basis
    d["listener"]["origin"] = listener_origin
    d["ear_spacing"] = ear_spacing
    d["min_order"], d["max_order"] = min_order, max_order
    return d


def _bt(B, v):
    """basis^T v with each sum in row order."""
    return np.array([B[0][a] * v[0] + B[1][a] * v[1] + B[2][a] * v[2] for a in range(3)])


def geometry(desc, channels, taps, mix_rate, nudge=(0.0, 0.0, 0.0)):
    """Steps 1 and 2 -> (s, l, [e_0 (, e_1)], d0, h, c, rate, N_free): N_free is step 2's N before max_order clamps it.
    nudge: float64 metres added to the widened source, for steps smaller than float32 can state."""
    d = np.asarray(desc).reshape(-1)[0]
    room = d["room"]
    B = room["basis"].astype(np.float64)
    o, h = room["origin"].astype(np.float64), room["half_extent"].astype(np.float64)
    c, rate = float(room["speed_of_sound"]), float(np.float32(mix_rate))
    s = _bt(B, d["source"].astype(np.float64) + np.asarray(nudge, np.float64) - o)
    l = _bt(B, d["listener"]["origin"].astype(np.float64) - o)
    r = _bt(B, d["listener"]["basis"].astype(np.float64)[:, 0])
    dx, dy, dz = s - l
    d0 = float(np.sqrt(dx * dx + dy * dy + dz * dz))
    half = float(d["ear_spacing"]) / 2.0
    ears = [l] if channels == 1 else [l - half * r, l + half * r]
    reach = c * float(taps) / rate + d0 + (half if channels == 2 else 0.0)
    n_free = [int(np.floor(reach / (2.0 * h[a]))) + 1 for a in range(3)]
    return s, l, ears, d0, h, c, rate, n_free


def box(desc, channels, taps, mix_rate):
    """-> (N, cells): step 2's box with the clamp to max_order, and the number of its cells (the refusal compares this
    with MAX_CELLS)."""
    d = np.asarray(desc).reshape(-1)[0]
    n = geometry(desc, channels, taps, mix_rate)[7]
    mo = int(d["max_order"])
    if mo:
        n = [min(v, mo) for v in n]
    return n, (2 * n[0] + 1) * (2 * n[1] + 1) * (2 * n[2] + 1)


def _power_table(neg, pos, n):
    """[2 n + 1], index m + n: the +a wall's reflectance p times and the -a wall's q times, as a running product."""
    t = np.ones(2 * n + 1)
    for m in range(1, n + 1):
        t[n + m] = t[n + m - 1] * (pos if m & 1 else neg)
        t[n - m] = t[n - m + 1] * (neg if m & 1 else pos)
    return t


def ir(desc, channels, taps, mix_rate, orders=None, keep=None, nudge=(0.0, 0.0, 0.0)):
    """orders = (lo, hi) replaces the descriptor's order mask; hi None = no upper limit.  (0, 0) is the direct sound
    alone, which the interface cannot ask for (its max_order 0 means no limit).  keep(m_x, m_y, m_z) -> bool, over
    broadcastable int64 arrays, removes further candidates.  nudge: see geometry()."""
    d = np.asarray(desc).reshape(-1)[0]
    keep_fn = keep
    s, l, ears, d0, h, c, rate, n_free = geometry(desc, channels, taps, mix_rate, nudge)
    if orders is None:
        lo, hi = int(d["min_order"]), (int(d["max_order"]) or None)
    else:
        lo, hi = orders
    N = [v if hi is None else min(v, hi) for v in n_free]
    refl = d["room"]["reflectance"].astype(np.float64)
    level = float(d["room"]["level"])
    m = [np.arange(-n, n + 1, dtype=np.int64) for n in N]
    am = [np.abs(v) for v in m]
    order = am[0][:, None, None] + am[1][None, :, None] + am[2][None, None, :]
    keep = order >= lo
    if hi is not None:
        keep &= order <= hi
    if keep_fn is not None:
        keep = keep & keep_fn(m[0][:, None, None], m[1][None, :, None], m[2][None, None, :])
    ix, iy, iz = np.nonzero(keep)
    img = [2.0 * m[a].astype(np.float64) * h[a] + np.where(am[a] & 1, -s[a], s[a]) for a in range(3)]
    T = [_power_table(refl[2 * a], refl[2 * a + 1], N[a]) for a in range(3)]
    R = (T[0][ix] * T[1][iy]) * T[2][iz]
    out = Ir()
    out.acc = np.zeros((channels, taps), np.int64)
    out.N, out.cells, out.candidates = N, (2 * N[0] + 1) * (2 * N[1] + 1) * (2 * N[2] + 1), len(ix)
    out.d0, out.rate, out.c = d0, rate, c
    out.m = np.stack([m[0][ix], m[1][iy], m[2][iz]], axis=1)
    out.pos, out.v = [], []
    for e, ear in enumerate(ears):
        dx, dy, dz = img[0][ix] - ear[0], img[1][iy] - ear[1], img[2][iz] - ear[2]
        dist = np.sqrt(dx * dx + dy * dy + dz * dz)
        v = R * d0 / np.maximum(dist, d0)
        pos = (dist - d0) / c * rate
        k = np.floor(pos)
        f = pos - k
        k = k.astype(np.int64)
        for kk, share in ((k, v * (1.0 - f)), (k + 1, v * f)):
            ok = (kk >= 0) & (kk < taps)
            np.add.at(out.acc[e], kk[ok], np.rint(share[ok] * ONE).astype(np.int64))
        if e == 0:
            out.in_range = int(np.count_nonzero((k + 1 >= 0) & (k < taps)))
        out.pos.append(pos)
        out.v.append(v)
    out.h = (level * out.acc.astype(np.float64) * (1.0 / ONE)).astype(np.float32)
    return out
