"""gas_conv_ir_from_room_diffuse and gas_conv_ir_from_room_hrtf_diffuse: the rule of include/gas_amd.h in numpy float64.

It shares nothing with the kernel but the rule.  The specular band sums of step 2 are tests/room_ir_ref.py's
(room_brir_ref.py's for the HRTF call) for an IR of K1 taps, one descriptor per band; steps 1 and 3 - 6 are written out
here (uint64 arithmetic that wraps, np.rint for llrint), and step 7 is tests/room_bands_ref.py's steps 2 - 5 over the
mixed sums.

ir() and brir() return room_bands_ref's Bands over acc' (h, y, u, acc, F, L, D, lam) with, in addition: K0, K1, ws, wd
(step 1), spec int64 [B][channels][K1] (step 2), rho, mu [B] and s0 (step 3), xi, f float64 [channels][taps] (step 4),
d float64 [B][channels][taps] (step 5)."""
import numpy as np

import room_bands_ref as BD
import room_brir_ref as BR
import room_ir_ref as R

ROOM_TAIL_DTYPE = np.dtype([("seed", np.uint32), ("mix_time_s", np.float32), ("fade_s", np.float32), ("gain", np.float32), ("reserved", np.uint32, (4,))])
S0_MAX = 1024.0
XI_DEN = float(np.sqrt(65536.0 * 65536.0 - 1.0))
M64 = (1 << 64) - 1


def describe(seed=0, mix_time_s=0.0, fade_s=0.0, gain=1.0):
    """A ROOM_TAIL_DTYPE scalar array ([1])."""
    t = np.zeros(1, ROOM_TAIL_DTYPE)
    t["seed"], t["mix_time_s"], t["fade_s"], t["gain"] = seed, mix_time_s, fade_s, gain
    return t


def marks(tail, taps, mix_rate):
    """Step 1 -> (K0, K1)."""
    t = np.asarray(tail).reshape(-1)[0]
    rate = float(np.float32(mix_rate))
    k0 = min(int(taps), int(np.rint(min(float(t["mix_time_s"]) * rate, 2.0**31))))
    k1 = min(int(taps), k0 + int(np.rint(min(float(t["fade_s"]) * rate, 2.0**31))))
    return k0, k1


def weights(k0, k1, taps):
    """Step 1 -> (ws, wd) float64 [taps]."""
    k = np.arange(taps, dtype=np.float64)
    kf = float(k1 - k0)
    x = np.where(k < k0, 0.0, np.where(k >= k1, 1.0, (k - k0) / (kf if kf else 1.0)))
    return np.sqrt(1.0 - x), np.sqrt(x)


def hash_scalar(seed, e, k):
    """Step 4's z for one (seed, e, k), in Python integers."""
    z = ((seed << 32) | (e << 24) | k) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hash_taps(seed, e, taps):
    """Step 4's z for k = 0 .. taps - 1, uint64 [taps]."""
    with np.errstate(over="ignore"):
        z = np.uint64((int(seed) << 32) | (int(e) << 24)) | np.arange(taps, dtype=np.uint64)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def numerator(z):
    """2 (u_0 + u_1 + u_2) - 196605 as int64."""
    z = np.asarray(z, np.uint64)
    u = [((z >> np.uint64(16 * i)) & np.uint64(0xFFFF)).astype(np.int64) for i in range(3)]
    return 2 * (u[0] + u[1] + u[2]) - 196605


def noise(seed, e, taps):
    """Step 4 -> (xi, f) float64 [taps]."""
    z = hash_taps(seed, e, taps)
    xi = numerator(z).astype(np.float64) / XI_DEN
    f = (((z >> np.uint64(48)) & np.uint64(0xFFFF)).astype(np.float64) + 0.5) / 65536.0
    return xi, f


def decay(desc, bands, tail, d0, c, rate):
    """Step 3 -> (rho [B], mu [B], s0)."""
    d = np.asarray(desc).reshape(-1)[0]
    bd = np.asarray(bands).reshape(-1)[0]
    t = np.asarray(tail).reshape(-1)[0]
    h = d["room"]["half_extent"].astype(np.float64)
    V = 8.0 * h[0] * h[1] * h[2]
    A = [4.0 * h[1] * h[2], 4.0 * h[0] * h[2], 4.0 * h[0] * h[1]]
    S = 2.0 * (A[0] + A[1] + A[2])
    rho, mu = [], []
    for b in range(int(bd["n_bands"])):
        r = bd["reflectance"][b].astype(np.float64)
        rho.append((A[0] * (r[0] * r[0] + r[1] * r[1]) + A[1] * (r[2] * r[2] + r[3] * r[3]) + A[2] * (r[4] * r[4] + r[5] * r[5])) / S)
        mu.append(np.inf if rho[-1] == 0.0 else -np.log(rho[-1]) * S / (4.0 * V))
    with np.errstate(over="ignore", invalid="ignore"):
        s0 = float(t["gain"]) * np.sqrt(((4.0 * np.pi * c) * (d0 * d0)) / (V * rate))
    return rho, mu, float(s0)


def _mix(desc, bands, tail, spec, channels, taps, d0, c, rate, k0, k1):
    """Steps 3 - 7 from the specular sums spec [B][channels][K1] (None when K1 == 0)."""
    bd = np.asarray(bands).reshape(-1)[0]
    t = np.asarray(tail).reshape(-1)[0]
    B = int(bd["n_bands"])
    rho, mu, s0 = decay(desc, bands, tail, d0, c, rate)
    assert np.isfinite(s0) and s0 <= S0_MAX
    ws, wd = weights(k0, k1, taps)
    k = np.arange(taps, dtype=np.float64)
    r = d0 + c * k / rate
    xi, f = zip(*[noise(int(t["seed"]), e, taps) for e in range(channels)])
    xi, f = np.stack(xi), np.stack(f)
    dd = np.zeros((B, channels, taps))
    acc = np.zeros((B, channels, taps), np.int64)
    for b in range(B):
        for e in range(channels):
            if rho[b] != 0.0:
                a = (s0 * np.exp(-(mu[b] * r) / 2.0)) * xi[e]
                dd[b, e] = a * (1.0 - f[e])
                dd[b, e, 1:] += a[:-1] * f[e, :-1]
            acc[b, e] = np.rint((wd * dd[b, e]) * R.ONE).astype(np.int64)
            if k1:
                s = spec[b][e]
                acc[b, e, :k1] += np.where(np.arange(k1) < k0, s, np.rint(ws[:k1] * s.astype(np.float64)).astype(np.int64))
    out = BD._combine(desc, bands, list(acc), c, rate)
    out.K0, out.K1, out.ws, out.wd = k0, k1, ws, wd
    out.spec, out.rho, out.mu, out.s0, out.xi, out.f, out.d = spec, rho, mu, s0, xi, f, dd
    return out


def ir(desc, bands, tail, channels, taps, mix_rate, orders=None):
    bd = np.asarray(bands).reshape(-1)[0]
    k0, k1 = marks(tail, taps, mix_rate)
    _, _, _, d0, _, c, rate, _ = R.geometry(desc, channels, taps, mix_rate)
    spec = None
    if k1:
        spec = np.stack([R.ir(BD.band_descriptor(desc, bands, b), channels, k1, mix_rate, orders=orders).acc for b in range(int(bd["n_bands"]))])
    return _mix(desc, bands, tail, spec, channels, taps, d0, c, rate, k0, k1)


def brir(desc, bands, tail, hrir, n_az, n_el, taps, mix_rate, orders=None):
    bd = np.asarray(bands).reshape(-1)[0]
    k0, k1 = marks(tail, taps, mix_rate)
    _, _, _, d0, _, c, rate, _ = R.geometry(desc, 1, taps, mix_rate)
    spec, near = None, 0
    if k1:
        per_band = [BR.brir(BD.band_descriptor(desc, bands, b), hrir, n_az, n_el, k1, mix_rate, orders=orders) for b in range(int(bd["n_bands"]))]
        spec = np.stack([p.acc for p in per_band])
        near = max(p.near_edge for p in per_band)
    out = _mix(desc, bands, tail, spec, 2, taps, d0, c, rate, k0, k1)
    out.near_edge = near
    return out
