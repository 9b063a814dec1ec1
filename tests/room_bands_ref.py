"""gas_conv_ir_from_room_bands and gas_conv_ir_from_room_hrtf_bands: the rule of include/gas_amd.h in numpy float64.

It shares nothing with the kernel but the rule.  The band sums of step 1 are tests/room_ir_ref.py's (room_brir_ref.py's
for the HRTF call), one descriptor per band with that band's reflectances; steps 2 - 5 are written out here.  The sums of
step 4 are numpy's (np.convolve), in its order, not the device's: the rule leaves the order open, and float64 sums of a
few thousand terms differ by parts in 1e-16 of their absolute sum, far below float32's last rounding.

ir() and brir() return a Bands: h float32 [channels][taps] (step 5), y float64 (step 4), u float64 [B][channels][taps]
(step 2), acc int64 [B][channels][taps] (step 1), F (step 3: a list of B float64 [L] rows), L, D, lam [B], and for brir()
near_edge, the largest room_brir_ref.near_edge over the bands (it depends on the geometry alone)."""
import numpy as np

import room_brir_ref as BR
import room_ir_ref as R

MAX_BANDS = 8
FILTER_MAX_TAPS = 4095
ROOM_BANDS_DTYPE = np.dtype([("n_bands", np.uint32), ("filter_taps", np.uint32), ("crossover_hz", np.float32, (MAX_BANDS - 1,)), ("reflectance", np.float32, (MAX_BANDS, 6)), ("air_db_per_m", np.float32, (MAX_BANDS,)), ("reserved", np.uint32)])
LN10 = 2.302585092994046


class Bands:
    pass


def describe(reflectance, crossover_hz=(), air_db_per_m=None, filter_taps=0):
    """A ROOM_BANDS_DTYPE scalar array ([1]): reflectance [B][6] (or [B], one value for all six walls)."""
    n = len(reflectance)
    assert 1 <= n <= MAX_BANDS and len(crossover_hz) == n - 1
    b = np.zeros(1, ROOM_BANDS_DTYPE)
    b["n_bands"], b["filter_taps"] = n, filter_taps
    b["crossover_hz"][0, : n - 1] = crossover_hz
    for i in range(n):
        b["reflectance"][0, i] = reflectance[i]
    b["air_db_per_m"][0, :n] = 0.0 if air_db_per_m is None else air_db_per_m
    return b


def filters(n_bands, filter_taps, crossover_hz, rate):
    """Step 3 -> (F, L, D): F is a list of n_bands float64 rows of L taps.  One band: L = 1, D = 0, F_0 = [1]."""
    if n_bands == 1:
        return [np.ones(1)], 1, 0
    L = int(filter_taps)
    assert L % 2 == 1 and 3 <= L <= FILTER_MAX_TAPS
    D = (L - 1) // 2
    j = np.arange(L, dtype=np.float64)
    w = 0.42 - 0.5 * np.cos(2.0 * np.pi * j / (L - 1)) + 0.08 * np.cos(4.0 * np.pi * j / (L - 1))
    x = j - D
    lp = []
    for i in range(n_bands - 1):
        nu = float(np.float32(crossover_hz[i])) / rate
        s = w * np.where(x == 0, 2.0 * nu, np.sin(2.0 * np.pi * nu * x) / (np.pi * np.where(x == 0, 1.0, x)))
        total = 0.0
        for v in s:  # ascending j
            total += float(v)
        lp.append(s / total)
    delta = np.zeros(L)
    delta[D] = 1.0
    F = [lp[0]] + [lp[b] - lp[b - 1] for b in range(1, n_bands - 1)] + [delta - lp[n_bands - 2]]
    return F, L, D


def band_descriptor(desc, bands, b):
    """`desc` with room.reflectance := bands.reflectance[b]."""
    d = np.asarray(desc).copy()
    d["room"]["reflectance"] = np.asarray(bands).reshape(-1)[0]["reflectance"][b]
    return d


def _combine(desc, bands, accs, c, rate):
    """Steps 2 - 5 from the band sums accs [B][channels][taps] int64."""
    bd = np.asarray(bands).reshape(-1)[0]
    B = int(bd["n_bands"])
    channels, taps = accs[0].shape
    out = Bands()
    out.F, out.L, out.D = filters(B, int(bd["filter_taps"]), bd["crossover_hz"], rate)
    out.acc = np.stack(accs)
    out.lam = [LN10 / 20.0 * float(bd["air_db_per_m"][b]) * c / rate for b in range(B)]
    k = np.arange(taps, dtype=np.float64)
    out.u = np.stack([(out.acc[b].astype(np.float64) * (1.0 / R.ONE)) * np.exp(-(out.lam[b] * k)) for b in range(B)])
    out.y = np.zeros((channels, taps))
    for b in range(B):
        for e in range(channels):
            out.y[e] += np.convolve(out.u[b, e], out.F[b])[out.D : out.D + taps]  # index t + D of the full convolution
    level = float(np.asarray(desc).reshape(-1)[0]["room"]["level"])
    out.h = (level * out.y).astype(np.float32)
    return out


def ir(desc, bands, channels, taps, mix_rate, orders=None):
    bd = np.asarray(bands).reshape(-1)[0]
    per_band = [R.ir(band_descriptor(desc, bands, b), channels, taps, mix_rate, orders=orders) for b in range(int(bd["n_bands"]))]
    return _combine(desc, bands, [p.acc for p in per_band], per_band[0].c, per_band[0].rate)


def brir(desc, bands, hrir, n_az, n_el, taps, mix_rate, orders=None):
    bd = np.asarray(bands).reshape(-1)[0]
    per_band = [BR.brir(band_descriptor(desc, bands, b), hrir, n_az, n_el, taps, mix_rate, orders=orders) for b in range(int(bd["n_bands"]))]
    out = _combine(desc, bands, [p.acc for p in per_band], per_band[0].mono.c, per_band[0].mono.rate)
    out.near_edge = max(p.near_edge for p in per_band)
    return out
