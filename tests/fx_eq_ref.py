"""Independent numpy restatement of GAS_FX_EQ6 / _EQ10 / _EQ21 (the header of csrc/k_fx_eq.hip):
[ENGINE] AudioEffectEQInstance::process over EQ::BandProcess, from recollection of the engine source -- parity
unpinned, like SURVEY Appendix B.

Coefficients per band are computed in f64 from the mix rate and rounded to f32.  Sequential in the engine's order: one
frame at a time, vectorised over sources x bands x ears, every product and sum a separate f32 operation, the band sum
in band order.  x is float32 [n][F][2]; settings is a gas_fx_eq_settings array [n]; j is the chain position whose gains
apply.
"""
import numpy as np

f32, f64 = np.float32, np.float64
DB2LIN = 0.11512925464970228
EQ6, EQ10, EQ21 = 16, 17, 18
FREQS = {
    EQ6: (32.0, 100.0, 320.0, 1000.0, 3200.0, 10000.0),
    EQ10: (31.25, 62.5, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0, 16000.0),
    EQ21: (22.0, 32.0, 44.0, 63.0, 90.0, 125.0, 175.0, 250.0, 350.0, 500.0, 700.0, 1000.0, 1400.0, 2000.0, 2800.0, 4000.0, 5600.0, 8000.0, 11000.0, 16000.0, 22000.0),
}


def db2lin_block(db):
    return np.exp(np.asarray(db, f64) * DB2LIN).astype(f32)


def band_geometry(kind, mix_rate):
    """Per band: centre f, lower edge frq_l, th = 2 pi f / sr, th_l = 2 pi frq_l / sr (f64)."""
    f = np.array(FREQS[kind], f64)
    lf = np.log2(f)
    gaps = np.diff(lf)
    octave = np.empty_like(f)
    octave[0], octave[-1] = gaps[0], gaps[-1]
    octave[1:-1] = (gaps[:-1] + gaps[1:]) * 0.5
    frq_l = np.round(f / 2.0 ** (octave / 2.0))
    sr = f64(f32(mix_rate))
    return f, frq_l, 2.0 * np.pi * f / sr, 2.0 * np.pi * frq_l / sr


def coefficients(kind, mix_rate, as_f64=False):
    """(c1, c2, c3) per band; a band with a == 0 or a negative discriminant gets 0, 0, 0 (the engine leaves it unset)."""
    _, _, th, th_l = band_geometry(kind, mix_rate)
    s = 0.5
    ct, ctl, stl = np.cos(th), np.cos(th_l), np.sin(th_l)
    a = s * ct * ct - 2.0 * s * ctl * ct + s - stl * stl
    b = 2.0 * s * ctl * ctl + s * ct * ct - 2.0 * s * ctl * ct - s + stl * stl
    c = 0.25 * s * ct * ct - 0.5 * s * ctl * ct + 0.25 * s - 0.25 * stl * stl
    disc = b * b - 4.0 * a * c
    ok = (a != 0.0) & (disc >= 0.0)
    r1 = np.where(ok, (-b + np.sqrt(np.where(ok, disc, 0.0))) / np.where(ok, 2.0 * a, 1.0), 0.0)
    c1 = np.where(ok, 2.0 * (0.5 - r1) / 2.0, 0.0)
    c2 = np.where(ok, 2.0 * r1, 0.0)
    c3 = np.where(ok, 2.0 * (0.5 + r1) * ct, 0.0)
    if as_f64:
        return c1, c2, c3, ok
    return c1.astype(f32), c2.astype(f32), c3.astype(f32), ok


def response(c1, c2, c3, w):
    """H_k(e^{jw}) = c1 (1 - z^-2) / (1 - c3 z^-1 + c2 z^-2) per band (f64, complex); w broadcasts against the bands."""
    z1 = np.exp(-1j * np.asarray(w, f64))
    return np.asarray(c1, f64) * (1.0 - z1 * z1) / (1.0 - np.asarray(c3, f64) * z1 + np.asarray(c2, f64) * z1 * z1)


class EqStage:
    """State of one equaliser at chain position j for n sources: a2, a3, b2, b3 per source, band and ear (f32)."""

    def __init__(self, kind, j, n, mix_rate=48000.0):
        self.kind, self.j = kind, j
        self.c1, self.c2, self.c3, _ = coefficients(kind, mix_rate)
        self.B = len(FREQS[kind])
        self.h = np.zeros((4, n, self.B, 2), f32)  # a2, a3, b2, b3

    def reset(self, s):
        self.h[:, s] = 0

    def block(self, x, settings):
        x = np.asarray(x, f32)
        n, F, _ = x.shape
        B = self.B
        g = db2lin_block(settings["band_gain_db"][:, self.j, :B])[:, :, None]  # [n][B][1]
        c1, c2, c3 = (c[None, :, None] for c in (self.c1, self.c2, self.c3))
        a2, a3, b2, b3 = self.h
        y = np.empty((n, F, 2), f32)
        for t in range(F):
            xt = x[:, t, None, :]  # [n][1][2]
            b1 = ((c1 * (xt - a3)) + (c3 * b2)) - (c2 * b3)
            a3, a2 = a2, np.broadcast_to(xt, a2.shape).astype(f32)
            b3, b2 = b2, b1
            p = b1 * g
            acc = np.zeros((n, 2), f32)
            for k in range(B):
                acc = acc + p[:, k]
            y[:, t] = acc
        self.h = np.stack([a2, a3, b2, b3])
        return y


def eq_f64(x, c1, c2, c3, gains):
    """The same recurrence in f64 from rest (coefficients and gains as given): [n][F][2] -> [n][F][2]."""
    x = np.asarray(x, f64)
    n, F, _ = x.shape
    c1, c2, c3 = (np.asarray(c, f64)[None, :, None] for c in (c1, c2, c3))
    g = np.asarray(gains, f64)[:, :, None]
    B = c1.shape[1]
    a2 = np.zeros((n, B, 2))
    a3, b2, b3 = a2.copy(), a2.copy(), a2.copy()
    y = np.empty((n, F, 2))
    for t in range(F):
        xt = x[:, t, None, :]
        b1 = c1 * (xt - a3) + c3 * b2 - c2 * b3
        a3, a2 = a2, np.broadcast_to(xt, a2.shape)
        b3, b2 = b2, b1
        y[:, t] = (b1 * g).sum(axis=1)
    return y


def draw_settings(rng, n, capi, lo=-60.0, hi=24.0):
    """Gains over the whole property range at every position and band."""
    s = capi.fx_eq_settings_defaults(n)
    s["band_gain_db"] = rng.uniform(lo, hi, size=s["band_gain_db"].shape).astype(f32)
    return s
