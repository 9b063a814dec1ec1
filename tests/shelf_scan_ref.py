"""References for the two arithmetic forms of a one-biquad filter stage (kinds 1 and 4 .. 8):

- Biquad64: the recurrence in float64 on the f32 coefficients the kernels use (fx_filter_ref.coefficients at one
  stage), vectorised over sources, history carried between blocks.  What both forms are measured against.
- ShelfScan: a numpy float32 model of k_shelf_scan.hip's scan branch, steps 1-4 of that file's header comment: lane l
  owns frames [P l, P l + P) (P = F / 64), its response from rest, the two homogeneous solutions p and q, the affine
  recurrence s_l = M s_(l-1) + c_l over the 64 lanes solved by a six-step doubling scan with M squared every step, then
  y = w + p s.x + q s.y.  The kernel's fused multiply-adds are modelled as a float64 product and sum rounded to f32 once
  (the product of two f32 is exact in f64; the sum then rounds twice instead of once), so the model is NOT bit-exact to
  the GPU: it follows the kernel's association and the growth of its error, not its last bit.
- the engine-order f32 restatement is fx_filter_ref.FilterStage at db = 0; there is no second one here.

Also the filter populations the gate tests draw (the CPU and the GPU tests share them) and the float64 peak gain of a
filter's all-pole part, the quantity the scan's error follows."""
import numpy as np

import fx_filter_ref as ref

f32, f64 = np.float32, np.float64
LANES = 64
MIX_RATE = 48000.0
# chain kinds (gas_amd.h) by fx_filter_ref type
HS, LP, HP, BP, NOTCH, LSH = 1, 4, 5, 6, 7, 8
TYPE_OF_KIND = {LP: ref.LOWPASS, HP: ref.HIGHPASS, BP: ref.BANDPASS, NOTCH: ref.NOTCH, LSH: ref.LOWSHELF, HS: ref.HIGHSHELF}


def coefficients(kinds, cutoff, resonance, gain, mix_rate=MIX_RATE):
    """-> [n][5] f32 (b0, b1, b2, a1, a2): the kernels' coefficient bits of one stage per source."""
    return np.array([ref.coefficients(TYPE_OF_KIND[int(k)], mix_rate, c, r, g, 1) for k, c, r, g in zip(kinds, cutoff, resonance, gain)], f32)


def allpole_peak_gain(co, grid=1 << 16):
    """max over w of 1 / |1 - a1 e^-jw - a2 e^-2jw| in f64 on a dense grid that is refined around its maximum (a pole
    pair next to z = 1 makes a peak far narrower than any uniform grid)."""
    co = np.atleast_2d(np.asarray(co, f64))
    a1, a2 = co[:, 3, None], co[:, 4, None]

    def mag2(w):
        z1 = np.exp(-1j * w)
        return np.abs(1.0 - a1 * z1 - a2 * z1 * z1) ** 2

    lo, hi = np.zeros((len(co), 1)), np.full((len(co), 1), np.pi)
    best = np.full(len(co), np.inf)
    per = 1 << 10
    for it in range(4):
        m = grid if it == 0 else per
        w = lo + (hi - lo) * (np.arange(m + 1) / m)[None]
        v = mag2(w)
        k = v.argmin(axis=1)
        best = np.minimum(best, v[np.arange(len(co)), k])
        step = (hi - lo) / m
        wk = w[np.arange(len(co)), k][:, None]
        lo, hi = np.maximum(wk - step, 0.0), np.minimum(wk + step, np.pi)
    with np.errstate(divide="ignore"):  # f32 rounding can put a pole ON the unit circle (20 Hz shelves): gain inf
        return 1.0 / np.sqrt(best)


class Biquad64:
    """y = b0 x + b1 x[-1] + b2 x[-2] + a1 y[-1] + a2 y[-2] in f64 for n sources and both ears."""

    def __init__(self, co):
        self.co = np.asarray(co, f32).astype(f64)
        self.h = np.zeros((4, len(self.co), 2), f64)  # y[-1], y[-2], x[-1], x[-2]

    def block(self, x):
        x = np.asarray(x, f32).astype(f64)
        b0, b1, b2, a1, a2 = (self.co[:, k, None] for k in range(5))
        y1, y2, x1, x2 = self.h
        out = np.empty_like(x)
        for t in range(x.shape[1]):
            v = x[:, t]
            yi = v * b0 + x1 * b1 + x2 * b2 + y1 * a1 + y2 * a2
            y2, x2, x1, y1 = y1, x1, v, yi
            out[:, t] = yi
        self.h = np.stack([y1, y2, x1, x2])
        return out


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


class ShelfScan:
    """The scan branch of k_shelf_scan.hip / k_hrtf_uni<FLT> in float32 for n sources (see the module docstring)."""

    def __init__(self, co):
        self.co = np.asarray(co, f32)
        n = len(self.co)
        self.ha1, self.ha2, self.hb1, self.hb2 = (np.zeros((n, 2), f32) for _ in range(4))

    def block(self, x):
        x = np.asarray(x, f32)
        n, F, _ = x.shape
        assert F % (2 * LANES) == 0
        P = F // LANES
        b0, b1, b2, a1, a2 = (self.co[:, k] for k in range(5))
        # homogeneous solutions: p from state (1, 0), q from state (0, 1); the same in every lane and for both ears
        p, q = np.empty((P, n), f32), np.empty((P, n), f32)
        p[0], q[0] = a1, a2
        p[1], q[1] = _fma(a1, p[0], a2), a1 * q[0]
        for k in range(2, P):
            p[k] = _fma(a1, p[k - 1], a2 * p[k - 2])
            q[k] = _fma(a1, q[k - 1], a2 * q[k - 2])
        xl = x.reshape(n, LANES, P, 2)
        c = lambda v: v[:, None, None]  # noqa: E731  per source -> [n][lane][ear]
        # 1 + 2: u and the lane's response from rest
        xm1 = np.concatenate([self.hb1[:, None], xl[:, :-1, P - 1]], axis=1)  # [n][lane][ear]: the frame in front of the lane's first
        xm2 = np.concatenate([self.hb2[:, None], xl[:, :-1, P - 2]], axis=1)
        w = np.empty((n, LANES, P, 2), f32)
        w1 = np.zeros((n, LANES, 2), f32)
        w2 = np.zeros((n, LANES, 2), f32)
        for k in range(P):
            xa = xl[:, :, k - 1] if k >= 1 else xm1
            xb = xl[:, :, k - 2] if k >= 2 else (xm1 if k == 1 else xm2)
            u = _fma(c(b2), xb, _fma(c(b1), xa, c(b0) * xl[:, :, k]))
            wk = _fma(c(a2), w2, _fma(c(a1), w1, u))
            w[:, :, k] = wk
            w2, w1 = w1, wk
        # 3: s_l = M s_(l-1) + c_l, inclusive scan over the lanes; lane 0's c absorbs the processor's history
        sx, sy = w[:, :, P - 1].copy(), w[:, :, P - 2].copy()
        e = lambda v: v[:, None]  # noqa: E731  per source -> [n][ear]
        sx[:, 0] = _fma(e(p[P - 1]), self.ha1, _fma(e(q[P - 1]), self.ha2, sx[:, 0]))
        sy[:, 0] = _fma(e(p[P - 2]), self.ha1, _fma(e(q[P - 2]), self.ha2, sy[:, 0]))
        m00, m01, m10, m11 = p[P - 1].copy(), q[P - 1].copy(), p[P - 2].copy(), q[P - 2].copy()
        d = 1
        while d < LANES:
            ox, oy = sx[:, :-d].copy(), sy[:, :-d].copy()
            sx[:, d:], sy[:, d:] = _fma(c(m00), ox, _fma(c(m01), oy, sx[:, d:])), _fma(c(m10), ox, _fma(c(m11), oy, sy[:, d:]))
            n00, n01 = _fma(m00, m00, m01 * m10), _fma(m00, m01, m01 * m11)
            n10, n11 = _fma(m10, m00, m11 * m10), _fma(m10, m01, m11 * m11)
            m00, m01, m10, m11 = n00, n01, n10, n11
            d *= 2
        # 4: the state entering each lane, applied to its response from rest
        ix = np.concatenate([self.ha1[:, None], sx[:, :-1]], axis=1)
        iy = np.concatenate([self.ha2[:, None], sy[:, :-1]], axis=1)
        y = np.empty_like(w)
        for k in range(P):
            y[:, :, k] = _fma(c(p[k]), ix, _fma(c(q[k]), iy, w[:, :, k]))
        self.ha1, self.ha2 = y[:, -1, P - 1].copy(), y[:, -1, P - 2].copy()
        self.hb1, self.hb2 = xl[:, -1, P - 1].copy(), xl[:, -1, P - 2].copy()
        return y.reshape(n, F, 2)


def filter_settings(capi, kinds, cutoff, resonance, gain):
    """The populations' draws as fx_filter_ref.FilterStage settings at position 0, 6 dB (one stage)."""
    s = capi.fx_filter_settings_defaults(len(kinds))
    s["type"][:, 0] = [TYPE_OF_KIND[int(k)] for k in kinds]
    s["db"][:, 0] = 0
    s["cutoff_hz"][:, 0], s["resonance"][:, 0], s["gain"][:, 0] = cutoff, resonance, gain
    return s


# ------------------------------------------------------------------------------------------------------------ populations
def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(f32)


def population(name, n=512):
    """-> (kinds [n] int, cutoff, resonance, gain [n] f32) at 48 kHz, fixed seeds:
    A  over-damped: LP, HP, BP, NOTCH in turn, cutoff log-uniform 30 .. 2000 Hz, resonance log-uniform 0.01 .. 0.3
    B  shelves near z = 1: LSH, cutoff log-uniform 60 .. 1000 Hz, resonance 0.2 .. 0.6, gain log-uniform 0.05 .. 1.5
    C  the high shelf of gas_params (resonance 1): cutoff log-uniform 20 .. 20500 Hz, gain log-uniform 0.001 .. 4
    D  control: LP, HP, BP, NOTCH, LSH in turn, 800 .. 12000 Hz, resonance 0.4 .. 1.2, gain log-uniform 0.1 .. 3"""
    rng = np.random.default_rng({"A": 7101, "B": 7102, "C": 7103, "D": 7104}[name])
    one = np.ones(n, f32)
    if name == "A":
        return np.resize([LP, HP, BP, NOTCH], n), _logu(rng, 30.0, 2000.0, n), _logu(rng, 0.01, 0.3, n), one
    if name == "B":
        return np.full(n, LSH), _logu(rng, 60.0, 1000.0, n), rng.uniform(0.2, 0.6, n).astype(f32), _logu(rng, 0.05, 1.5, n)
    if name == "C":
        return np.full(n, HS), _logu(rng, 20.0, 20500.0, n), one, _logu(rng, 0.001, 4.0, n)
    if name == "D":
        return np.resize([LP, HP, BP, NOTCH, LSH], n), _logu(rng, 800.0, 12000.0, n), rng.uniform(0.4, 1.2, n).astype(f32), _logu(rng, 0.1, 3.0, n)
    raise ValueError(name)


# settings named in ADVICE.md and DESIGN.md 3.5 (a): (kind, cutoff, resonance, gain); every one is ill-conditioned
NAMED = {
    "LP 200 Hz Q 0.1": (LP, 200.0, 0.1, 1.0),
    "HP 90 Hz Q 0.05": (HP, 90.0, 0.05, 1.0),
    "LP 50 Hz Q 0.02": (LP, 50.0, 0.02, 1.0),
    "LSH 427 Hz Q 0.31 gain 0.79": (LSH, 427.0, 0.31, 0.79),
    "BP 100 Hz Q 0.05": (BP, 100.0, 0.05, 1.0),
}
# well-conditioned settings the scan must keep: the resource defaults and a mid low-pass
CONTROL = {
    "LP 2000 Hz Q 0.5": (LP, 2000.0, 0.5, 1.0),
    "HS 5000 Hz": (HS, 5000.0, 1.0, 0.25),
    "LP 1500 Hz Q 0.7": (LP, 1500.0, 0.7, 1.0),
}
# a setting that looks as harmless and is not: all-pole peak gain 98 (two poles at radius 0.928, 6 degrees from z = 1).
# As a low-pass the scan model is off by 6e-6 of the peak, as the high-pass or notch with the SAME a1, a2 by 1.0e-5 to
# 1.5e-5, and the gate sees a1 and a2 only: it goes serial.
BORDERLINE = {"LP 800 Hz Q 0.7": (LP, 800.0, 0.7, 1.0)}


def row_error(y, y64):
    """[n]: the largest deviation of a source's block from the f64 rows over that block's f64 peak."""
    y64 = np.asarray(y64, f64)
    err = np.abs(np.asarray(y, f64) - y64).max(axis=(1, 2))
    return err / np.maximum(np.abs(y64).max(axis=(1, 2)), 1e-30)
