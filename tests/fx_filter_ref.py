"""Numpy restatement of GAS_FX_FILTER (k_fx_filter.hip): the engine's AudioEffectFilter of any subclass
at FILTER_6DB .. FILTER_24DB and AudioEffectBandLimitFilter, as recalled (parity with the engine's source is unpinned).

Coefficients: AudioFilterSW::prepare_coefficients in f64 `math`, members stored f32, then normalised by a0 with the
feedback terms negated; the stage correction of Q and gain comes after the mode's Q tweak and the gain clamp, before
alpha.  Cascade: a float32 loop, per frame processors 0 .. stages - 1 of the ear with process_one in the engine's
operation order; processors from `stages` up are not run and keep their history."""
import math

import numpy as np

f32, f64 = np.float32, np.float64

LOWPASS, HIGHPASS, BANDPASS, NOTCH, LOWSHELF, HIGHSHELF, BANDLIMIT = range(7)
TYPES = (LOWPASS, HIGHPASS, BANDPASS, NOTCH, LOWSHELF, HIGHSHELF, BANDLIMIT)
MAX_STAGES = 4
TAU = 6.2831853071795864769252867666
LN2 = 0.6931471805599453


def coefficients(ftype, mix_rate, cutoff_hz, resonance, gain, stages):
    """-> (b0, b1, b2, a1, a2) as f32.  mix_rate, cutoff_hz, resonance and gain are taken as the f32 the library holds."""
    sr32 = f32(mix_rate)
    sr = float(sr32)
    cutoff, res, g = float(f32(cutoff_hz)), float(f32(resonance)), float(f32(gain))
    if ftype == BANDLIMIT:
        hi = res
        center = (cutoff + res) / 2.0
        bw = (math.log(center) - math.log(hi)) / LN2
        omega = TAU * center / sr
        sin_v, cos_v = math.sin(omega), math.cos(omega)
        alpha = sin_v * math.sinh(LN2 / 2.0 * bw * omega / sin_v)
        a0 = 1.0 + alpha
        m = [f32(alpha), f32(0.0), f32(-alpha), f32(-2.0 * cos_v), f32(1.0 - alpha)]
    else:
        sr_limit = int(sr32 / f32(2)) + 512
        final_cutoff = float(sr_limit) if cutoff > sr_limit else cutoff
        if final_cutoff < 1:
            final_cutoff = 1.0
        omega = TAU * final_cutoff / sr
        sin_v, cos_v = math.sin(omega), math.cos(omega)
        Q = res
        if Q <= 0.0:
            Q = 0.0001
        if ftype == BANDPASS:
            Q *= 2.0
        tmpgain = g
        if tmpgain < 0.001:
            tmpgain = 0.001
        if stages > 1:
            Q = math.pow(Q, 1.0 / stages) if Q > 1.0 else Q
            tmpgain = math.pow(tmpgain, 1.0 / (stages + 1))
        alpha = sin_v / (2 * Q)
        a0 = 1.0 + alpha
        if ftype == LOWPASS:
            m = [f32((1.0 - cos_v) / 2.0), f32(1.0 - cos_v), f32((1.0 - cos_v) / 2.0), f32(-2.0 * cos_v), f32(1.0 - alpha)]
        elif ftype == HIGHPASS:
            m = [f32((1.0 + cos_v) / 2.0), f32(-(1.0 + cos_v)), f32((1.0 + cos_v) / 2.0), f32(-2.0 * cos_v), f32(1.0 - alpha)]
        elif ftype == BANDPASS:
            m = [f32(alpha * math.sqrt(Q + 1)), f32(0.0), f32(-alpha * math.sqrt(Q + 1)), f32(-2.0 * cos_v), f32(1.0 - alpha)]
        elif ftype == NOTCH:
            m = [f32(1.0), f32(-2.0 * cos_v), f32(1.0), f32(-2.0 * cos_v), f32(1.0 - alpha)]
        else:
            tmpq = math.sqrt(Q)
            if tmpq <= 0:
                tmpq = 0.001
            beta = math.sqrt(tmpgain) / tmpq
            if ftype == LOWSHELF:
                a0 = (tmpgain + 1.0) + (tmpgain - 1.0) * cos_v + beta * sin_v
                m = [
                    f32(tmpgain * ((tmpgain + 1.0) - (tmpgain - 1.0) * cos_v + beta * sin_v)),
                    f32(2.0 * tmpgain * ((tmpgain - 1.0) - (tmpgain + 1.0) * cos_v)),
                    f32(tmpgain * ((tmpgain + 1.0) - (tmpgain - 1.0) * cos_v - beta * sin_v)),
                    f32(-2.0 * ((tmpgain - 1.0) + (tmpgain + 1.0) * cos_v)),
                    f32((tmpgain + 1.0) + (tmpgain - 1.0) * cos_v - beta * sin_v),
                ]
            elif ftype == HIGHSHELF:
                a0 = (tmpgain + 1.0) - (tmpgain - 1.0) * cos_v + beta * sin_v
                m = [
                    f32(tmpgain * ((tmpgain + 1.0) + (tmpgain - 1.0) * cos_v + beta * sin_v)),
                    f32(-2.0 * tmpgain * ((tmpgain - 1.0) + (tmpgain + 1.0) * cos_v)),
                    f32(tmpgain * ((tmpgain + 1.0) + (tmpgain - 1.0) * cos_v - beta * sin_v)),
                    f32(2.0 * ((tmpgain - 1.0) - (tmpgain + 1.0) * cos_v)),
                    f32((tmpgain + 1.0) - (tmpgain - 1.0) * cos_v - beta * sin_v),
                ]
            else:
                raise ValueError(ftype)
    b0, b1, b2 = (f32(float(v) / a0) for v in m[:3])
    a1, a2 = (f32(float(v) / (0.0 - a0)) for v in m[3:])
    return b0, b1, b2, a1, a2


def response(co, w):
    """H(e^{jw}) of one stage with coefficients (b0, b1, b2, a1, a2) in the stored convention (feedback negated)."""
    b0, b1, b2, a1, a2 = (float(v) for v in co)
    z1 = np.exp(-1j * np.asarray(w, f64))
    return (b0 + b1 * z1 + b2 * z1 * z1) / (1.0 - a1 * z1 - a2 * z1 * z1)


def settings_coefficients(settings, j, mix_rate):
    """-> ([n][5] f32 coefficients, [n] stages) of chain position j."""
    n = len(settings)
    co = np.empty((n, 5), f32)
    st = settings["db"][:, j].astype(np.int64) + 1
    cache = {}
    for i in range(n):
        key = (int(settings["type"][i, j]), float(settings["cutoff_hz"][i, j]), float(settings["resonance"][i, j]), float(settings["gain"][i, j]), int(st[i]))
        if key not in cache:
            cache[key] = coefficients(key[0], mix_rate, key[1], key[2], key[3], key[4])
        co[i] = cache[key]
    return co, st


class FilterStage:
    """State of one GAS_FX_FILTER at chain position j for n sources: h[n][stage][a1, a2, b1, b2][ear] (f32)."""

    def __init__(self, j, n, mix_rate=48000.0):
        self.j, self.mix_rate = j, mix_rate
        self.h = np.zeros((n, MAX_STAGES, 4, 2), f32)

    def reset(self, s):
        self.h[s] = 0

    def block(self, x, settings):
        x = np.asarray(x, f32)
        n, F, _ = x.shape
        co, stages = settings_coefficients(settings, self.j, self.mix_rate)
        cb0, cb1, cb2, ca1, ca2 = (co[:, k, None] for k in range(5))  # [n][1]
        h = self.h
        y = np.empty((n, F, 2), f32)
        top = int(stages.max())
        on = [(stages > s)[:, None] for s in range(top)]
        for t in range(F):
            v = x[:, t]
            for s in range(top):
                a1, a2, b1, b2 = h[:, s, 0], h[:, s, 1], h[:, s, 2], h[:, s, 3]
                yi = v * cb0 + b1 * cb1 + b2 * cb2 + a1 * ca1 + a2 * ca2  # f32, left to right
                m = on[s]
                h[:, s, 1] = np.where(m, a1, a2)
                h[:, s, 3] = np.where(m, b1, b2)
                h[:, s, 2] = np.where(m, v, b1)
                h[:, s, 0] = np.where(m, yi, a1)
                v = np.where(m, yi, v)
            y[:, t] = v
        return y


def cascade_f64(x, co, stages):
    """`stages` equal stages with coefficients co from rest, all in f64: [F][2] -> [F][2]."""
    b0, b1c, b2c, a1c, a2c = (float(v) for v in co)
    v = np.asarray(x, f64)
    for _ in range(stages):
        a1 = a2 = b1 = b2 = np.zeros(2)
        out = np.empty_like(v)
        for t in range(len(v)):
            yi = v[t] * b0 + b1 * b1c + b2 * b2c + a1 * a1c + a2 * a2c
            a2, b2, b1, a1 = a1, b1, v[t], yi
            out[t] = yi
        v = out
    return v


def draw_settings(rng, n, capi, types=TYPES, dbs=(0, 1, 2, 3), lo_hz=20.0, hi_hz=20500.0):
    """Every position: a type and slope from the given sets, cutoff log-uniform, resonance and gain over their ranges
    (the band limit's resonance stays above 0.01: it is refused at 0)."""
    s = capi.fx_filter_settings_defaults(n)
    shape = s["type"].shape
    s["type"] = rng.choice(np.asarray(types), size=shape)
    s["db"] = rng.choice(np.asarray(dbs), size=shape)
    s["cutoff_hz"] = np.exp(rng.uniform(np.log(lo_hz), np.log(hi_hz), size=shape)).astype(f32)
    s["resonance"] = rng.uniform(0.01, 1.0, size=shape).astype(f32)
    s["gain"] = rng.uniform(0.0, 4.0, size=shape).astype(f32)
    return s
