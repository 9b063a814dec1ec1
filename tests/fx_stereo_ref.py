"""Independent numpy restatement of GAS_FX_PANNER, GAS_FX_STEREO_ENHANCE and GAS_FX_LIMITER (the
header of csrc/k_fx_stereo.hip): [ENGINE] AudioEffectPannerInstance::process, AudioEffectStereoEnhanceInstance::process
and AudioEffectLimiterInstance::process, from recollection of the engine source -- parity unpinned, like SURVEY
Appendix B.

Block constants in f64, rounded to f32 where the engine's C++ holds a float; every f32 product and sum a separate
operation in the engine's order; the limiter's per-sample log and exp in f64, rounded to f32.
x is float32 [n][F][2]; settings is a gas_fx_stereo_settings array [n]; j is the chain position whose settings apply.
"""
import numpy as np

f32, f64 = np.float32, np.float64
DB2LIN = 0.11512925464970228
LIN2DB = 8.685889638065035
PANNER, ENHANCE, LIMITER = 21, 22, 23


def db2lin_block(db):
    return np.exp(np.asarray(db, f64) * DB2LIN).astype(f32)


def ring_frames(mix_rate):
    """The engine's stereo-enhance ring: 1 << bitlength((int)((50 + 2) / 1000 sr)) mono frames."""
    return 1 << int((50.0 + 2.0) / 1000.0 * float(f32(mix_rate))).bit_length()


def delay_frames(ms, mix_rate):
    """(unsigned)((double)ms / 1000.0 * sr), ms f32 per source."""
    return (np.asarray(ms, f32).astype(f64) / 1000.0 * f64(f32(mix_rate))).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------- panner
def panner_constants(settings, j):
    pan = settings["panner_pan"][:, j].astype(f64)
    lvol = np.clip(1.0 - pan, 0.0, 1.0).astype(f32)
    rvol = np.clip(1.0 + pan, 0.0, 1.0).astype(f32)
    cl = (1.0 - lvol.astype(f64)).astype(f32)
    cr = (1.0 - rvol.astype(f64)).astype(f32)
    return lvol, rvol, cl, cr


class PannerStage:
    def __init__(self, j, n, mix_rate=48000.0):
        self.j = j

    def reset(self, s):
        pass

    def block(self, x, settings):
        x = np.asarray(x, f32)
        lvol, rvol, cl, cr = (k[:, None] for k in panner_constants(settings, self.j))
        L, R = x[..., 0], x[..., 1]
        y = np.empty_like(x)
        y[..., 0] = (L * lvol).astype(f32) + (R * cr).astype(f32)
        y[..., 1] = (R * rvol).astype(f32) + (L * cl).astype(f32)
        return y


# --------------------------------------------------------------------------------------------------- stereo enhance
class EnhanceStage:
    """State of one stereo enhance at chain position j for n sources: the mono ring and pos."""

    def __init__(self, j, n, mix_rate=48000.0):
        self.j, self.sr = j, mix_rate
        self.R = ring_frames(mix_rate)
        self.ring = np.zeros((n, self.R), f32)
        self.pos = np.zeros(n, np.int64)  # u32 in the kernel; only pos mod R matters (R divides 2^32)

    def reset(self, s):
        self.ring[s] = 0
        self.pos[s] = 0

    def block(self, x, settings):
        """Frame by frame, in the engine's order: write ring[pos], read ring[pos - delay], pos++."""
        x = np.asarray(x, f32)
        n, F, _ = x.shape
        j, mask = self.j, self.R - 1
        pull = settings["enhance_pan_pullout"][:, j].astype(f32)
        sur = settings["enhance_surround"][:, j].astype(f32)
        mode = sur > 0
        delay = delay_frames(settings["enhance_time_pullout_ms"][:, j], self.sr)
        rows = np.arange(n)
        y = np.empty_like(x)
        half = f32(0.5)
        for i in range(F):
            L, R = x[:, i, 0], x[:, i, 1]
            c = (L + R) * half
            l = c + (L - c) * pull
            r = c + (R - c) * pull
            self.ring[rows, self.pos & mask] = np.where(mode, (l + r) * half, r)
            d = self.ring[rows, (self.pos - delay) & mask]
            o = d * sur
            y[:, i, 0] = np.where(mode, l + o, l)
            y[:, i, 1] = np.where(mode, r - o, d)
            self.pos += 1
        return y


# ---------------------------------------------------------------------------------------------------------- limiter
def limiter_constants(settings, j):
    """ceiling, makeup, scv, scmult (f32, from f64) and ceil_db (f32) per source."""
    ceil_db = settings["limiter_ceiling_db"][:, j].astype(f64)
    thr_db = settings["limiter_threshold_db"][:, j].astype(f64)
    sc = -settings["limiter_soft_clip_db"][:, j].astype(f64)
    ceiling = np.exp(ceil_db * DB2LIN).astype(f32)
    makeup = np.exp((ceil_db - thr_db) * DB2LIN).astype(f32)
    scv = np.exp(sc * DB2LIN).astype(f32)
    scmult = np.abs((ceil_db - sc) / ((ceil_db + 25.0) - sc)).astype(f32)
    return ceiling, makeup, scv, scmult, settings["limiter_ceiling_db"][:, j].astype(f32)


class LimiterStage:
    def __init__(self, j, n, mix_rate=48000.0):
        self.j = j

    def reset(self, s):
        pass

    def block(self, x, settings):
        x = np.asarray(x, f32)
        ceiling, makeup, scv, scmult, ceil_db = (k[:, None, None] for k in limiter_constants(settings, self.j))
        one = f32(1)
        s = x * makeup
        a = np.abs(s)
        sign = np.where(s < 0, -one, one)
        soft = a > scv
        with np.errstate(divide="ignore"):
            over = (np.log(np.where(soft, a, one).astype(f64)) * LIN2DB).astype(f32) - ceil_db
        e = np.exp((over * scmult).astype(f32).astype(f64) * DB2LIN).astype(f32)
        s = np.where(soft, sign * (scv + e).astype(f32), s).astype(f32)
        return (np.minimum(ceiling, np.abs(s)) * np.where(s < 0, -one, one)).astype(f32)


def limiter_f64(x, settings, j):
    """The limiter with every constant and operation in f64: [n][F][2] -> [n][F][2] f64."""
    x = np.asarray(x, f64)
    ceil_db = settings["limiter_ceiling_db"][:, j].astype(f64)[:, None, None]
    thr_db = settings["limiter_threshold_db"][:, j].astype(f64)[:, None, None]
    sc = -settings["limiter_soft_clip_db"][:, j].astype(f64)[:, None, None]
    ceiling, makeup, scv = np.exp(ceil_db * DB2LIN), np.exp((ceil_db - thr_db) * DB2LIN), np.exp(sc * DB2LIN)
    scmult = np.abs((ceil_db - sc) / ((ceil_db + 25.0) - sc))
    y = np.empty_like(x)
    it = np.nditer(x, flags=["multi_index"])
    for v in it:
        k = it.multi_index[0]
        s = float(v) * makeup[k, 0, 0]
        a = abs(s)
        if a > scv[k, 0, 0]:
            s = (-1.0 if s < 0 else 1.0) * (scv[k, 0, 0] + np.exp((np.log(a) * LIN2DB - ceil_db[k, 0, 0]) * scmult[k, 0, 0] * DB2LIN))
        y[it.multi_index] = min(ceiling[k, 0, 0], abs(s)) * (-1.0 if s < 0 else 1.0)
    return y


def make_stage(kind, j, n, mix_rate=48000.0):
    return {PANNER: PannerStage, ENHANCE: EnhanceStage, LIMITER: LimiterStage}[kind](j, n, mix_rate)


_EDGES = {
    "panner_pan": (-1.0, 1.0, 0.0),
    "enhance_pan_pullout": (0.0, 4.0, 1.0),
    "enhance_time_pullout_ms": (0.0, 50.0),
    "enhance_surround": (0.0, 1.0),
    "limiter_ceiling_db": (-20.0, -0.1),
    "limiter_threshold_db": (-30.0, 0.0),
    "limiter_soft_clip_db": (0.0, 6.0),
    "limiter_soft_clip_ratio": (3.0, 20.0),
}


def draw_settings(rng, n, capi, edges=True):
    """Every field over its whole range at every position; with edges, about a fifth of the entries of every field sit
    on one of its range's ends (and the panner's centre, the enhance's unit pullout).  About half the stereo enhances
    are in the surround mode (surround > 0)."""
    s = capi.fx_stereo_settings_defaults(n)
    for name, e in _EDGES.items():
        sh = s[name].shape
        lo, hi = e[0], e[1]
        v = rng.uniform(lo, hi, sh)
        if name == "enhance_surround":
            v = np.where(rng.uniform(size=sh) < 0.5, 0.0, v)
        if edges:
            v = np.where(rng.uniform(size=sh) < 0.2, rng.choice(np.array(e), sh), v)
        s[name] = np.clip(v.astype(f32), f32(lo), f32(hi))  # (f32(-0.1) lies inside the f32 range check's f32(-0.1))
    return s
