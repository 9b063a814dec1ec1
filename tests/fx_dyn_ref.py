"""Independent numpy restatement of GAS_FX_DISTORTION / GAS_FX_COMPRESSOR (the header of
csrc/k_fx_dyn.hip): [ENGINE] AudioEffectDistortionInstance::process and AudioEffectCompressorInstance::process
(no sidechain), from recollection of the engine source -- parity unpinned, like SURVEY Appendix B.

Block constants are computed in f64 and rounded to f32; the per-sample products, sums and the recurrences are separate
f32 operations in the engine's order; per-sample transcendentals are evaluated in f64 and rounded.  x is float32
[n][F][2]; settings is a gas_fx_dyn_settings array [n]; j is the chain position whose settings apply.
"""
import numpy as np

f32, f64 = np.float32, np.float64
DB2LIN = 0.11512925464970228
LIN2DB = 8.685889638065035
CLIP, ATAN, LOFI, OVERDRIVE, WAVESHAPE = 0, 1, 2, 3, 4


def db2lin_block(db):
    return np.exp(np.asarray(db, f64) * DB2LIN).astype(f32)


def undenormalize(v):
    """[ENGINE] undenormalize: values whose biased exponent is below 16 (|v| < 2^-111) become 0."""
    v = np.asarray(v, f32)
    return np.where((v.view(np.uint32) & 0x7F800000) < 0x08000000, f32(0.0), v).astype(f32)


def distortion_constants(settings, j, mix_rate):
    d = settings["distortion_drive"][:, j].astype(f32)
    keep = settings["distortion_keep_hf_hz"][:, j].astype(f64)
    k = {}
    k["mode"] = settings["distortion_mode"][:, j].astype(np.int32)
    k["c"] = np.exp(-2.0 * np.pi * keep / f64(f32(mix_rate))).astype(f32)
    k["ic"] = (f32(1.0) - k["c"]).astype(f32)
    k["pre"] = db2lin_block(settings["distortion_pre_gain_db"][:, j])
    k["post"] = db2lin_block(settings["distortion_post_gain_db"][:, j])
    k["clip_e"] = (1.0001 - d.astype(f64)).astype(f32)
    k["atan_mult"] = (10.0 ** ((d * d).astype(f64) * 3.0) - 1.0 + 0.001).astype(f32)
    k["atan_div"] = (1.0 / (np.arctan(k["atan_mult"].astype(f64)).astype(f32).astype(f64) * (1.0 + (d * f32(8.0)).astype(f64)))).astype(f32)
    k["lofi_mult"] = (2.0 ** (2.0 + (1.0 - d.astype(f64)) * 14.0)).astype(f32)
    k["ws_k"] = ((f32(2.0) * d).astype(f64) / (1.00001 - d.astype(f64))).astype(f32)
    return k


def shape(mode, a, k, sel):
    """The waveshaper of one mode over a[sel] (f32), constants of those sources."""
    a = a[sel]
    col = lambda name: k[name][sel][:, None, None]  # noqa: E731
    if mode == CLIP:
        sign = np.where(a < 0, f32(-1.0), f32(1.0))
        r = (np.abs(a).astype(f64) ** col("clip_e").astype(f64)).astype(f32) * sign
        return np.clip(r, f32(-1.0), f32(1.0)).astype(f32)
    if mode == ATAN:
        return (np.arctan((a * col("atan_mult")).astype(f64)).astype(f32) * col("atan_div")).astype(f32)
    if mode == LOFI:
        m = col("lofi_mult")
        return (np.floor(a * m + f32(0.5)) / m).astype(f32)
    if mode == OVERDRIVE:
        x = a.astype(f64) * 0.686306
        z = 1.0 + np.exp(np.sqrt(np.abs(x)) * -0.75)
        return ((np.exp(x) - np.exp(-x * z)) / (np.exp(x) + np.exp(-x))).astype(f32)
    kk = col("ws_k").astype(f64)
    a64 = a.astype(f64)
    return ((1.0 + kk) * a64 / (1.0 + kk * np.abs(a64))).astype(f32)


def distortion(x, settings, j, h, mix_rate=48000.0):
    """One block; h (float32 [n][2]) is the per-ear state, updated in place.  Returns (y, the low band before shaping)."""
    x = np.asarray(x, f32)
    k = distortion_constants(settings, j, mix_rate)
    u = (x * k["ic"][:, None, None]).astype(f32)
    c = k["c"][:, None]
    lo = np.empty_like(x)
    hh = h.astype(f32)
    for i in range(x.shape[1]):
        hh = undenormalize(u[:, i, :] + c * hh)
        lo[:, i, :] = hh
    h[:] = hh
    a = (lo * k["pre"][:, None, None]).astype(f32)
    for m in (CLIP, ATAN, LOFI, OVERDRIVE, WAVESHAPE):
        sel = k["mode"] == m
        if sel.any():
            a[sel] = shape(m, a, k, sel)
    y = (a * k["post"][:, None, None] + (x - lo)).astype(f32)
    return y, lo


def compressor_constants(settings, j, mix_rate):
    sr = f64(f32(mix_rate))
    k = {}
    k["thr"] = db2lin_block(settings["compressor_threshold_db"][:, j])
    k["at"] = np.exp(-1.0 / (settings["compressor_attack_us"][:, j].astype(f64) * 1e-6 * sr)).astype(f32)
    k["rel"] = np.exp(-1.0 / (settings["compressor_release_ms"][:, j].astype(f64) * 1e-3 * sr)).astype(f32)
    k["mk"] = db2lin_block(settings["compressor_gain_db"][:, j])
    k["ratio"] = settings["compressor_ratio"][:, j].astype(f32)
    k["mix"] = settings["compressor_mix"][:, j].astype(f32)
    return k


def compressor(x, settings, j, rundb, mix_rate=48000.0):
    """One block; rundb (float32 [n]) is updated in place.  Returns (y, over [n][F], rundb per frame [n][F])."""
    x = np.asarray(x, f32)
    k = compressor_constants(settings, j, mix_rate)
    peak = np.maximum(np.abs(x[..., 0]), np.abs(x[..., 1]))
    q = (peak / k["thr"][:, None]).astype(f32)
    with np.errstate(divide="ignore"):
        lg = np.log(q.astype(f64)).astype(f32)
    over = (f32(2.08136898) * (lg * f32(LIN2DB))).astype(f32)
    over = np.where(over < 0, f32(0.0), over).astype(f32)
    rd = rundb.astype(f32)
    at, rel = k["at"], k["rel"]
    runs = np.empty_like(over)
    for i in range(x.shape[1]):
        o = over[:, i]
        rd = (o + np.where(o > rd, at, rel) * (rd - o)).astype(f32)
        runs[:, i] = rd
    rundb[:] = rd
    gr = ((-runs * (k["ratio"] - f32(1.0))[:, None]) / k["ratio"][:, None]).astype(f32)
    g = np.exp((gr * f32(DB2LIN)).astype(f64)).astype(f32)
    mk, mix = k["mk"][:, None, None], k["mix"][:, None, None]
    y = (((x * g[..., None]) * mk) * mix + x * (f32(1.0) - mix)).astype(f32)
    return y, over, runs


class DynStage:
    """State of one GAS_FX_DISTORTION / GAS_FX_COMPRESSOR at chain position j for n sources."""

    def __init__(self, kind, j, n, mix_rate=48000.0, distortion_kind=11):
        self.distortion = kind == distortion_kind
        self.j, self.mix_rate = j, mix_rate
        self.h = np.zeros((n, 2), f32)
        self.rundb = np.zeros(n, f32)

    def reset(self, s):
        self.h[s] = 0.0
        self.rundb[s] = 0.0

    def block(self, x, settings):
        if self.distortion:
            return distortion(x, settings, self.j, self.h, self.mix_rate)[0]
        return compressor(x, settings, self.j, self.rundb, self.mix_rate)[0]


def draw_settings(rng, n, capi, modes=None, edges=True, max_pre_db=60.0):
    """Settings across the engine's property ranges (distortion pre_gain -60..60 dB, keep_hf 1..20000 Hz, drive 0..1,
    post_gain -80..24 dB; compressor threshold -60..0 dB, ratio 1..48, gain -20..20 dB, attack 20..2000 us, release
    20..2000 ms, mix 0..1) at every chain position, with the edges on some sources."""
    s = capi.fx_dyn_settings_defaults(n)
    shp = (n, capi.MAX_EFFECTS)
    s["distortion_mode"] = rng.integers(0, 5, shp) if modes is None else rng.choice(modes, shp)
    s["distortion_pre_gain_db"] = rng.uniform(-60.0, max_pre_db, shp)
    s["distortion_keep_hf_hz"] = np.exp(rng.uniform(0.0, np.log(20000.0), shp))
    s["distortion_drive"] = rng.uniform(0.0, 1.0, shp)
    s["distortion_post_gain_db"] = rng.uniform(-80.0, 24.0, shp)
    s["compressor_threshold_db"] = rng.uniform(-60.0, 0.0, shp)
    s["compressor_ratio"] = rng.uniform(1.0, 48.0, shp)
    s["compressor_gain_db"] = rng.uniform(-20.0, 20.0, shp)
    s["compressor_attack_us"] = rng.uniform(20.0, 2000.0, shp)
    s["compressor_release_ms"] = rng.uniform(20.0, 2000.0, shp)
    s["compressor_mix"] = rng.uniform(0.0, 1.0, shp)
    if edges:
        i = np.arange(n)
        s["distortion_drive"][i % 7 == 0] = 0.0
        s["distortion_drive"][i % 7 == 1] = 1.0
        s["distortion_keep_hf_hz"][i % 5 == 0] = 1.0
        s["distortion_keep_hf_hz"][i % 5 == 1] = 20000.0
        s["compressor_ratio"][i % 4 == 0] = 48.0
        s["compressor_ratio"][i % 9 == 1] = 1.0
        s["compressor_attack_us"][i % 3 == 0] = 20.0
        s["compressor_release_ms"][i % 6 == 1] = 20.0
        s["compressor_mix"][i % 8 == 2] = 0.0
        s["compressor_mix"][i % 8 == 3] = 1.0
    return s
