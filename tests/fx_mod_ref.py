"""Independent numpy restatement of GAS_FX_CHORUS and GAS_FX_PHASER (the header of csrc/k_fx_mod.hip):
[ENGINE] AudioEffectChorusInstance::process and AudioEffectPhaserInstance::process, from recollection of the engine
source -- parity unpinned, like SURVEY Appendix B.

Block constants in f64, rounded to f32 where the engine's C++ does; every sine is (float)sin((double)arg); every f32
product and sum a separate operation.  The chorus splits a block into chunks of at most 256 frames, as the engine does.
x is float32 [n][F][2]; settings is a gas_fx_mod_settings array [n]; j is the chain position whose settings apply.
"""
import numpy as np

f32, f64 = np.float32, np.float64
DB2LIN = 0.11512925464970228
TAU = 6.283185307179586
CHORUS, PHASER = 19, 20
CHUNK = 256


def db2lin_block(db):
    return np.exp(np.asarray(db, f64) * DB2LIN).astype(f32)


def ring_frames(mix_rate):
    """The engine's chorus ring: 1 << bitlength((int)(0.24 sr)) frames."""
    return 1 << int(0.24 * float(f32(mix_rate))).bit_length()


def chorus_voice_constants(settings, j, v, L, mix_rate):
    """Per source: inc (int64), the cycle step after a chunk of L frames (int64), D, md, c1, c2, vol [n][2]."""
    sr = f64(f32(mix_rate))
    t = f32(L) / f32(mix_rate)
    cyc = f64(t) * settings["chorus_rate_hz"][:, j, v].astype(f64)
    inc = np.rint(cyc / L * 65536.0).astype(np.int64)
    step = np.rint((cyc * 65536.0).astype(f32)).astype(np.int64)
    D = np.rint((settings["chorus_delay_ms"][:, j, v].astype(f64) / 1000.0 * sr).astype(f32)).astype(np.int64)
    md = (settings["chorus_depth_ms"][:, j, v].astype(f64) / 1000.0 * sr).astype(f32)
    floor = md.astype(np.int64) + 10  # (unsigned)md + 10: md >= 0
    D = np.where(floor > D, floor, D)
    cut = settings["chorus_cutoff_hz"][:, j, v]
    c2 = np.where(cut >= 16000.0, f32(0), np.exp(-TAU * cut.astype(f64) / sr).astype(f32)).astype(f32)
    c1 = np.where(cut >= 16000.0, f32(1), f32(1) - c2).astype(f32)
    vol = settings["chorus_wet"][:, j].astype(f32) * db2lin_block(settings["chorus_level_db"][:, j, v])
    pan = settings["chorus_pan"][:, j, v].astype(f64)
    vl = (vol.astype(f64) * np.clip(1.0 - pan, 0.0, 1.0)).astype(f32)
    vr = (vol.astype(f64) * np.clip(1.0 + pan, 0.0, 1.0)).astype(f32)
    return inc, step, D, md, c1, c2, np.stack([vl, vr], axis=1)


class ChorusStage:
    """State of one chorus at chain position j for n sources: the stereo ring, pos, cycles[4] and h[4][2]."""

    def __init__(self, j, n, mix_rate=48000.0):
        self.j, self.sr = j, mix_rate
        self.R = ring_frames(mix_rate)
        self.ring = np.zeros((n, self.R, 2), f32)
        self.pos = np.zeros(n, np.int64)  # u32 in the kernel; only pos mod R matters (R divides 2^32)
        self.cycles = np.zeros((n, 4), np.uint64)
        self.h = np.zeros((n, 4, 2), f32)

    def reset(self, s):
        self.ring[s] = 0
        self.pos[s] = 0
        self.cycles[s] = 0
        self.h[s] = 0

    def block(self, x, settings):
        x = np.asarray(x, f32)
        n, F, _ = x.shape
        j, mask = self.j, self.R - 1
        vc = settings["chorus_voice_count"][:, j]
        dry = settings["chorus_dry"][:, j].astype(f32)
        rows = np.arange(n)[:, None]
        y = np.empty((n, F, 2), f32)
        for c0 in range(0, F, CHUNK):
            L = min(CHUNK, F - c0)
            i = np.arange(L)
            self.ring[rows, (self.pos[:, None] + i[None, :]) & mask] = x[:, c0 : c0 + L]
            out = x[:, c0 : c0 + L] * dry[:, None, None]
            for v in range(4):
                on = vc > v
                inc, step, D, md, c1, c2, vol = chorus_voice_constants(settings, j, v, L, self.sr)
                lc = (self.cycles[:, v, None] + (i[None, :] * inc[:, None]).astype(np.uint64)) & np.uint64(0xFFFF)
                ph = lc.astype(f32) / f32(65536.0)
                w = np.sin(ph.astype(f64) * TAU).astype(f32) * md[:, None]
                wf = np.floor(w).astype(np.int64)
                fr = (w - wf.astype(f32))[:, :, None]
                src = self.pos[:, None] + i[None, :] - D[:, None] - wf
                a = self.ring[rows, src & mask]
                b = self.ring[rows, (src - 1) & mask]
                q = ((a + (b - a) * fr) * vol[:, None, :]) * c1[:, None, None]
                h = self.h[:, v].copy()
                hs = np.empty_like(q)
                for k in range(L):
                    h = h * c2[:, None] + q[:, k]
                    hs[:, k] = h
                out = np.where(on[:, None, None], out + hs, out)
                self.h[:, v] = np.where(on[:, None], h, self.h[:, v])
                self.cycles[:, v] = np.where(on, self.cycles[:, v] + step.astype(np.uint64), self.cycles[:, v])
            y[:, c0 : c0 + L] = out
            self.pos = self.pos + L
        return y


def phaser_constants(settings, j, mix_rate):
    sr = f64(f32(mix_rate))
    dmin = (settings["phaser_range_min_hz"][:, j].astype(f64) / (sr / 2.0)).astype(f32)
    dmax = (settings["phaser_range_max_hz"][:, j].astype(f64) / (sr / 2.0)).astype(f32)
    inc = (TAU * (settings["phaser_rate_hz"][:, j].astype(f64) / sr).astype(f32).astype(f64)).astype(f32)
    return dmin, dmax, inc


class PhaserStage:
    """State of one phaser at chain position j for n sources: phase, h[2] and zm1[6][2]."""

    def __init__(self, j, n, mix_rate=48000.0):
        self.j, self.sr = j, mix_rate
        self.phase = np.zeros(n, f32)
        self.h = np.zeros((n, 2), f32)
        self.zm1 = np.zeros((n, 6, 2), f32)

    def reset(self, s):
        self.phase[s] = 0
        self.h[s] = 0
        self.zm1[s] = 0

    def lfo(self, F, settings):
        """a1 [n][F] of the next F frames (advances the phase)."""
        dmin, dmax, inc = phaser_constants(settings, self.j, self.sr)
        a1 = np.empty((len(inc), F), f32)
        phase = self.phase
        for k in range(F):
            phase = phase + inc
            while (phase.astype(f64) >= TAU).any():
                phase = np.where(phase.astype(f64) >= TAU, (phase.astype(f64) - TAU).astype(f32), phase)
            sn = np.sin(phase.astype(f64)).astype(f32)
            d = dmin + (dmax - dmin) * ((sn + f32(1)) / f32(2))
            a1[:, k] = (f32(1) - d) / (f32(1) + d)
        self.phase = phase
        return a1

    def block(self, x, settings):
        x = np.asarray(x, f32)
        n, F, _ = x.shape
        fb = settings["phaser_feedback"][:, self.j, None].astype(f32)
        depth = settings["phaser_depth"][:, self.j, None].astype(f32)
        a1 = self.lfo(F, settings)
        h, z = self.h, self.zm1
        y = np.empty((n, F, 2), f32)
        for k in range(F):
            a = a1[:, k, None]
            u = x[:, k] + h * fb
            for q in range(5, -1, -1):
                yy = u * (-a) + z[:, q]
                z[:, q] = yy * a + u
                u = yy
            h = u
            y[:, k] = x[:, k] + u * depth
        self.h = h
        return y


def phaser_f64(x, a1, fb, depth):
    """The phaser chain in f64 from rest, a1 per source and frame ([n][F], or [n][1] for a constant d: LTI):
    [n][F][2] -> [n][F][2]."""
    x = np.asarray(x, f64)
    a1 = np.broadcast_to(np.asarray(a1, f64), x.shape[:2])
    fb, depth = np.asarray(fb, f64).reshape(-1, 1), np.asarray(depth, f64).reshape(-1, 1)
    n, F, _ = x.shape
    h = np.zeros((n, 2))
    z = np.zeros((n, 6, 2))
    y = np.empty((n, F, 2))
    for k in range(F):
        u = x[:, k] + h * fb
        a = a1[:, k, None]
        for q in range(5, -1, -1):
            yy = -u * a + z[:, q]
            z[:, q] = yy * a + u
            u = yy
        h = u
        y[:, k] = x[:, k] + u * depth
    return y


def make_stage(kind, j, n, mix_rate=48000.0):
    return ChorusStage(j, n, mix_rate) if kind == CHORUS else PhaserStage(j, n, mix_rate)


def draw_settings(rng, n, capi):
    """Every field over its whole range at every position and voice (voice counts 1 .. 4)."""
    s = capi.fx_mod_settings_defaults(n)
    sh = s["chorus_delay_ms"].shape
    s["chorus_voice_count"] = rng.integers(1, 5, size=s["chorus_voice_count"].shape)
    s["chorus_dry"] = rng.uniform(0, 1, s["chorus_dry"].shape)
    s["chorus_wet"] = rng.uniform(0, 1, s["chorus_wet"].shape)
    s["chorus_delay_ms"] = rng.uniform(0, 50, sh)
    s["chorus_rate_hz"] = rng.uniform(0.1, 20, sh)
    s["chorus_depth_ms"] = rng.uniform(0, 20, sh)
    s["chorus_level_db"] = rng.uniform(-60, 24, sh)
    s["chorus_cutoff_hz"] = np.where(rng.uniform(size=sh) < 0.25, rng.uniform(16000, 20500, sh), np.exp(rng.uniform(0, np.log(16000), sh)))
    s["chorus_pan"] = rng.uniform(-1, 1, sh)
    s["phaser_range_min_hz"] = np.exp(rng.uniform(np.log(10), np.log(10000), s["phaser_range_min_hz"].shape))
    s["phaser_range_max_hz"] = np.exp(rng.uniform(np.log(10), np.log(10000), s["phaser_range_max_hz"].shape))
    s["phaser_rate_hz"] = rng.uniform(0.01, 20, s["phaser_rate_hz"].shape)
    s["phaser_feedback"] = rng.uniform(0.1, 0.9, s["phaser_feedback"].shape)
    s["phaser_depth"] = rng.uniform(0.1, 4, s["phaser_depth"].shape)
    return s
