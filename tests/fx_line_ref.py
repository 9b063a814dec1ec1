"""Independent numpy restatement of GAS_FX_DELAY / GAS_FX_REVERB (the header of csrc/k_fx_line.hip):
[ENGINE] AudioEffectDelayInstance::process and AudioEffectReverbInstance / Reverb::process, from recollection of the
engine source -- parity unpinned, like SURVEY Appendix B.

Sequential in the engine's order: one frame at a time, vectorised over sources (and ears).  Block constants are computed
in f64 and rounded to f32; the per-frame products and sums are separate f32 operations, except the comb damping sum,
which the engine evaluates in f64 (`out * (1.0 - damp) + damp_h * damp`).  x is float32 [n][F][2]; settings is a
gas_fx_line_settings array [n]; j is the chain position whose settings apply.

Memory sizes: the delay ring and feedback buffer and the reverb's echo buffer only need to be longer than the longest
delay a test uses (the output does not depend on their length beyond that), so a stage can be built smaller than the
library's lines (`max_ms`, `echo_frames`) to keep 8192-source references in memory.
"""
import numpy as np

f32, f64 = np.float32, np.float64
DB2LIN = 0.11512925464970228
TWO_PI = 6.283185307179586
COMB_T = (0.025306122448979593, 0.026938775510204082, 0.028956916099773241, 0.03074829931972789, 0.032244897959183672, 0.03380952380952381, 0.035306122448979592, 0.036666666666666667)
ALLPASS_T = (0.0051020408163265302, 0.007732426303854875, 0.01, 0.012607709750566893)
SPREAD_BASE = (0.0, 0.000521)
DELAY, REVERB = 13, 14


def db2lin_block(db):
    return np.exp(np.asarray(db, f64) * DB2LIN).astype(f32)


def undenormalize(v):
    """[ENGINE] undenormalize: values whose biased exponent is below 16 (|v| < 2^-111) become 0."""
    v = np.asarray(v, f32)
    return np.where((v.view(np.uint32) & 0x7F800000) < 0x08000000, f32(0.0), v).astype(f32)


def _trunc(v):
    return np.trunc(np.asarray(v, f64)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- delay
def delay_constants(settings, j, mix_rate):
    sr = f64(f32(mix_rate))
    col = lambda name: settings[name][:, j]  # noqa: E731
    k = {"dry": col("delay_dry").astype(f32)}
    for t in (1, 2):
        lvl = np.where(col(f"delay_tap{t}_active") != 0, db2lin_block(col(f"delay_tap{t}_level_db")), f32(0.0)).astype(f32)
        pan = col(f"delay_tap{t}_pan").astype(f64)
        k[f"v{t}"] = np.stack([(lvl.astype(f64) * np.clip(1.0 - pan, 0.0, 1.0)).astype(f32), (lvl.astype(f64) * np.clip(1.0 + pan, 0.0, 1.0)).astype(f32)], axis=1)
        k[f"d{t}"] = _trunc(col(f"delay_tap{t}_ms").astype(f64) / 1000.0 * sr)
    k["fl"] = np.where(col("delay_feedback_active") != 0, db2lin_block(col("delay_feedback_level_db")), f32(0.0)).astype(f32)
    k["dfb"] = _trunc(col("delay_feedback_ms").astype(f64) / 1000.0 * sr)
    k["c"] = np.exp(-TWO_PI * col("delay_feedback_lowpass_hz").astype(f64) / sr).astype(f32)
    k["ic"] = (f32(1.0) - k["c"]).astype(f32)
    return k


class DelayStage:
    """State of one GAS_FX_DELAY at chain position j for n sources: ring (write position P), feedback buffer (q), h."""

    def __init__(self, j, n, mix_rate=48000.0, max_ms=1500.0):
        self.j, self.mix_rate = j, mix_rate
        sr = f64(f32(mix_rate))
        dmax = int(max_ms / 1000.0 * sr)
        ring = 1
        while ring < dmax + 1:
            ring *= 2
        self.mask = ring - 1
        self.ring = np.zeros((n, ring, 2), f32)
        self.fb = np.zeros((n, dmax + 1, 2), f32)
        self.P = np.zeros(n, np.int64)
        self.q = np.zeros(n, np.int64)
        self.h = np.zeros((n, 2), f32)

    def reset(self, s):
        self.ring[s] = 0
        self.fb[s] = 0
        self.P[s] = 0
        self.q[s] = 0
        self.h[s] = 0

    def block(self, x, settings):
        x = np.asarray(x, f32)
        n, F, _ = x.shape
        k = delay_constants(settings, self.j, self.mix_rate)
        assert k["d1"].max() <= self.mask and k["d2"].max() <= self.mask and k["dfb"].max() < self.fb.shape[1], "stage built too small"
        ix = np.arange(n)
        y = np.empty_like(x)
        dry = k["dry"][:, None]
        fl, c, ic = k["fl"][:, None], k["c"][:, None], k["ic"][:, None]
        for i in range(F):
            xi = x[:, i, :]
            self.ring[ix, self.P & self.mask] = xi
            r1 = self.ring[ix, (self.P - k["d1"]) & self.mask]
            r2 = self.ring[ix, (self.P - k["d2"]) & self.mask]
            out = ((xi * dry + r1 * k["v1"]) + r2 * k["v2"]).astype(f32)
            out = (out + self.fb[ix, self.q]).astype(f32)
            fbin = undenormalize((out * fl) * ic + self.h * c)
            self.h = fbin
            self.fb[ix, self.q] = fbin
            y[:, i, :] = out
            self.P += 1
            self.q += 1
            self.q = np.where(self.q >= k["dfb"], 0, self.q)
        return y


# ---------------------------------------------------------------------------------------------------------------- reverb
def reverb_geometry(mix_rate):
    """Per ear e: extra spread frames xs[e], comb and allpass sizes; the echo size."""
    sr = f64(f32(mix_rate))
    xs = [int(np.rint(b * sr)) for b in SPREAD_BASE]
    return {
        "xs": xs,
        "comb": [[int(np.rint(t * sr)) + xs[e] for t in COMB_T] for e in range(2)],
        "allpass": [[int(np.rint(t * sr)) + xs[e] for t in ALLPASS_T] for e in range(2)],
        "echo": int(0.5 * sr + 1.0),
    }


def reverb_constants(settings, j, mix_rate, geo):
    sr = f64(f32(mix_rate))
    col = lambda name: settings[name][:, j]  # noqa: E731
    k = {}
    k["pd"] = np.clip(np.rint(col("reverb_predelay_ms").astype(f64) / 1000.0 * sr).astype(np.int64), 10, geo["echo"] - 1)
    k["pfb"] = col("reverb_predelay_feedback").astype(f32)
    k["fbk"] = np.clip(0.7 + col("reverb_room_size").astype(f64) * 0.28, 0.7, 0.98).astype(f32)
    aux = (col("reverb_damping").astype(f64) / 2.0 + 0.5).astype(f32)
    aux = (aux * aux).astype(f32)
    k["damp"] = np.exp(-TWO_PI * aux.astype(f64) * 10000.0 / sr).astype(f32)
    hip = col("reverb_hipass").astype(f32)
    k["hp"] = hip > 0
    hpaux = np.exp(-TWO_PI * hip.astype(f64) * 6000.0 / sr).astype(f32)
    k["a1"] = ((1.0 + hpaux.astype(f64)) / 2.0).astype(f32)
    k["a2"] = (-k["a1"]).astype(f32)
    k["b1"] = hpaux
    k["wet"] = col("reverb_wet").astype(f32)
    k["dry"] = col("reverb_dry").astype(f32)
    spread = col("reverb_spread").astype(f64)
    # cut[n][ear] = lrintf(xs (1 - spread)): how much shorter than its size a comb / allpass runs
    k["cut"] = np.stack([np.rint((f64(f32(geo["xs"][e])) * (1.0 - spread)).astype(f32)).astype(np.int64) for e in range(2)], axis=1)
    return k


class ReverbStage:
    """State of one GAS_FX_REVERB at chain position j for n sources: two mono reverbs (ears) each."""

    def __init__(self, j, n, mix_rate=48000.0, echo_frames=None):
        self.j, self.mix_rate = j, mix_rate
        self.geo = reverb_geometry(mix_rate)
        g = self.geo
        self.echo_len = g["echo"] if echo_frames is None else echo_frames
        self.echo = np.zeros((n, 2, self.echo_len), f32)
        self.epos = np.zeros((n, 2), np.int64)
        self.h1 = np.zeros((n, 2), f32)
        self.h2 = np.zeros((n, 2), f32)
        self.comb = [np.zeros((n, 2, g["comb"][1][k]), f32) for k in range(8)]  # ear 0 uses the first comb[0][k]
        self.cpos = np.zeros((8, n, 2), np.int64)
        self.dh = np.zeros((8, n, 2), f32)
        self.ap = [np.zeros((n, 2, g["allpass"][1][k]), f32) for k in range(4)]
        self.apos = np.zeros((4, n, 2), np.int64)

    def reset(self, s):
        self.echo[s] = 0
        self.epos[s] = 0
        self.h1[s] = 0
        self.h2[s] = 0
        for b in self.comb + self.ap:
            b[s] = 0
        self.cpos[:, s] = 0
        self.dh[:, s] = 0
        self.apos[:, s] = 0

    def block(self, x, settings):
        x = np.asarray(x, f32)
        n, F, _ = x.shape
        g = self.geo
        k = reverb_constants(settings, self.j, self.mix_rate, g)
        assert self.echo_len == g["echo"] or k["pd"].max() < self.echo_len, "stage built too small"
        i0 = np.arange(n)[:, None]
        e1 = np.arange(2)[None, :]
        climit = [np.array(g["comb"])[:, c][None, :] - k["cut"] for c in range(8)]
        alimit = [np.array(g["allpass"])[:, a][None, :] - k["cut"] for a in range(4)]
        pd, pfb = k["pd"][:, None], k["pfb"][:, None]
        fbk, damp = k["fbk"][:, None], k["damp"][:, None]
        omd = 1.0 - damp.astype(f64)
        hp = np.broadcast_to(k["hp"][:, None], (n, 2))
        a1, a2, b1 = k["a1"][:, None], k["a2"][:, None], k["b1"][:, None]
        wet, dry = k["wet"][:, None], k["dry"][:, None]
        y = np.empty_like(x)
        for i in range(F):
            xi = x[:, i, :]
            # 1. predelay echo
            self.epos = np.where(self.epos >= self.echo_len, 0, self.epos)
            rd = self.epos - pd
            rd = np.where(rd < 0, rd + self.echo_len, rd)
            u = undenormalize(self.echo[i0, e1, rd] * pfb + xi)
            self.echo[i0, e1, self.epos] = u
            self.epos = self.epos + 1
            # 2. high-pass
            if hp.any():
                v = u
                hy = ((v * a1 + self.h1 * a2) + self.h2 * b1).astype(f32)
                self.h2 = np.where(hp, hy, self.h2).astype(f32)
                self.h1 = np.where(hp, v, self.h1).astype(f32)
                u = np.where(hp, hy, u).astype(f32)
            # 3. combs
            d = np.zeros((n, 2), f32)
            for c in range(8):
                p = np.where(self.cpos[c] >= climit[c], 0, self.cpos[c])
                buf = self.comb[c]
                o = undenormalize(buf[i0, e1, p] * fbk)
                o = (o.astype(f64) * omd + (self.dh[c] * damp).astype(f64)).astype(f32)
                self.dh[c] = o
                buf[i0, e1, p] = (u + o).astype(f32)
                d = (d + o).astype(f32)
                self.cpos[c] = p + 1
            # 4. allpasses
            for a in range(4):
                p = np.where(self.apos[a] >= alimit[a], 0, self.apos[a])
                buf = self.ap[a]
                aux = buf[i0, e1, p]
                nb = undenormalize(f32(0.7) * aux + d)
                buf[i0, e1, p] = nb
                d = (aux - f32(0.7) * nb).astype(f32)
                self.apos[a] = p + 1
            # 5. out
            y[:, i, :] = ((d * wet) * f32(0.6)) + xi * dry
        return y


def reverb_impulse_f64(x, fbk, damp, pd, pfb, wet, dry, comb, allpass, echo, a1=None, b1=None):
    """Independent float64 loop over ONE mono reverb of the same network (no f32 rounding, no undenormalize):
    x is a 1-D signal; comb / allpass are the lengths (no extra spread)."""
    buf_e = [0.0] * echo
    cb = [[0.0] * m for m in comb]
    cp = [0] * 8
    cdh = [0.0] * 8
    ab = [[0.0] * m for m in allpass]
    ap = [0] * 4
    ep = 0
    h1 = h2 = 0.0
    out = []
    for xv in x:
        xv = float(xv)
        r = ep - pd
        if r < 0:
            r += echo
        v = buf_e[r] * pfb + xv
        buf_e[ep] = v
        ep = (ep + 1) % echo
        if a1 is not None:
            yv = v * a1 - h1 * a1 + h2 * b1
            h2, h1, v = yv, v, yv
        d = 0.0
        for c in range(8):
            o = cb[c][cp[c]] * fbk
            o = o * (1.0 - damp) + cdh[c] * damp
            cdh[c] = o
            cb[c][cp[c]] = v + o
            cp[c] = (cp[c] + 1) % comb[c]
            d += o
        for a in range(4):
            aux = ab[a][ap[a]]
            ab[a][ap[a]] = 0.7 * aux + d
            d = aux - 0.7 * ab[a][ap[a]]
            ap[a] = (ap[a] + 1) % allpass[a]
        out.append(d * wet * 0.6 + xv * dry)
    return np.array(out)


# ---------------------------------------------------------------------------------------------------------------- both
def make_stage(kind, j, n, mix_rate=48000.0, max_ms=1500.0, echo_frames=None):
    return DelayStage(j, n, mix_rate, max_ms) if kind == DELAY else ReverbStage(j, n, mix_rate, echo_frames)


def draw_settings(rng, n, capi, max_ms=1500.0, max_predelay_ms=500.0, edges=True):
    """Legal settings across the property ranges at every chain position (delays up to max_ms, predelay up to
    max_predelay_ms), with the edges on some sources."""
    s = capi.fx_line_settings_defaults(n)
    shp = (n, capi.MAX_EFFECTS)
    s["delay_dry"] = rng.uniform(0.0, 1.0, shp)
    for t in (1, 2):
        s[f"delay_tap{t}_active"] = rng.integers(0, 4, shp) > 0
        s[f"delay_tap{t}_ms"] = rng.uniform(0.0, max_ms, shp)
        s[f"delay_tap{t}_level_db"] = rng.uniform(-60.0, 0.0, shp)
        s[f"delay_tap{t}_pan"] = rng.uniform(-1.0, 1.0, shp)
    s["delay_feedback_active"] = rng.integers(0, 3, shp) > 0
    s["delay_feedback_ms"] = rng.uniform(0.0, max_ms, shp)
    s["delay_feedback_level_db"] = rng.uniform(-60.0, 0.0, shp)
    s["delay_feedback_lowpass_hz"] = np.exp(rng.uniform(0.0, np.log(16000.0), shp))
    s["reverb_predelay_ms"] = rng.uniform(20.0, max_predelay_ms, shp)
    s["reverb_predelay_feedback"] = rng.uniform(0.0, 0.98, shp)
    for name in ("reverb_room_size", "reverb_damping", "reverb_spread", "reverb_dry", "reverb_wet"):
        s[name] = rng.uniform(0.0, 1.0, shp)
    s["reverb_hipass"] = np.where(rng.integers(0, 2, shp) > 0, rng.uniform(0.0, 1.0, shp), 0.0)
    if edges:
        i = np.arange(n)
        s["delay_tap1_ms"][i % 7 == 0] = 0.0
        s["delay_tap2_ms"][i % 7 == 1] = max_ms
        s["delay_feedback_ms"][i % 5 == 0] = 0.0
        s["delay_feedback_lowpass_hz"][i % 6 == 2] = 1.0
        s["reverb_room_size"][i % 4 == 0] = 1.0
        s["reverb_predelay_feedback"][i % 4 == 1] = 0.98
        s["reverb_predelay_ms"][i % 5 == 3] = 20.0
        s["reverb_spread"][i % 6 == 4] = 0.0
    return s
