"""Numpy restatement of GAS_FX_COMPRESSOR with a sidechain (the header of csrc/k_fx_dyn.hip):
[ENGINE] AudioEffectCompressorInstance::process reading its detector frame from the sidechain bus when one is named,
from recollection of the engine source -- parity unpinned, like SURVEY Appendix B.

With s = compressor_sidechain[j] of a source, the detector frame is d[i] = x[i] when s == 0 and keys[s - 1][i]
otherwise; over, the rundb recurrence and the gain are fx_dyn_ref.compressor's, operation for operation, and the gain
always lands on the source's own x.  Constants and rounding conventions are fx_dyn_ref's, by import.  x is float32
[n][F][2], keys float32 [MAX_SIDECHAINS][F][2], settings a gas_fx_dyn_settings array [n], j the chain position.
"""
import numpy as np

import fx_dyn_ref as ref
from fx_dyn_ref import DB2LIN, LIN2DB, f32, f64

MAX_SIDECHAINS = 8


def detector_frames(x, keys, sidechain):
    """d [n][F][2]: the source's own frames, or those of key sidechain - 1."""
    x = np.asarray(x, f32)
    keys = np.asarray(keys, f32)
    s = np.asarray(sidechain).astype(np.int64)
    assert keys.shape == (MAX_SIDECHAINS,) + x.shape[1:] and s.shape == (x.shape[0],) and s.min() >= 0 and s.max() <= MAX_SIDECHAINS
    d = x.copy()
    keyed = s != 0
    d[keyed] = keys[s[keyed] - 1]
    return d


def compressor(x, keys, settings, j, rundb, mix_rate=48000.0):
    """One block; rundb (float32 [n]) is updated in place.  Returns (y, over [n][F], rundb per frame [n][F])."""
    x = np.asarray(x, f32)
    k = ref.compressor_constants(settings, j, mix_rate)
    d = detector_frames(x, keys, settings["compressor_sidechain"][:, j])
    peak = np.maximum(np.abs(d[..., 0]), np.abs(d[..., 1]))
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


class KeyedStage:
    """State of one GAS_FX_COMPRESSOR at chain position j for n sources: the one rundb, whatever the sidechain is."""

    def __init__(self, j, n, mix_rate=48000.0):
        self.j, self.mix_rate = j, mix_rate
        self.rundb = np.zeros(n, f32)

    def reset(self, s):
        self.rundb[s] = 0.0

    def block(self, x, keys, settings):
        return compressor(x, keys, settings, self.j, self.rundb, self.mix_rate)[0]


def draw_sidechains(rng, n, positions=4):
    """A random sidechain 0 .. MAX_SIDECHAINS per source and chain position."""
    return rng.integers(0, MAX_SIDECHAINS + 1, (n, positions)).astype(np.uint32)
