"""GAS_FLAG_HRTF_BLEND_FADE: the composed reference.

No new arithmetic.  The HRTF stage is linear in the HRIR and its carried state does not depend on the direction (the
premise of hrtf_blend_ref.py, checked in test_hrtf_blend_reference.py), so both sides of the fade are weighted sums of
the existing oracle's single-direction renders:  y = t * Y_new + (1 - t) * Y_old,  Y = sum_k w_k * render(dir_k),
t = (float)i * (1 / F) in float32 as include/gas_amd.h states it, the sums and the lerp in float64.  Per source one
non-cross-fade oracle per distinct direction in play this block (at most eight), the idle ones run on direction 0 so
that all eight stay in step.  The old effective row is tracked here, not taken from the code under test."""
import numpy as np


def effective_row(blend, hrtf_dir, dirs):
    """What the HRTF stage makes of a slot's gas_hrtf_blend row: non-zero weights to the front in index order, directions
    clamped as hrtf_dir is, the rest zero; the all-zero row becomes {hrtf_dir, 1}.  Returns (dir uint32[4], weight
    float32[4])."""
    d, w = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    k = 0
    for i in range(4):
        if np.float32(blend["weight"][i]) != 0.0:
            d[k] = blend["dir"][i] if blend["dir"][i] < dirs else 0
            w[k] = blend["weight"][i]
            k += 1
    if k == 0:
        d[0], w[0] = (hrtf_dir if hrtf_dir < dirs else 0), 1.0
    return d, w


def same_row(a, b):
    """Bitwise equality of the eight words."""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def ramp(frames):
    """(t, 1 - t) as the kernels compute them: float32, t = (float)i * (1 / F)."""
    t = np.arange(frames, dtype=np.float32) * (np.float32(1.0) / np.float32(frames))
    return t, np.float32(1.0) - t


class BlendFadeReference:
    """n sources of one KIND_EFFECT chain (one HRTF in it), advanced one callback at a time."""

    def __init__(self, ob, n, frames, chain, hrir, er_ring_frames=4096, fade=True):
        self.ob, self.n, self.frames, self.dirs, self.fade = ob, n, frames, hrir.shape[0], fade
        self.oracles = [[ob.BatchOracle(ob.KIND_EFFECT, 1, frames, chain=chain, hrir=hrir, er_ring_frames=er_ring_frames) for _ in range(8)] for _ in range(n)]
        self.chain, self.hrir, self.ring = chain, hrir, er_ring_frames
        self.old = [None] * n

    def reset(self, s):
        """gas_source_reset / free + re-alloc of source s: fresh DSP state, no old row."""
        self.oracles[s] = [self.ob.BatchOracle(self.ob.KIND_EFFECT, 1, self.frames, chain=self.chain, hrir=self.hrir, er_ring_frames=self.ring) for _ in range(8)]
        self.old[s] = None

    def block(self, params, blends, src, active=None):
        """params: PARAMS_DTYPE [m]; blends: HRTF_BLEND_DTYPE [m]; src: float32 [m][F][2]; active: the m source numbers
        this callback processes (all n by default) -- a source left out keeps its state and its old row.  Returns
        (rows64 [m][F][2], peaks [m][2], mix64 [F][2])."""
        ob = self.ob
        active = list(range(self.n)) if active is None else list(active)
        params = np.ascontiguousarray(params).astype(ob.PARAMS_DTYPE)
        t, one_t = (x.astype(np.float64)[:, None] for x in ramp(self.frames))
        rows = np.zeros((len(active), self.frames, 2), np.float64)
        for r, s in enumerate(active):
            new = effective_row(blends[r], int(params["hrtf_dir"][r]), self.dirs)
            old = self.old[s]
            changed = self.fade and old is not None and not same_row(old, new)
            in_play = [int(d) for d, w in zip(*new) if w != 0.0]
            if changed:
                in_play += [int(d) for d, w in zip(*old) if w != 0.0]
            distinct = sorted(set(in_play))
            assert len(distinct) <= 8
            render = {}
            for i in range(8):
                p = params[r : r + 1].copy()
                p["hrtf_dir"] = distinct[i] if i < len(distinct) else 0
                _, _, y64 = self.oracles[s][i].block(p, src[r : r + 1], want64=True)
                if i < len(distinct):
                    render[distinct[i]] = y64[0]
            y_new = sum(float(w) * render[int(d)] for d, w in zip(*new) if w != 0.0)
            if changed:
                y_old = sum(float(w) * render[int(d)] for d, w in zip(*old) if w != 0.0)
                rows[r] = t * y_new + one_t * y_old
            else:
                rows[r] = y_new
            self.old[s] = new
        return rows, np.abs(rows).max(axis=1), rows.sum(axis=0)
