"""GAS_FLAG_ER_TAP_FADE: the composed reference.

No new arithmetic.  The early-reflection rule (er_ref.py) is linear in the taps, and a playback's history -- its own
input -- does not depend on them.  So per playback two er_ref.ErSource run in lockstep on the same x: one renders the
block with the old effective taps, the other with the new ones, and

    y = t * Y_new + (1 - t) * Y_old,   t = (float)f * (1 / F) in float32 as include/gas_amd.h states it,

the sums and the lerp in float64.  A block whose effective row (eight gains as bits, eight delays after min(d, R - F))
equals the old one bitwise, or that has no old row, is Y_new alone.  The old row is tracked here, never taken from the
code under test."""
import numpy as np

import er_ref


def effective_row(gains, delays, F, R):
    """(gain float32[8], delay uint32[8] after the clamp): the 16 words the stage compares."""
    return np.asarray(gains, np.float32).copy(), er_ref.effective_delays(delays, F, R).astype(np.uint32)


def same_row(a, b):
    """Bitwise equality of the 16 words (0.0 and -0.0 differ)."""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def ramp(frames):
    """(t, 1 - t) as the kernel computes them: float32, t = (float)f * (1 / F)."""
    t = np.arange(frames, dtype=np.float32) * (np.float32(1.0) / np.float32(frames))
    return t, np.float32(1.0) - t


class ErFadeSource:
    """One playback: two closed forms fed the same input, and the row it last rendered with."""

    def __init__(self, F, R, fade=True):
        self.F, self.R, self.fade = F, R, fade
        self.a, self.b = er_ref.ErSource(F, R), er_ref.ErSource(F, R)
        self.old = None
        self.faded = 0  # blocks that took the fade

    def block(self, gains, delays, x):
        new = effective_row(gains, delays, self.F, self.R)
        changed = self.fade and self.old is not None and not same_row(self.old, new)
        y_new = self.a.block(new[0], new[1], x)
        old = self.old if changed else new
        y_old = self.b.block(old[0], old[1], x)  # always advanced: the two histories stay in step
        self.old = new
        if not changed:
            return y_new
        self.faded += 1
        t, one_t = (v.astype(np.float64)[:, None] for v in ramp(self.F))
        return t * y_new + one_t * y_old


class ErFadeBank:
    """n playbacks, advanced one callback at a time; a playback left out of a callback keeps history and old row."""

    def __init__(self, n, F, R, fade=True):
        self.n, self.F, self.R, self.fade = n, F, R, fade
        self.sources = [ErFadeSource(F, R, fade) for _ in range(n)]

    def reset(self, s):
        """gas_source_reset / free + re-alloc of source s: empty history, no old row."""
        self.sources[s] = ErFadeSource(self.F, self.R, self.fade)

    def block(self, params, src, active=None):
        """params [m] (er_gain, er_delay fields, raw), src [m][F][2], active: the m source numbers (default: all n).
        Returns rows float64 [m][F][2]."""
        active = range(self.n) if active is None else active
        return np.stack([self.sources[s].block(params["er_gain"][r], params["er_delay"][r], src[r]) for r, s in enumerate(active)])

    def faded(self):
        return [s.faded for s in self.sources]
