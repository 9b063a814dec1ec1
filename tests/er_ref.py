"""GAS_FX_EARLY_REFLECTIONS: the rule, written once in numpy, and the delay tables that pin it at its edges.

The effect has no counterpart in the engine; its meaning is what include/gas_amd.h says at er_delay:

    d_k  = min(er_delay[k], er_ring_frames - frames)        as unsigned; 0 is legal and adds the frame itself
    y[t] = x[t] + sum_k er_gain[k] * x[t - d_k]

over the playback's OWN history: the concatenation of the callbacks it took part in, zeros before its first one.  The
gains and delays are those of the callback that t falls in.  Everything here is float64 over that growing history --
no ring, no write position and no modulo, so it shares no structure with oracle/gas_oracle.c::fx_early_reflections or
with the kernels' tap loops."""
import numpy as np

ER_TAPS = 8
FRAMES_RINGS = [(128, 256), (256, 512), (384, 1024), (512, 1024), (512, 4096), (256, 8192)]


def callbacks(F, R):
    """2R/F + 3 (rounded up): the write position wraps twice and the longest tap reads real frames, not the zeros in
    front of the stream."""
    return -(-2 * R // F) + 3


def effective_delays(delays, F, R):
    """min(er_delay, R - F) as unsigned, as int64."""
    return np.minimum(np.asarray(delays).astype(np.uint32).astype(np.int64), R - F)


def edge_delays(F, R):
    """(inside, outside): the legal delays at lane / register boundaries (63, 64, 65), at the seam between this
    callback's row and the ring (F - 1, F, F + 1) and at the far end m = R - F of the range (m - 65 .. m - 63: the same
    boundaries seen from the other side; m - 1, m: the frame about to be overwritten), and the values outside 1 .. m.
    Entries outside 1 .. m are dropped from `inside` here (F + 1 at R = 2F), duplicates too."""
    m = R - F
    inside = sorted({d for d in (1, 2, 63, 64, 65, F - 1, F, F + 1, m - 65, m - 64, m - 63, m - 1, m) if 1 <= d <= m})
    outside = [0, m + 1, R, R + 1, 0xFFFFFFFF]
    return inside, outside


class ErSource:
    """One playback's closed form."""

    def __init__(self, F, R):
        self.F, self.R = F, R
        self.hist = np.zeros((0, 2), np.float64)

    def block(self, gains, delays, x):
        """One callback this playback takes part in: gains float [8], delays uint32 [8] (raw), x [F][2] -> y float64 [F][2]."""
        F = self.F
        x = np.asarray(x, np.float64)
        assert x.shape == (F, 2)
        t0 = len(self.hist)
        self.hist = np.concatenate([self.hist, x])
        y = x.copy()
        for g, d in zip(np.asarray(gains, np.float64), effective_delays(delays, F, self.R)):
            lo = t0 - int(d)  # history index of the frame the tap adds to y[0]
            first = max(lo, 0)
            if lo + F > first:
                y[first - lo :] += g * self.hist[first : lo + F]
        return y


class ErBank:
    """n playbacks, advanced one callback at a time; a playback left out of a callback keeps its history."""

    def __init__(self, n, F, R):
        self.n, self.F, self.R = n, F, R
        self.sources = [ErSource(F, R) for _ in range(n)]

    def reset(self, s):
        self.sources[s] = ErSource(self.F, self.R)

    def block(self, params, src, active=None):
        """params [m] (er_gain, er_delay fields), src [m][F][2], active: the m source numbers (default: all n).
        Returns rows float64 [m][F][2]."""
        active = range(self.n) if active is None else active
        return np.stack([self.sources[s].block(params["er_gain"][r], params["er_delay"][r], src[r]) for r, s in enumerate(active)])


class TapDrawer:
    """Delays and gains for n sources per draw, built so that the table is covered by construction and the coverage
    is then asserted over what was really handed out.

    Per source: one tap has gain 0 (its delay is a random table entry and does not count), at least one of the others
    is negative, the gain of tap k is +-0.7^(k+1).  Every fourth source (counted across draws, so that a one-source case
    gets one too) repeats another tap's delay on one tap.  The remaining taps take the table's entries in turn, the
    turn carrying on from source to source and from draw to draw; each source's taps are then shuffled."""

    def __init__(self, rng, F, R, table=None):
        self.rng, self.F, self.R = rng, F, R
        inside, outside = edge_delays(F, R)
        self.table = list(table) if table is not None else inside + outside
        self.order = list(rng.permutation(len(self.table)))
        self.cursor = 0
        self.count = 0
        self.draws = []  # per draw: the set of table entries on taps with a non-zero gain

    def _next(self):
        v = self.table[self.order[self.cursor % len(self.table)]]
        self.cursor += 1
        return v

    def draw(self, n):
        """-> (delays uint32 [n][8], gains float32 [n][8])"""
        rng = self.rng
        delays = np.zeros((n, ER_TAPS), np.uint32)
        gains = np.zeros((n, ER_TAPS), np.float32)
        seen = set()
        for s in range(n):
            slots = list(rng.permutation(ER_TAPS))
            zero, neg = slots[0], slots[1]
            repeat = slots[2] if self.count % 4 == 1 else None
            self.count += 1
            sign = np.where(rng.random(ER_TAPS) < 0.5, -1.0, 1.0)
            sign[neg] = -1.0
            gains[s] = sign * 0.7 ** np.arange(1, ER_TAPS + 1)
            gains[s, zero] = 0.0
            for k in slots[3:] + [neg]:
                delays[s, k] = self._next()
            if repeat is not None:
                delays[s, repeat] = delays[s, slots[3]]
            else:
                delays[s, slots[2]] = self._next()
            delays[s, zero] = self.table[int(rng.integers(len(self.table)))]
            seen.update(int(d) for d, g in zip(delays[s], gains[s]) if g != 0.0)
            assert (gains[s] == 0).sum() == 1 and (gains[s] < 0).any()
        self.draws.append(seen)
        return delays, gains

    def repeats(self):
        return sum(1 for c in range(self.count) if c % 4 == 1)

    def assert_covered(self, per_draw=True):
        """Every entry of the table was on a tap with a non-zero gain: in each draw, or (a case too small to hold the
        table in one draw) over the draws of the case."""
        want = set(int(d) for d in self.table)
        assert self.draws
        if per_draw:
            for i, seen in enumerate(self.draws):
                assert want <= seen, f"draw {i} misses {sorted(want - seen)}"
        else:
            seen = set().union(*self.draws)
            assert want <= seen, f"the case misses {sorted(want - seen)}"
