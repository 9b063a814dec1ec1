"""GAS_FLAG_HRTF_INTERPOLATE: the composed reference and the bilinear rule.

The HRTF stage is linear in the HRIR, and the state it carries from block to block (gained mono history, previous gain,
the early-reflection ring in front of it) does not depend on the direction.  So the output of a source whose HRIR is the
blend sum_i w_i hrir[dir_i] is the weighted sum of what the existing oracle renders for that source with
hrtf_dir = dir_i.  No new reference arithmetic: up to four single-source oracle.binding.BatchOracle instances per source,
fed the same rows and parameters except hrtf_dir, combined in float64."""
import numpy as np


def one_row(dirs):
    """Explicit one-row blends {dir, 1, 0, 0, 0}: what the all-zero row stands for."""
    from godot_audio_spatializer_amd import capi

    b = np.zeros(len(dirs), capi.HRTF_BLEND_DTYPE)
    b["dir"][:, 0] = dirs
    b["weight"][:, 0] = 1.0
    return b


class BlendReference:
    """n sources of one KIND_EFFECT chain (one HRTF in it), advanced one callback at a time."""

    def __init__(self, ob, n, frames, chain, hrir, er_ring_frames=4096):
        self.ob, self.n, self.frames = ob, n, frames
        self.oracles = [[ob.BatchOracle(ob.KIND_EFFECT, 1, frames, chain=chain, hrir=hrir, er_ring_frames=er_ring_frames) for _ in range(4)] for _ in range(n)]

    def block(self, params, blends, src):
        """params: PARAMS_DTYPE [n]; blends: HRTF_BLEND_DTYPE [n] (an all-zero row = hrtf_dir at weight 1); src: float32
        [n][F][2].  Returns (rows64 [n][F][2], peaks [n][2], mix64 [F][2]).  Every one of a source's four oracles runs
        every block (entries of weight 0 with direction 0), so that their states stay in step."""
        ob = self.ob
        params = np.ascontiguousarray(params).astype(ob.PARAMS_DTYPE)
        rows = np.zeros((self.n, self.frames, 2), np.float64)
        for s in range(self.n):
            d = np.array(blends["dir"][s], np.uint32)
            w = np.array(blends["weight"][s], np.float64)
            if not w.any():
                d, w = np.array([params["hrtf_dir"][s], 0, 0, 0], np.uint32), np.array([1.0, 0.0, 0.0, 0.0])
            for i in range(4):
                p = params[s : s + 1].copy()
                p["hrtf_dir"] = d[i] if w[i] != 0.0 else 0
                _, _, y64 = self.oracles[s][i].block(p, src[s : s + 1], want64=True)
                if w[i] != 0.0:
                    rows[s] += w[i] * y64[0]
        return rows, np.abs(rows).max(axis=1), rows.sum(axis=0)


def bilinear_blend(az, el, n_az, n_el):
    """The rule include/gas_amd.h states for gas_calc_spatialization, float64: (dir [4], weight [4]) for one direction.
    u = az / 2pi * n_az wrapped mod n_az, v = (el + pi/2) / pi * (n_el - 1) clamped; corners (floor u, floor v),
    (floor u + 1 mod n_az, floor v) and the same two one row up; at n_el == 1 or on the top row the upper pair has
    weight 0."""
    two_pi = 6.2831853071795864769252867666
    u = (az / two_pi * n_az) % n_az
    a0 = int(np.floor(u))
    fu = u - a0
    if a0 >= n_az:
        a0, fu = 0, 0.0
    a1 = (a0 + 1) % n_az
    top = n_el - 1
    v = min(max((el + two_pi / 4) / (two_pi / 2) * top, 0.0), float(top))
    e0 = int(np.floor(v))
    fv = v - e0
    e1 = min(e0 + 1, top)
    d = np.array([e0 * n_az + a0, e0 * n_az + a1, e1 * n_az + a0, e1 * n_az + a1], np.uint32)
    w = np.array([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], np.float64)
    return d, w


def nearest_cell(az, el, n_az, n_el):
    """Today's hrtf_dir: the nearest grid cell (k_calc_spatialization.hip)."""
    two_pi = 6.2831853071795864769252867666
    ai = int(np.floor(az / two_pi * n_az + 0.5)) % n_az
    ei = int(np.floor((el + two_pi / 4) / (two_pi / 2) * (n_el - 1) + 0.5)) if n_el > 1 else 0
    return min(max(ei, 0), n_el - 1) * n_az + ai
