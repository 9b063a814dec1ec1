"""The parameter generator (gas_calc_spatialization[_areas]) once, in float64 numpy.

Written from the reference's formulas -- audio_spatializer_3d.cpp:57-151 (SPCAP, stereo pan law, attenuation models),
:154-197 (calc_reverb_vol), :277-489 (listener loop, max distance, cone, Doppler, latch) -- and from the grid rule in
include/gas_amd.h (hrtf_dir = elevation_index * n_az + azimuth_index, azimuth_index = round(az / 2pi * n_az) mod n_az,
elevation_index = round((el + pi/2) / pi * (n_el - 1)), azimuth from -Z towards +X, towards the loudest listener,
hrtf_gain that listener's multiplier; no listener in range: gain 0 and the direction of (0, 0, -1)).  It shares no code
with oracle/gas_oracle.c or the kernel and is vectorised over the sources, not a row-by-row restatement.

Inputs are the structured arrays the GPU call takes, widened to float64 exactly; there is no float32 intermediate.  The
speaker directions are the reference's float32 constants (Vector3(...).normalized() in real_t), widened.  MAX(a, b) is
the engine's `a > b ? a : b`, so a NaN on the right wins and one on the left loses, as in the reference.  round() is
C's (halves away from zero).

`margins` says, per source, how far each decision was from flipping (see MARGINS_DTYPE).  The tests use it to keep
random rows away from knife edges, where float32 and float64 may branch differently, and to prove that a differing
hrtf_dir sits on a rounding border.  Knife edges themselves are tested with hand-placed values exact in float32.

Measured on the CPU (tests/test_calc_spat_reference.py prints the figures under pytest -s and fails when they leave
MEASURED below): the float32 oracle's worst deviation from this module, |got - want| / (atol + |want|) with the
project's atol (1e-7 for volumes, 1e-8 for linear_attenuation and hrtf_gain), over the far, near and quirk scenes of
tests/calc_spat_scenes.py with n in {1, 255, 256, 257, 1000}, listeners in {1, 3, 16}, 64 configs and two ticks, no row
left out, rows placed with the guards below:

    field               oracle vs float64   recorded   GPU bound = 4 x recorded   the project's rtol (cap)
    mix_volumes         3.45e-06            3.5e-06    1.4e-05                    3e-5
    reverb volumes      3.46e-06            3.5e-06    1.4e-05                    5e-5
    pitch_scale         2.74e-07            2.8e-07    1.12e-06                   3e-5
    linear_attenuation  8.41e-07            8.5e-07    3.4e-06                    3e-5
    hrtf_gain           1.63e-06            1.7e-06    6.8e-06                    3e-5

Integer fields, the cutoff and the latch are compared for equality; hrtf_dir may differ only where az_border or
el_border is below GRID_BORDER (on the fixed seeds the oracle differs from this module on no row at all).  Guards: a
random row closer than this to a cancellation or a branch border is redrawn (badly_placed):

    GUARD_SPCAP_AMP  64    spcap_amp.  The reference passes SPCAP an un-normalised direction (:391), so 1 + dot cancels
                           when the source is far: float32 leaves the position, and so each dot, wrong by a few 1e-8 of
                           (1 + |position|), and volume k = |g_k| / sqrt(sum g_j^2), g_j ~ (1 + dot_j)^tightness, carries
                           tightness * (1 + |position|) * (1 / |1 + dot_k| + sum_j share_j / |1 + dot_j|) times that.  Only
                           the volumes that survive the max-combine over the listeners count.  With the absolute guard
                           min |1 + dot| >= 0.1 alone the oracle deviated by 1.7e-5 (4 x that is above the cap), and no
                           absolute guard can hold for a source 360 away from sixteen listeners, hence the relative form.
    GUARD_SPCAP_SIGN 1e-4  spcap_rel, every listener in range: float32 gets the sign of 1 + dot right (the NaN pattern)
    GUARD_SPCAP      0.1   spcap; the near scene asserts it on every row (1 + dot >= 0.1 by construction)
    GUARD_PAN        0.02  pan: at full panning strength a source on the listener's x axis leaves
                           sqrt((1 - f cos x) / 2) (:109) the root of a difference of float32 roundings
    GUARD_TAPER      0.05  taper: 1 - dist / max_distance (:372) is the same kind of difference
    GUARD_BRANCH     1e-4  |dist|, |att|, |rev_att| and mult_gap (an exact tie excepted: one value, first listener wins)
    GUARD_CONE_DEG   1e-3  |cone|, degrees
"""
import numpy as np

GUARD_SPCAP = 0.1
GUARD_SPCAP_AMP = 64.0
GUARD_SPCAP_SIGN = 1e-4
GUARD_PAN = 0.02
GUARD_TAPER = 0.05
GUARD_BRANCH = 1e-4
GUARD_CONE_DEG = 1e-3
GRID_BORDER = 1e-4  # a hrtf_dir that differs is accepted only this close (grid units) to a rounding border

# the oracle's worst deviation from this module as measured (docstring), rounded up to two digits
MEASURED = {"mix_volumes": 3.5e-6, "reverb": 3.5e-6, "pitch_scale": 2.8e-7, "linear_attenuation": 8.5e-7, "hrtf_gain": 1.7e-6}
RTOL_CAP = {"mix_volumes": 3e-5, "reverb": 5e-5, "pitch_scale": 3e-5, "linear_attenuation": 3e-5, "hrtf_gain": 3e-5}  # what the project grants this kernel
GPU_RTOL = {f: 4.0 * v for f, v in MEASURED.items()}
assert all(GPU_RTOL[f] <= RTOL_CAP[f] for f in GPU_RTOL)  # above the cap the guards are to be raised, never the bound
ATOL = {"mix_volumes": 1e-7, "reverb": 1e-7, "pitch_scale": 0.0, "linear_attenuation": 1e-8, "hrtf_gain": 1e-8}

CMP_EPSILON = 0.00001
_INF = np.inf

MARGINS_DTYPE = np.dtype(
    [
        ("spcap", np.float64),  # min |1 + dot| over speakers and listeners in range; inf: stereo or nobody in range
        ("spcap_rel", np.float64),  # min |1 + dot| / (1 + |position|), likewise: how surely float32 gets that sum's sign
        ("spcap_amp", np.float64),  # how much SPCAP amplifies a relative rounding error of the position, largest over the
        # volumes that survive the max-combine (see output_vol); 0: stereo
        ("pan", np.float64),  # min 1 - |f cos x| over listeners in range (stereo), inf otherwise
        ("taper", np.float64),  # min 1 - dist / max_distance over listeners in range, inf without max_distance
        ("dist", np.float64),  # dist - total_max, the listener where it is smallest in magnitude; inf without max_distance
        ("cone", np.float64),  # angle - emission_angle (degrees), likewise; inf with the cone off
        ("att", np.float64),  # att + volume_db - max_db before the clamp, likewise (direct path and area distance)
        ("rev_att", np.float64),  # attenuation - 1 in calc_reverb_vol, likewise; inf where it is not evaluated
        ("az_border", np.float64),  # distance of az / 2pi * n_az from k + 1/2, grid units (0 .. 0.5); inf without a grid
        ("el_border", np.float64),  # the same for (el + pi/2) / pi * (n_el - 1); inf for n_el <= 1
        ("mult_gap", np.float64),  # (largest - second largest multiplier) / largest over listeners in range; inf below two
    ]
)

_S32 = np.array([(-1, 0, -1), (1, 0, -1), (0, 0, -1), (-1, 0, 1), (1, 0, 1), (-1, 0, 0), (1, 0, 0)], np.float32)
SPEAKERS = (_S32 / np.sqrt((_S32 * _S32).sum(axis=1, dtype=np.float32))[:, None]).astype(np.float64)  # real_t normalized()
SPEAKER_COUNT = np.array([2, 3, 5, 7])


def _max(a, b):
    return np.where(a > b, a, b)


def _closer(old, new, on):
    """Keep, per source, the signed margin of smallest magnitude."""
    return np.where(on & (np.abs(new) < np.abs(old)), new, old)


def _norm(v):
    l2 = (v * v).sum(axis=-1, keepdims=True)
    return np.where(l2 == 0, 0.0, v / np.sqrt(np.where(l2 == 0, 1.0, l2)))


def _round(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def db_to_linear(db):
    return np.exp(db * 0.11512925464970228420089957273422)


def attenuation_db(c, s, dist):
    """:123-151; returns (att, att + volume_db - max_db before the clamp)."""
    q = dist / c["unit_size"]
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        by_model = [20.0 * np.log10(1.0 / (q + CMP_EPSILON)), 20.0 * np.log10(1.0 / (q * q + CMP_EPSILON)), -20.0 * np.log(q + CMP_EPSILON)]
    att = np.select([c["attenuation_model"] == m for m in range(3)], by_model, 0.0) + s["volume_db"]
    return np.where(att > s["max_db"], s["max_db"], att), att - s["max_db"]


def output_vol(c, d):
    """calc_output_vol :112-121 for directions d [n][3]: (volumes [n][4][2], min |1 + dot| [n], min |1 + dot| / (1 + |d|) [n],
    1 - |f cos x| [n], error amplification per volume [n][4][2])."""
    n = len(d)
    out = np.zeros((n, 4, 2))
    stereo = c["speaker_mode"] == 0
    # stereo pan law :103-110
    pan = c["global_panning_strength"] * c["panning_strength"]
    flat = np.sqrt(d[:, 0] ** 2 + d[:, 2] ** 2)
    g = np.clip((1.0 - pan) ** 2, 0.0, 1.0)
    f = (1.0 - g) / (1.0 + g)
    fcos = np.clip(d[:, 0] / np.where(flat == 0.0, 1.0, flat), -1.0, 1.0) * f
    # SPCAP :57-98, :903-938
    tight = c["global_panning_strength"] * 2.0 * c["panning_strength"]
    count = SPEAKER_COUNT[c["speaker_mode"]]
    live = np.arange(7)[None, :] < count[:, None]  # [n][7]
    pair = 0.5 * (1.0 + SPEAKERS @ SPEAKERS.T)  # [7][7]
    eff = (pair[None, :, :] * live[:, None, :]).sum(axis=2)  # effective_number_of_speakers for this count
    base = 1.0 + d @ SPEAKERS.T
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gain = 0.5 * np.power(base, tight[:, None]) / eff
        sq = np.where(live, gain * gain, 0.0)
        vol = np.sqrt(sq / sq.sum(axis=1, keepdims=True))
    vol = np.where(live, vol, 0.0)
    out[:, 0, 0] = np.where(stereo, np.sqrt((1.0 - fcos) / 2.0), vol[:, 0])
    out[:, 0, 1] = np.where(stereo, np.sqrt((1.0 + fcos) / 2.0), vol[:, 1])
    out[:, 1, 0] = np.where(stereo, 0.0, vol[:, 2])
    out[:, 1, 1] = np.where(stereo, 0.0, 1.0)  # LFE: always full power
    out[:, 2, 0], out[:, 2, 1] = vol[:, 3], vol[:, 4]
    out[:, 3, 0], out[:, 3, 1] = vol[:, 5], vol[:, 6]
    spcap = np.where(stereo, _INF, np.where(live, np.abs(base), _INF).min(axis=1))
    reach = 1.0 + np.sqrt((d * d).sum(axis=1))  # an error of one part in the position moves a dot by up to this
    rel = np.where(stereo, _INF, spcap / reach)
    # first-order error amplification of volume k = |g_k| / sqrt(sum g_j^2), g_j ~ base_j^t: t * reach / |base_k| of its
    # own base and the same of the others', weighted by their share of the sum
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        per = np.where(live, tight[:, None] * reach[:, None] / np.abs(base), 0.0)
        shared = (np.where(live, sq / sq.sum(axis=1, keepdims=True), 0.0) * per).sum(axis=1)
        per = np.nan_to_num(per + shared[:, None], nan=0.0, posinf=_INF)  # a NaN row is compared by pattern only
    amp = np.zeros((n, 4, 2))
    for k, (a, b) in enumerate([(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (3, 0), (3, 1)]):
        amp[:, a, b] = np.where(stereo, 0.0, per[:, k])
    return out, spcap, rel, np.where(stereo, 1.0 - np.abs(fcos), _INF), amp


def reverb_vol(c, s, uniformity, amount, lap, direct, direct_amp):
    """calc_reverb_vol :154-197 for every source: (volumes [n][4][2], attenuation - 1 and att + volume_db - max_db where
    evaluated, else inf, error amplification per volume)."""
    dist = np.sqrt((lap * lap).sum(axis=1))
    att_db, att_margin = attenuation_db(c, s, dist)
    att = db_to_linear(att_db)
    chan = c["speaker_mode"] + 1
    center = np.array([0.5, 0.25, 0.16666, 0.125], np.float32).astype(np.float64)[chan - 1][:, None, None]
    flatpos = lap.copy()
    flatpos[:, 1] = 0.0
    panned, _, _, _, panned_amp = output_vol(c, _norm(flatpos))
    a = att[:, None, None]
    uni = np.where(a < 1.0, panned + (center - panned) * a, center)
    u = uniformity[:, None, None]
    blended = direct + (uni * a - direct) * u
    live = (np.arange(4)[None, :] < chan[:, None])[:, :, None]
    with_u = np.where(live, blended, 0.0) * amount[:, None, None]
    out = np.where(u > 0.0, with_u, direct * amount[:, None, None])
    amp = np.where((u > 0.0) & (a < 1.0), np.maximum(direct_amp, panned_amp), direct_amp)
    return out, np.where(uniformity > 0.0, att - 1.0, _INF), np.where(uniformity > 0.0, att_margin, _INF), amp


def calc(cfgs, cfg_index, poses, listeners, was_further, areas=None, listener_area_pos=None):
    """One physics tick.  was_further: [n] truth values from the previous tick.  Returns a dict: the generated
    gas_params fields (float64 / int64 arrays named as in PARAMS_DTYPE), `hrtf_written` (config has a grid), `reverb`
    [n][4][2], `in_range`, `was_further` (the next latch) and `margins` (MARGINS_DTYPE)."""
    n, nl = len(poses), len(listeners)
    ci = np.zeros(n, np.int64) if cfg_index is None else np.asarray(cfg_index, np.int64)
    c = {k: np.asarray(cfgs[k])[ci].astype(np.float64 if np.asarray(cfgs[k]).dtype.kind == "f" else np.int64) for k in cfgs.dtype.names}
    s = {k: np.asarray(poses[k], np.float64) for k in poses.dtype.names}
    if areas is None:
        present = np.zeros(n, bool)
        uniformity = amount = np.zeros(n)
        using = present
    else:
        present = np.asarray(areas["present"]) != 0
        using = np.asarray(areas["using_reverb_bus"]) != 0
        uniformity = np.asarray(areas["reverb_uniformity"], np.float64)
        amount = np.asarray(areas["reverb_amount"], np.float64)
    area_reverb = present & using
    area_uniform = area_reverb & (uniformity > 0) & (listener_area_pos is not None)
    lap_all = np.zeros((n, nl, 3)) if listener_area_pos is None else np.asarray(listener_area_pos, np.float64)

    pos = s["position"]
    doppler = c["doppler_tracking"] != 0
    src_vel = np.where(doppler[:, None], s["velocity"], 0.0)
    has_max = c["max_distance"] > 0
    out_vol = np.zeros((n, 4, 2))
    rev = np.zeros((n, 4, 2))
    out_amp = np.zeros((n, 4, 2))
    rev_amp = np.zeros((n, 4, 2))
    in_range = np.zeros(n, bool)
    lin_att = np.zeros(n)
    cutoff = np.full(n, 5000.0)
    best_mult = np.full(n, -1.0)
    mults = np.full((n, max(nl, 1)), -_INF)
    best_local = np.tile(np.array([0.0, 0.0, -1.0]), (n, 1))
    log_scale = np.zeros(n)
    log_weight = np.zeros(n)
    m = np.full(n, _INF, MARGINS_DTYPE)

    for li in range(nl):
        B = np.asarray(listeners["basis"][li], np.float64)
        rel = pos - np.asarray(listeners["origin"][li], np.float64)
        # affine_inverse of an orthonormal transform: the transposed basis; written as sums of products, so that signed
        # zeros come out as in any other such sum
        local = np.stack([B[0, k] * rel[:, 0] + B[1, k] * rel[:, 1] + B[2, k] * rel[:, 2] for k in range(3)], axis=1)
        with np.errstate(over="ignore"):
            dist = np.sqrt((local * local).sum(axis=1))
        att_db, att_margin = attenuation_db(c, s, dist)
        mult = db_to_linear(att_db)
        lap = np.where(area_uniform[:, None], lap_all[:, li], 0.0)
        lap_len = np.sqrt((lap * lap).sum(axis=1))
        total_max = np.where(area_uniform, _max(c["max_distance"], lap_len), c["max_distance"])
        heard = ~(has_max & ((dist > total_max) | (total_max > c["max_distance"])))
        with np.errstate(invalid="ignore", divide="ignore"):
            taper = np.where(has_max, 1.0 - dist / np.where(has_max, c["max_distance"], 1.0), 1.0)
        mult = np.where(has_max, mult * _max(0.0, taper), mult)
        m["dist"] = _closer(m["dist"], dist - total_max, has_max)
        m["taper"] = np.where(has_max & heard, np.minimum(m["taper"], taper), m["taper"])
        m["att"] = _closer(m["att"], att_margin, c["attenuation_model"] != 3)
        in_range |= heard

        db_att = (1.0 - np.where(1.0 < mult, 1.0, mult)) * c["attenuation_filter_db"]
        cone = (c["emission_angle_enabled"] != 0) & heard
        cosine = (_norm(rel) * _norm(s["forward"])).sum(axis=1)
        angle = np.degrees(np.arccos(np.clip(cosine, -1.0, 1.0)))  # Math::acos clamps its argument
        db_att = np.where(cone & (angle > c["emission_angle"]), db_att + c["emission_angle_filter_attenuation_db"], db_att)
        m["cone"] = _closer(m["cone"], angle - c["emission_angle"], cone)
        lin_att = np.where(heard, db_to_linear(db_att), lin_att)  # the last listener in range wins
        cutoff = np.where(heard, c["attenuation_filter_cutoff_hz"], cutoff)

        pan, spcap, spcap_rel, panm, amp = output_vol(c, local)  # the un-normalised position, as the reference passes it (:391)
        tmp = mult[:, None, None] * pan
        taken = heard[:, None, None] & ~(out_vol > tmp)
        out_amp = np.where(taken, amp, out_amp)
        out_vol = np.where(heard[:, None, None], _max(out_vol, tmp), out_vol)
        m["spcap"] = np.where(heard, np.minimum(m["spcap"], spcap), m["spcap"])
        m["spcap_rel"] = np.where(heard, np.minimum(m["spcap_rel"], spcap_rel), m["spcap_rel"])
        m["pan"] = np.where(heard, np.minimum(m["pan"], panm), m["pan"])

        r, rev_margin, rev_att_margin, r_amp = reverb_vol(c, s, uniformity, amount, lap, tmp, amp)
        send = heard & area_reverb
        rev_amp = np.where(send[:, None, None] & ~(rev > r), r_amp, rev_amp)
        rev = np.where(send[:, None, None], _max(rev, r), rev)
        m["rev_att"] = _closer(m["rev_att"], rev_margin, send)
        m["att"] = _closer(m["att"], rev_att_margin, send & (c["attenuation_model"] != 3))

        louder = heard & (mult > best_mult)
        best_local = np.where(louder[:, None], local, best_local)
        best_mult = np.where(louder, mult, best_mult)
        mults[:, li] = np.where(heard, mult, -_INF)

        dv = src_vel - np.asarray(listeners["velocity"][li], np.float64)
        lv = np.stack([B[0, k] * dv[:, 0] + B[1, k] * dv[:, 1] + B[2, k] * dv[:, 2] for k in range(3)], axis=1)
        moving = heard & doppler & (lv != 0).any(axis=1)
        approaching = (_norm(local) * _norm(lv)).sum(axis=1)
        speed = np.sqrt((lv * lv).sum(axis=1))
        sos = c["doppler_speed_of_sound"]
        with np.errstate(divide="ignore", invalid="ignore"):
            dps = np.clip(s["pitch_scale"] * sos / (sos + speed * approaching), 0.125, 8.0)
        weight = np.zeros(n)
        for k in range(4):
            for e in range(2):
                weight = np.where(tmp[:, k, e] > weight, tmp[:, k, e], weight)
        log_scale = np.where(moving, log_scale + weight * np.log2(dps), log_scale)
        log_weight = np.where(moving, log_weight + weight, log_weight)

    with np.errstate(invalid="ignore", divide="ignore"):
        pitch = np.where(log_weight > 0, np.exp2(log_scale / np.where(log_weight > 0, log_weight, 1.0)), s["pitch_scale"])
        top = np.sort(mults, axis=1)[:, ::-1]
        if nl >= 2:
            m["mult_gap"] = np.where(np.isfinite(top[:, 1]), (top[:, 0] - top[:, 1]) / np.where(top[:, 0] > 0, top[:, 0], 1.0), _INF)
    m["spcap_amp"] = np.maximum(out_amp.max(axis=(1, 2)), rev_amp.max(axis=(1, 2)))
    was = np.asarray(was_further) != 0
    n_az, n_el = c["hrtf_n_az"], c["hrtf_n_el"]
    grid = (n_az > 0) & (n_el > 0)
    naz = np.where(grid, n_az, 1)
    u = np.arctan2(best_local[:, 0], -best_local[:, 2]) / (2.0 * np.pi) * naz
    el = np.arctan2(best_local[:, 1], np.sqrt(best_local[:, 0] ** 2 + best_local[:, 2] ** 2))
    v = (el + np.pi / 2.0) / np.pi * (np.where(grid, n_el, 1) - 1)
    ai = np.mod(_round(u).astype(np.int64), naz)
    ei = np.clip(_round(v).astype(np.int64), 0, np.maximum(np.where(grid, n_el, 1) - 1, 0))
    m["az_border"] = np.where(grid, np.abs(np.abs(u - np.floor(u)) - 0.5), _INF)
    m["el_border"] = np.where(grid & (n_el > 1), np.abs(np.abs(v - np.floor(v)) - 0.5), _INF)
    return {
        "mix_volumes": out_vol,
        "pitch_scale": pitch,
        "linear_attenuation": lin_att,
        "attenuation_filter_cutoff_hz": cutoff,
        "update_parameters": np.where(~in_range & was, 0, 1),
        "hrtf_written": grid,
        "hrtf_gain": np.where(grid, np.where(in_range, best_mult, 0.0), 0.0),
        "hrtf_dir": np.where(grid, ei * naz + ai, 0),
        "reverb": rev,
        "in_range": in_range,
        "was_further": (~in_range).astype(np.int32),
        "margins": m,
    }


def badly_placed(margins, border=GUARD_BRANCH):
    """Rows of a random scene that sit on a cancellation or within float32's reach of a branch border."""
    g = margins
    bad = (g["spcap_amp"] > GUARD_SPCAP_AMP) | (g["spcap_rel"] < GUARD_SPCAP_SIGN) | (g["pan"] < GUARD_PAN) | (g["taper"] < GUARD_TAPER)
    # an exact tie is no knife edge: the multipliers are one value (the max_db clamp, attenuation disabled), equal in
    # float32 as well, and the first listener keeps the direction in both
    bad |= (g["mult_gap"] < border) & (g["mult_gap"] > 0)
    for k in ("dist", "att", "rev_att"):
        bad |= np.abs(g[k]) < border
    return bad | (np.abs(g["cone"]) < GUARD_CONE_DEG)


def on_grid_border(margins):
    return (margins["az_border"] < GRID_BORDER) | (margins["el_border"] < GRID_BORDER)
