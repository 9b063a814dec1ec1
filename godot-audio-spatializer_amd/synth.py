"""Seeded synthetic workloads of SURVEY.md section 8(d): sources, SpatializerParameters drawn from the
reference's own pan / attenuation formulas, and a synthetic HRIR set.  Harness-side numpy only
(tests and bench.py); nothing here is on the audio path."""
import numpy as np

from .capi import ER_TAPS, HRTF_BLEND_DTYPE, HRTF_TAPS, PARAMS_DTYPE


def db_to_linear(db):
    # [ENGINE] Math::db_to_linear
    return np.exp(np.asarray(db, dtype=np.float64) * 0.11512925464970228)


def stereo_pan(azimuth, pan_strength=0.5):
    """calc_output_vol_stereo, audio_spatializer_3d.cpp:103-110 (f64). azimuth 0 = front, +pi/2 = right."""
    cosx = np.clip(np.sin(azimuth), -1.0, 1.0)
    g = np.clip((1.0 - pan_strength) ** 2, 0.0, 1.0)
    f = (1.0 - g) / (1.0 + g)
    fcosx = cosx * f
    return np.stack([np.sqrt((-fcosx + 1.0) / 2.0), np.sqrt((fcosx + 1.0) / 2.0)], axis=-1)


def draw_params(rng, n, dirs=1024, channel_count=1, ring_frames=4096, frames=512, unit_size=10.0, filter_db=-24.0, cutoff_hz=5000.0):
    """One physics tick of parameters for n sources: azimuth ~ U(-pi, pi),
    distance ~ logU(1, 100) m, inverse-distance multiplier min(1, unit_size/d)
    (audio_spatializer_3d.cpp:127), high-shelf gain db_to_linear((1 - mult) * -24 dB) (:376,:387)."""
    p = np.zeros(n, dtype=PARAMS_DTYPE)
    az = rng.uniform(-np.pi, np.pi, n)
    d = np.exp(rng.uniform(np.log(1.0), np.log(100.0), n))
    mult = np.minimum(1.0, unit_size / d)
    pan = stereo_pan(az) * mult[:, None]
    p["mix_volumes"][:, 0, :] = pan
    for c in range(1, channel_count):  # surround pairs: independent plausible gains
        p["mix_volumes"][:, c, :] = stereo_pan(rng.uniform(-np.pi, np.pi, n)) * mult[:, None] * 0.5
    p["pitch_scale"] = 1.0
    p["linear_attenuation"] = db_to_linear((1.0 - np.minimum(1.0, mult)) * filter_db)
    p["attenuation_filter_cutoff_hz"] = cutoff_hz
    p["update_parameters"] = 1
    p["hrtf_gain"] = mult
    p["hrtf_dir"] = rng.integers(0, dirs, n)
    p["fx_shelf_gain"] = p["linear_attenuation"]
    p["fx_shelf_cutoff_hz"] = cutoff_hz
    p["er_gain"] = 0.7 ** np.arange(1, ER_TAPS + 1)
    hi = min(4000, ring_frames - frames)
    p["er_delay"] = rng.integers(48, hi + 1, (n, ER_TAPS))
    return p


def draw_sources(rng, n, frames):
    """i.i.d. uniform(-0.5, 0.5) per ear, float32 [n][frames][2]."""
    return rng.uniform(-0.5, 0.5, (n, frames, 2)).astype(np.float32)


def synthetic_hrir(rng, dirs=1024):
    """Decaying noise exp(-k/32) N(0,1) with a per-direction interaural delay."""
    k = np.arange(HRTF_TAPS)
    h = rng.standard_normal((dirs, 2, HRTF_TAPS)) * np.exp(-k / 32.0)
    itd = rng.integers(0, 32, dirs)
    out = np.zeros_like(h)
    for d in range(dirs):
        s = int(itd[d])
        out[d, 0, :] = h[d, 0, :]
        out[d, 1, s:] = h[d, 1, : HRTF_TAPS - s]
    return (out * 0.25).astype(np.float32)


def draw_blends(rng, n, dirs):
    """n gas_hrtf_blend rows (FLAG_HRTF_INTERPOLATE): 1 .. 4 non-zero weights summing to 1, at random positions of the
    row, each on a direction of its own; the other entries are zero (their directions are not read)."""
    b = np.zeros(n, dtype=HRTF_BLEND_DTYPE)
    for i in range(n):
        k = int(rng.integers(1, 5))
        pos = np.sort(rng.choice(4, size=k, replace=False))
        w = rng.uniform(0.1, 1.0, k)
        b["weight"][i, pos] = (w / w.sum()).astype(np.float32)
        b["dir"][i, pos] = rng.choice(dirs, size=k, replace=dirs < k)
    return b


def draw_room_scene(rng, n, n_rooms=4):
    """A scene for gas_calc_early_reflections: (rooms ROOM_DTYPE [n_rooms], room_index uint32 [n], poses POSE_DTYPE [n],
    listener LISTENER_DTYPE [1]).  Axis-aligned boxes around one listener at the origin, half-extents 2 .. 10 m, wall
    reflectances 0.3 .. 0.95; every source uniform inside its room."""
    from .capi import LISTENER_DTYPE, POSE_DTYPE, default_rooms

    rooms = default_rooms(n_rooms)
    rooms["half_extent"] = rng.uniform(2.0, 10.0, (n_rooms, 3))
    rooms["origin"] = rng.uniform(-0.5, 0.5, (n_rooms, 3)) * rooms["half_extent"]
    rooms["reflectance"] = rng.uniform(0.3, 0.95, (n_rooms, 6))
    room_index = rng.integers(0, n_rooms, n).astype(np.uint32)
    poses = np.zeros(n, POSE_DTYPE)
    poses["position"] = rooms["origin"][room_index] + rng.uniform(-0.98, 0.98, (n, 3)) * rooms["half_extent"][room_index]
    poses["pitch_scale"] = 1.0
    listener = np.zeros(1, LISTENER_DTYPE)
    listener["basis"] = np.eye(3, dtype=np.float32)
    return rooms, room_index, poses, listener
