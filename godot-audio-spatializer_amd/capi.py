"""ctypes binding of libgas_amd.so (include/gas_amd.h).

Fails loudly when the HIP library is missing or cannot be loaded: there is no CPU path.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

MAX_CHANNELS = 4
LOOKAHEAD = 64
HRTF_TAPS = 256
ER_TAPS = 8

KIND_3D_MIX = 0
KIND_3D_PROCESS = 1
KIND_EFFECT = 2
FX_HIGHSHELF = 1
FX_EARLY_REFLECTIONS = 2
FX_HRTF = 3
FX_LOWPASS, FX_HIGHPASS, FX_BANDPASS, FX_NOTCH, FX_LOWSHELF, FX_AMPLIFY = 4, 5, 6, 7, 8, 9
MAX_EFFECTS = 4
MAX_SIDECHAINS = 8  # GAS_MAX_SIDECHAINS: key blocks per context (SpatializerContext.sidechain_set)
# gas_fx_settings: settings of the engine-effect kinds by chain position (64 bytes)
FX_SETTINGS_DTYPE = np.dtype([("filter_cutoff_hz", np.float32, (MAX_EFFECTS,)), ("filter_resonance", np.float32, (MAX_EFFECTS,)), ("filter_gain", np.float32, (MAX_EFFECTS,)), ("amplify_volume_db", np.float32, (MAX_EFFECTS,))])
# the engine's nonlinear / dynamics kinds (10 is not assigned); settings: gas_fx_dyn_settings by chain position
FX_DISTORTION, FX_COMPRESSOR = 11, 12
DISTORTION_CLIP, DISTORTION_ATAN, DISTORTION_LOFI, DISTORTION_OVERDRIVE, DISTORTION_WAVESHAPE = 0, 1, 2, 3, 4
FX_DYN_SETTINGS_DTYPE = np.dtype(
    [
        ("distortion_mode", np.int32, (MAX_EFFECTS,)),
        ("distortion_pre_gain_db", np.float32, (MAX_EFFECTS,)),
        ("distortion_keep_hf_hz", np.float32, (MAX_EFFECTS,)),
        ("distortion_drive", np.float32, (MAX_EFFECTS,)),
        ("distortion_post_gain_db", np.float32, (MAX_EFFECTS,)),
        ("compressor_threshold_db", np.float32, (MAX_EFFECTS,)),
        ("compressor_ratio", np.float32, (MAX_EFFECTS,)),
        ("compressor_gain_db", np.float32, (MAX_EFFECTS,)),
        ("compressor_attack_us", np.float32, (MAX_EFFECTS,)),
        ("compressor_release_ms", np.float32, (MAX_EFFECTS,)),
        ("compressor_mix", np.float32, (MAX_EFFECTS,)),
        ("compressor_sidechain", np.uint32, (MAX_EFFECTS,)),  # 0: none, k: key k - 1 of the context
    ]
)
assert FX_DYN_SETTINGS_DTYPE.itemsize == 192


def fx_dyn_settings_defaults(n):
    """[ENGINE] AudioEffectDistortion / AudioEffectCompressor resource defaults, n rows."""
    d = np.zeros(n, FX_DYN_SETTINGS_DTYPE)
    d["distortion_mode"] = DISTORTION_CLIP
    d["distortion_keep_hf_hz"] = 16000.0
    d["compressor_ratio"] = 4.0
    d["compressor_attack_us"] = 20.0
    d["compressor_release_ms"] = 250.0
    d["compressor_mix"] = 1.0
    return d


# the engine's delay and reverb (one "line" of delay memory per instance, gas_ctx_reserve_fx_lines); settings:
# gas_fx_line_settings by chain position
FX_DELAY, FX_REVERB = 13, 14
FX_LINE_SETTINGS_DTYPE = np.dtype(
    [
        ("delay_dry", np.float32, (MAX_EFFECTS,)),
        ("delay_tap1_active", np.int32, (MAX_EFFECTS,)),
        ("delay_tap1_ms", np.float32, (MAX_EFFECTS,)),
        ("delay_tap1_level_db", np.float32, (MAX_EFFECTS,)),
        ("delay_tap1_pan", np.float32, (MAX_EFFECTS,)),
        ("delay_tap2_active", np.int32, (MAX_EFFECTS,)),
        ("delay_tap2_ms", np.float32, (MAX_EFFECTS,)),
        ("delay_tap2_level_db", np.float32, (MAX_EFFECTS,)),
        ("delay_tap2_pan", np.float32, (MAX_EFFECTS,)),
        ("delay_feedback_active", np.int32, (MAX_EFFECTS,)),
        ("delay_feedback_ms", np.float32, (MAX_EFFECTS,)),
        ("delay_feedback_level_db", np.float32, (MAX_EFFECTS,)),
        ("delay_feedback_lowpass_hz", np.float32, (MAX_EFFECTS,)),
        ("reverb_predelay_ms", np.float32, (MAX_EFFECTS,)),
        ("reverb_predelay_feedback", np.float32, (MAX_EFFECTS,)),
        ("reverb_room_size", np.float32, (MAX_EFFECTS,)),
        ("reverb_damping", np.float32, (MAX_EFFECTS,)),
        ("reverb_spread", np.float32, (MAX_EFFECTS,)),
        ("reverb_hipass", np.float32, (MAX_EFFECTS,)),
        ("reverb_dry", np.float32, (MAX_EFFECTS,)),
        ("reverb_wet", np.float32, (MAX_EFFECTS,)),
    ]
)
assert FX_LINE_SETTINGS_DTYPE.itemsize == 336


def fx_line_settings_defaults(n):
    """[ENGINE] AudioEffectDelay / AudioEffectReverb resource defaults, n rows."""
    d = np.zeros(n, FX_LINE_SETTINGS_DTYPE)
    for name, v in (
        ("delay_dry", 1.0),
        ("delay_tap1_active", 1),
        ("delay_tap1_ms", 250.0),
        ("delay_tap1_level_db", -6.0),
        ("delay_tap1_pan", 0.2),
        ("delay_tap2_active", 1),
        ("delay_tap2_ms", 500.0),
        ("delay_tap2_level_db", -12.0),
        ("delay_tap2_pan", -0.4),
        ("delay_feedback_active", 0),
        ("delay_feedback_ms", 340.0),
        ("delay_feedback_level_db", -6.0),
        ("delay_feedback_lowpass_hz", 16000.0),
        ("reverb_predelay_ms", 150.0),
        ("reverb_predelay_feedback", 0.4),
        ("reverb_room_size", 0.8),
        ("reverb_damping", 0.5),
        ("reverb_spread", 1.0),
        ("reverb_hipass", 0.0),
        ("reverb_dry", 1.0),
        ("reverb_wet", 0.5),
    ):
        d[name] = v
    return d


# the engine's graphic equalisers (one "bank" of state per instance, gas_ctx_reserve_fx_eq); settings:
# gas_fx_eq_settings, band gains in dB by chain position, then band
FX_EQ6, FX_EQ10, FX_EQ21 = 16, 17, 18
EQ_MAX_BANDS = 21
EQ_BANDS = {FX_EQ6: 6, FX_EQ10: 10, FX_EQ21: 21}
FX_EQ_SETTINGS_DTYPE = np.dtype([("band_gain_db", np.float32, (MAX_EFFECTS, EQ_MAX_BANDS))])
assert FX_EQ_SETTINGS_DTYPE.itemsize == 336


def fx_eq_settings_defaults(n):
    """0 dB at every position and band, n rows (what a slot starts with)."""
    return np.zeros(n, FX_EQ_SETTINGS_DTYPE)


# the engine's chorus and phaser (one chorus "line" / phaser "bank" per instance, gas_ctx_reserve_fx_mod); settings:
# gas_fx_mod_settings by chain position (then voice for the chorus's per-voice arrays)
FX_CHORUS, FX_PHASER = 19, 20
CHORUS_MAX_VOICES = 4
_PV = (MAX_EFFECTS, CHORUS_MAX_VOICES)
FX_MOD_SETTINGS_DTYPE = np.dtype(
    [
        ("chorus_voice_count", np.int32, (MAX_EFFECTS,)),
        ("chorus_dry", np.float32, (MAX_EFFECTS,)),
        ("chorus_wet", np.float32, (MAX_EFFECTS,)),
        ("chorus_delay_ms", np.float32, _PV),
        ("chorus_rate_hz", np.float32, _PV),
        ("chorus_depth_ms", np.float32, _PV),
        ("chorus_level_db", np.float32, _PV),
        ("chorus_cutoff_hz", np.float32, _PV),
        ("chorus_pan", np.float32, _PV),
        ("phaser_range_min_hz", np.float32, (MAX_EFFECTS,)),
        ("phaser_range_max_hz", np.float32, (MAX_EFFECTS,)),
        ("phaser_rate_hz", np.float32, (MAX_EFFECTS,)),
        ("phaser_feedback", np.float32, (MAX_EFFECTS,)),
        ("phaser_depth", np.float32, (MAX_EFFECTS,)),
    ]
)
assert FX_MOD_SETTINGS_DTYPE.itemsize == 512


def fx_mod_settings_defaults(n):
    """The engine's AudioEffectChorus / AudioEffectPhaser defaults at every position, n rows (what a slot starts with)."""
    d = np.zeros(n, FX_MOD_SETTINGS_DTYPE)
    d["chorus_voice_count"] = 2
    d["chorus_dry"] = 1.0
    d["chorus_wet"] = 0.5
    d["chorus_delay_ms"] = (15.0, 20.0, 12.0, 12.0)
    d["chorus_rate_hz"] = (0.8, 1.2, 1.0, 1.0)
    d["chorus_depth_ms"] = (2.0, 3.0, 0.0, 0.0)
    d["chorus_cutoff_hz"] = (8000.0, 8000.0, 16000.0, 16000.0)
    d["chorus_pan"] = (-0.5, 0.5, 0.0, 0.0)
    d["phaser_range_min_hz"] = 440.0
    d["phaser_range_max_hz"] = 1600.0
    d["phaser_rate_hz"] = 0.5
    d["phaser_feedback"] = 0.7
    d["phaser_depth"] = 1.0
    return d


# the engine's panner, stereo enhance and limiter (no recurrence over frames; one mono "ring" per stereo enhance,
# gas_ctx_reserve_fx_stereo; panner and limiter hold no state); settings: gas_fx_stereo_settings by chain position
FX_PANNER, FX_STEREO_ENHANCE, FX_LIMITER = 21, 22, 23
FX_STEREO_SETTINGS_DTYPE = np.dtype(
    [
        ("panner_pan", np.float32, (MAX_EFFECTS,)),
        ("enhance_pan_pullout", np.float32, (MAX_EFFECTS,)),
        ("enhance_time_pullout_ms", np.float32, (MAX_EFFECTS,)),
        ("enhance_surround", np.float32, (MAX_EFFECTS,)),
        ("limiter_ceiling_db", np.float32, (MAX_EFFECTS,)),
        ("limiter_threshold_db", np.float32, (MAX_EFFECTS,)),
        ("limiter_soft_clip_db", np.float32, (MAX_EFFECTS,)),
        ("limiter_soft_clip_ratio", np.float32, (MAX_EFFECTS,)),
    ]
)
assert FX_STEREO_SETTINGS_DTYPE.itemsize == 128


def fx_stereo_settings_defaults(n):
    """The engine's AudioEffectPanner / StereoEnhance / Limiter defaults at every position, n rows (what a slot starts with)."""
    d = np.zeros(n, FX_STEREO_SETTINGS_DTYPE)
    d["enhance_pan_pullout"] = 1.0
    d["limiter_ceiling_db"] = -0.1
    d["limiter_soft_clip_db"] = 2.0
    d["limiter_soft_clip_ratio"] = 10.0
    return d


# the engine's AudioEffectFilter at any slope and AudioEffectBandLimitFilter (one "bank" of state per instance,
# gas_ctx_reserve_fx_filter); settings: gas_fx_filter_settings by chain position
FX_FILTER = 24
FILTER_LOWPASS, FILTER_HIGHPASS, FILTER_BANDPASS, FILTER_NOTCH, FILTER_LOWSHELF, FILTER_HIGHSHELF, FILTER_BANDLIMIT = range(7)
FILTER_6DB, FILTER_12DB, FILTER_18DB, FILTER_24DB = range(4)
FX_FILTER_SETTINGS_DTYPE = np.dtype(
    [
        ("type", np.int32, (MAX_EFFECTS,)),
        ("db", np.int32, (MAX_EFFECTS,)),
        ("cutoff_hz", np.float32, (MAX_EFFECTS,)),
        ("resonance", np.float32, (MAX_EFFECTS,)),
        ("gain", np.float32, (MAX_EFFECTS,)),
        ("reserved", np.uint32, (12,)),
    ]
)
assert FX_FILTER_SETTINGS_DTYPE.itemsize == 128


class FxFilterSettings(C.Structure):
    """gas_fx_filter_settings for callers that use ctypes directly."""

    _fields_ = [
        ("type", C.c_int32 * MAX_EFFECTS),
        ("db", C.c_int32 * MAX_EFFECTS),
        ("cutoff_hz", C.c_float * MAX_EFFECTS),
        ("resonance", C.c_float * MAX_EFFECTS),
        ("gain", C.c_float * MAX_EFFECTS),
        ("reserved", C.c_uint32 * 12),
    ]


assert C.sizeof(FxFilterSettings) == 128


def fx_filter_settings_defaults(n):
    """The engine's AudioEffectFilter defaults at every position, n rows (what a slot starts with): low-pass, 6 dB."""
    d = np.zeros(n, FX_FILTER_SETTINGS_DTYPE)
    d["type"] = FILTER_LOWPASS
    d["db"] = FILTER_6DB
    d["cutoff_hz"] = 2000.0
    d["resonance"] = 0.5
    d["gain"] = 1.0
    return d


# gas_hrtf_blend (GAS_FLAG_HRTF_INTERPOLATE): the HRIR rows one playback's HRTF stage blends; all-zero = no blend
HRTF_BLEND_DTYPE = np.dtype([("dir", np.uint32, (4,)), ("weight", np.float32, (4,))])
assert HRTF_BLEND_DTYPE.itemsize == 32


class HrtfBlend(C.Structure):
    """gas_hrtf_blend for callers that use ctypes directly."""

    _fields_ = [("dir", C.c_uint32 * 4), ("weight", C.c_float * 4)]


assert C.sizeof(HrtfBlend) == 32

MEM_HOST = 0
MEM_DEVICE = 1
# gas_pcm_format (gas_stream_create)
PCM_S16 = 0
PCM_F32 = 1
PCM_IMA_ADPCM = 2
PCM_QOA = 3


def qoa_file_bytes(frames, channels):
    """Bytes of the QOA file of a stream (include/gas_amd.h): 8, and per 5120 frames 8 + 16 * channels + 8 * slices *
    channels with slices = ceil(frames in it / 20)."""
    full, rest = divmod(int(frames), 5120)
    per = lambda n: 8 + 16 * channels + 8 * ((n + 19) // 20) * channels  # noqa: E731
    return 8 + full * per(5120) + (per(rest) if rest else 0)


# gas_loop_mode (gas_stream_set_loop)
LOOP_DISABLED = 0
LOOP_FORWARD = 1
LOOP_PINGPONG = 2
FLAG_PEAKS_DRAINING_ONLY = 1
FLAG_HRTF_CROSSFADE = 2
FLAG_DIRECTION_ORDER = 4
FLAG_PIPELINED_MIX = 8
FLAG_DIRECTION_RUNS = 16
FLAG_XCD_ORDER = 32
FLAG_BATCHED_LAUNCH = 64
FLAG_HRTF_INTERPOLATE = 128
FLAG_HRTF_BLEND_FADE = 256  # with FLAG_HRTF_INTERPOLATE only: fade from the previous callback's blend to this one's
FLAG_ER_TAP_FADE = 512  # fade early-reflection taps from the row a slot last rendered with to this callback's (needs er_ring_frames)

STATUS = {
    0: "GAS_OK",
    -1: "GAS_ERR_INVALID_ARGUMENT",
    -2: "GAS_ERR_OUT_OF_SLOTS",
    -3: "GAS_ERR_BAD_SLOT",
    -4: "GAS_ERR_FRAME_COUNT",
    -5: "GAS_ERR_NO_HRTF",
    -6: "GAS_ERR_UNSUPPORTED_CHAIN",
    -7: "GAS_ERR_DEVICE",
    -8: "GAS_ERR_NO_DEVICE",
    -9: "GAS_ERR_OUT_OF_MEMORY",
    -10: "GAS_ERR_KIND_MISMATCH",
    -11: "GAS_ERR_BAD_CHANNEL",
    -12: "GAS_ERR_NO_PARAMS",
}

# gas_params, 128 bytes (include/gas_amd.h)
PARAMS_DTYPE = np.dtype(
    [
        ("mix_volumes", np.float32, (MAX_CHANNELS, 2)),
        ("pitch_scale", np.float32),
        ("linear_attenuation", np.float32),
        ("attenuation_filter_cutoff_hz", np.float32),
        ("update_parameters", np.uint32),
        ("hrtf_gain", np.float32),
        ("hrtf_dir", np.uint32),
        ("fx_shelf_gain", np.float32),
        ("fx_shelf_cutoff_hz", np.float32),
        ("er_gain", np.float32, (ER_TAPS,)),
        ("er_delay", np.uint32, (ER_TAPS,)),
    ]
)
assert PARAMS_DTYPE.itemsize == 128


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("max_sources", C.c_uint32),
        ("frames", C.c_uint32),
        ("channel_count", C.c_uint32),
        ("mix_rate", C.c_float),
        ("er_ring_frames", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class Profile(C.Structure):
    _fields_ = [
        ("launches", C.c_uint64),
        ("kernel_ms", C.c_double),
        ("bytes_per_launch", C.c_uint64),
        ("kernel_name", C.c_char * 64),
        ("callbacks_per_launch", C.c_uint32),
        ("reserved", C.c_uint32),
        ("bytes_per_callback_formula", C.c_uint64),
    ]


SPAT3D_CONFIG_DTYPE = np.dtype(
    [
        ("attenuation_model", np.int32),
        ("unit_size", np.float32),
        ("max_distance", np.float32),
        ("panning_strength", np.float32),
        ("emission_angle_enabled", np.int32),
        ("emission_angle", np.float32),
        ("emission_angle_filter_attenuation_db", np.float32),
        ("attenuation_filter_cutoff_hz", np.float32),
        ("attenuation_filter_db", np.float32),
        ("doppler_tracking", np.int32),
        ("doppler_speed_of_sound", np.float32),
        ("global_panning_strength", np.float32),
        ("speaker_mode", np.int32),
        ("hrtf_n_az", np.uint32),
        ("hrtf_n_el", np.uint32),
        ("reserved", np.uint32),
    ]
)
POSE_DTYPE = np.dtype([("position", np.float32, (3,)), ("volume_db", np.float32), ("velocity", np.float32, (3,)), ("max_db", np.float32), ("forward", np.float32, (3,)), ("pitch_scale", np.float32)])
AREA_SEND_DTYPE = np.dtype([("using_reverb_bus", np.uint32), ("reverb_uniformity", np.float32), ("reverb_amount", np.float32), ("present", np.uint32)])
MAX_MORE_SENDS = 4
BUS_ROUTE_DTYPE = np.dtype([("dry_bus", np.uint32), ("send_bus", np.uint32), ("send", np.float32, (MAX_CHANNELS, 2)), ("more_bus", np.uint32, (MAX_MORE_SENDS,)), ("more_send", np.float32, (MAX_MORE_SENDS, MAX_CHANNELS, 2))])
BUS_NONE = 0xFFFFFFFF


def bus_routes(n):
    """n default routes: dry bus 0, no sends (gas_bus_route with every send slot GAS_BUS_NONE)."""
    r = np.zeros(n, BUS_ROUTE_DTYPE)
    r["send_bus"] = BUS_NONE
    r["more_bus"] = BUS_NONE
    return r
LISTENER_DTYPE = np.dtype([("basis", np.float32, (3, 3)), ("origin", np.float32, (3,)), ("velocity", np.float32, (3,)), ("pad", np.float32)])
assert SPAT3D_CONFIG_DTYPE.itemsize == 64 and POSE_DTYPE.itemsize == 48 and LISTENER_DTYPE.itemsize == 64
# gas_room / gas_er_taps (gas_calc_early_reflections)
MAX_ROOMS = 64
ROOM_NONE = 0xFFFFFFFF
ROOM_DTYPE = np.dtype([("basis", np.float32, (3, 3)), ("origin", np.float32, (3,)), ("half_extent", np.float32, (3,)), ("reflectance", np.float32, (6,)), ("speed_of_sound", np.float32), ("level", np.float32), ("max_order", np.uint32)])
ER_TAPS_DTYPE = np.dtype([("gain", np.float32, (ER_TAPS,)), ("delay", np.uint32, (ER_TAPS,))])
assert ROOM_DTYPE.itemsize == 96 and ER_TAPS_DTYPE.itemsize == 64
# gas_room_ir (gas_conv_ir_from_room)
ROOM_IR_DTYPE = np.dtype([("room", ROOM_DTYPE), ("source", np.float32, (3,)), ("listener", LISTENER_DTYPE), ("ear_spacing", np.float32), ("min_order", np.uint32), ("max_order", np.uint32)])
assert ROOM_IR_DTYPE.itemsize == 184


def default_rooms(n=1, **kw):
    """n box rooms: identity basis at the origin, 4 x 2.5 x 3 m half-extents, every wall 0.8, 343 m/s, level 1, second order."""
    r = np.zeros(n, ROOM_DTYPE)
    r["basis"] = np.eye(3, dtype=np.float32)
    r["half_extent"] = (4.0, 2.5, 3.0)
    r["reflectance"] = 0.8
    r["speed_of_sound"] = 343.0
    r["level"] = 1.0
    r["max_order"] = 2
    for k, v in kw.items():
        r[k] = v
    return r


def default_room_ir(room=None, source=(1.0, 0.5, 0.25), listener_origin=(-1.0, 0.0, 0.0), ear_spacing=0.18, min_order=0, max_order=0):
    """One gas_room_ir ([1]): `room` (a ROOM_DTYPE entry; default default_rooms()) heard by a listener with the identity
    basis at listener_origin from an emitter at `source`, ears 18 cm apart, every order the IR's length reaches."""
    d = np.zeros(1, ROOM_IR_DTYPE)
    d["room"] = (default_rooms() if room is None else np.asarray(room).reshape(-1))[0]
    d["source"] = source
    d["listener"]["basis"] = np.eye(3, dtype=np.float32)
    d["listener"]["origin"] = listener_origin
    d["ear_spacing"] = ear_spacing
    d["min_order"], d["max_order"] = min_order, max_order
    return d


# gas_room_plane / gas_room_planes (gas_conv_ir_from_planes)
ROOM_MAX_PLANES = 16
ROOM_PLANES_MAX_ORDER = 8
ROOM_PLANE_DTYPE = np.dtype([("normal", np.float32, (3,)), ("offset", np.float32), ("reflectance", np.float32)])
ROOM_PLANES_DTYPE = np.dtype([("planes", ROOM_PLANE_DTYPE, (ROOM_MAX_PLANES,)), ("n_planes", np.uint32), ("speed_of_sound", np.float32), ("level", np.float32), ("source", np.float32, (3,)), ("listener", LISTENER_DTYPE), ("ear_spacing", np.float32), ("min_order", np.uint32), ("max_order", np.uint32)])
assert ROOM_PLANE_DTYPE.itemsize == 20 and ROOM_PLANES_DTYPE.itemsize == 420


def planes_from_box(room):
    """The six walls of a gas_room (one ROOM_DTYPE entry) as ROOM_PLANE_DTYPE [6], in gas_room's wall order -x, +x, -y,
    +y, -z, +z: inward normals are the basis' columns and their negatives, offsets are worked out in float64 and stored
    as float32 (exact for an axis-aligned box whose origin and half-extents are short binary fractions)."""
    r = np.asarray(room, dtype=ROOM_DTYPE).reshape(-1)[0]
    B, o, h = r["basis"].astype(np.float64), r["origin"].astype(np.float64), r["half_extent"].astype(np.float64)
    p = np.zeros(6, ROOM_PLANE_DTYPE)
    for a in range(3):
        for side, sign in ((0, 1.0), (1, -1.0)):  # the -a wall looks along +a
            n = sign * B[:, a]
            p[2 * a + side] = (n, float(n @ o) - h[a], r["reflectance"][2 * a + side])
    return p


def default_room_planes(planes=None, source=(1.0, 1.2, 0.5), listener_origin=(-1.0, 1.5, -0.75), ear_spacing=0.18, min_order=0, max_order=3, speed_of_sound=343.0, level=1.0):
    """One gas_room_planes ([1]).  planes: ROOM_PLANE_DTYPE [P] (or rows of (normal, offset, reflectance)); by default an
    attic of seven planes, every one 0.8: a floor at y = 0, walls at x = -+3 and z = -+4, and two roof slopes from the
    eaves at y = 1.5 to a ridge at y = 3.5 above x = 0.  Identity listener basis, ears 18 cm apart, orders 0 .. 3."""
    if planes is None:
        k = 13.0**-0.5
        planes = [((0, 1, 0), 0.0, 0.8), ((1, 0, 0), -3.0, 0.8), ((-1, 0, 0), -3.0, 0.8), ((0, 0, 1), -4.0, 0.8), ((0, 0, -1), -4.0, 0.8), ((-2 * k, -3 * k, 0), -10.5 * k, 0.8), ((2 * k, -3 * k, 0), -10.5 * k, 0.8)]
    planes = np.asarray(planes, dtype=ROOM_PLANE_DTYPE).reshape(-1)
    assert 1 <= len(planes) <= ROOM_MAX_PLANES
    d = np.zeros(1, ROOM_PLANES_DTYPE)
    d["planes"][0, : len(planes)] = planes
    d["n_planes"] = len(planes)
    d["speed_of_sound"], d["level"] = speed_of_sound, level
    d["source"] = source
    d["listener"]["basis"] = np.eye(3, dtype=np.float32)
    d["listener"]["origin"] = listener_origin
    d["ear_spacing"] = ear_spacing
    d["min_order"], d["max_order"] = min_order, max_order
    return d


# gas_room_bands (gas_conv_ir_from_room_bands, gas_conv_ir_from_room_hrtf_bands)
ROOM_MAX_BANDS = 8
ROOM_BAND_FILTER_MAX_TAPS = 4095
ROOM_BANDS_DTYPE = np.dtype([("n_bands", np.uint32), ("filter_taps", np.uint32), ("crossover_hz", np.float32, (ROOM_MAX_BANDS - 1,)), ("reflectance", np.float32, (ROOM_MAX_BANDS, 6)), ("air_db_per_m", np.float32, (ROOM_MAX_BANDS,)), ("reserved", np.uint32)])
assert ROOM_BANDS_DTYPE.itemsize == 264


def default_room_bands(crossover_hz=(500.0, 4000.0), reflectance=((0.9,) * 6, (0.8,) * 6, (0.6,) * 6), air_db_per_m=(0.0, 0.005, 0.05), filter_taps=255):
    """One gas_room_bands ([1]) of len(reflectance) bands: by default low / mid / high split at 500 Hz and 4 kHz, walls
    that absorb more towards the highs, air that takes 0.05 dB per metre from the high band, 255-tap band filters.
    reflectance: one value or six (gas_room's wall order) per band."""
    n = len(reflectance)
    assert 1 <= n <= ROOM_MAX_BANDS and len(crossover_hz) == n - 1 and len(air_db_per_m) == n
    b = np.zeros(1, ROOM_BANDS_DTYPE)
    b["n_bands"], b["filter_taps"] = n, filter_taps
    b["crossover_hz"][0, : n - 1] = crossover_hz
    for i in range(n):
        b["reflectance"][0, i] = reflectance[i]
    b["air_db_per_m"][0, :n] = air_db_per_m
    return b


# gas_room_tail (gas_conv_ir_from_room_diffuse, gas_conv_ir_from_room_hrtf_diffuse)
ROOM_TAIL_DTYPE = np.dtype([("seed", np.uint32), ("mix_time_s", np.float32), ("fade_s", np.float32), ("gain", np.float32), ("reserved", np.uint32, (4,))])
assert ROOM_TAIL_DTYPE.itemsize == 32


def default_room_tail(seed=0, mix_time_s=0.08, fade_s=0.02, gain=1.0):
    """One gas_room_tail ([1]): image sources for the first 80 ms after the direct sound, then 20 ms of cross-fade into
    the diffuse tail at the rule's level."""
    t = np.zeros(1, ROOM_TAIL_DTYPE)
    t["seed"], t["mix_time_s"], t["fade_s"], t["gain"] = seed, mix_time_s, fade_s, gain
    return t


def default_spat3d_config(n=1, **kw):
    """AudioSpatializer3D defaults (audio_spatializer_3d.h:171-187), stereo, global panning strength 0.5."""
    c = np.zeros(n, SPAT3D_CONFIG_DTYPE)
    c["unit_size"] = 10.0
    c["panning_strength"] = 1.0
    c["emission_angle"] = 45.0
    c["emission_angle_filter_attenuation_db"] = -12.0
    c["attenuation_filter_cutoff_hz"] = 5000.0
    c["attenuation_filter_db"] = -24.0
    c["doppler_speed_of_sound"] = 343.0
    c["global_panning_strength"] = 0.5
    for k, v in kw.items():
        c[k] = v
    return c


# every symbol include/gas_amd.h declares
EXPORTS = [
    "gas_abi_version",
    "gas_ctx_create",
    "gas_ctx_destroy",
    "gas_ctx_set_stream",
    "gas_ctx_synchronize",
    "gas_ctx_join_outputs",
    "gas_ctx_get_config",
    "gas_strerror",
    "gas_last_device_error",
    "gas_source_alloc",
    "gas_source_free",
    "gas_source_reset",
    "gas_source_set_draining",
    "gas_params_publish",
    "gas_fx_settings_publish",
    "gas_fx_dyn_settings_publish",
    "gas_sidechain_set",
    "gas_fx_line_settings_publish",
    "gas_ctx_reserve_fx_lines",
    "gas_fx_eq_settings_publish",
    "gas_ctx_reserve_fx_eq",
    "gas_fx_mod_settings_publish",
    "gas_ctx_reserve_fx_mod",
    "gas_fx_stereo_settings_publish",
    "gas_ctx_reserve_fx_stereo",
    "gas_fx_filter_settings_publish",
    "gas_ctx_reserve_fx_filter",
    "gas_params_publish_batch",
    "gas_hrtf_load",
    "gas_hrtf_blend_publish",
    "gas_hrtf_load_positions",
    "gas_calc_spatialization",
    "gas_calc_spatialization_areas",
    "gas_calc_early_reflections",
    "gas_stream_create",
    "gas_stream_destroy",
    "gas_stream_get_info",
    "gas_stream_positions",
    "gas_stream_set_resampled",
    "gas_stream_set_loop",
    "gas_stream_get_loop",
    "gas_source_bind_stream",
    "gas_process_block_streams",
    "gas_process_block_streams_buses",
    "gas_source_feed_rows",
    "gas_stream_last_fused",
    "gas_process_block",
    "gas_bus_routes_publish",
    "gas_process_block_buses",
    "gas_ctx_reserve_conv",
    "gas_conv_ir_load",
    "gas_conv_ir_free",
    "gas_conv_ir_get_info",
    "gas_conv_ir_from_room",
    "gas_conv_ir_from_planes",
    "gas_conv_ir_from_room_hrtf",
    "gas_conv_ir_from_room_bands",
    "gas_conv_ir_from_room_hrtf_bands",
    "gas_conv_ir_from_room_diffuse",
    "gas_conv_ir_from_room_hrtf_diffuse",
    "gas_conv_create",
    "gas_conv_destroy",
    "gas_conv_reset",
    "gas_conv_set_ir",
    "gas_conv_set_levels",
    "gas_conv_fade_to",
    "gas_conv_fade_remaining",
    "gas_conv_process",
    "gas_process_frames_1",
    "gas_mix_channel_1",
    "gas_profile_enable",
    "gas_profile_read",
    "gas_bandwidth_probe",
    "gas_ctx_set_batch_depth",
    "gas_ctx_read_hrtf_order",
    "gas_tune_uni12_min",
    "gas_tune_nt_hist_min",
]


class GasError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        name = STATUS.get(status, str(status))
        super().__init__(f"{where}: {name}" + (f" ({detail})" if detail else ""))


_lib = None


def library_path():
    # GAS_AMD_LIB: development override for A/B-ing kernel builds (tools/README.md); never a fallback
    return os.environ.get("GAS_AMD_LIB") or _build.LIB


def load_library():
    """Load libgas_amd.so; raises if it was never built (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The spatializer has no CPU fallback."
        )
    # PyTorch-ROCm wheels bundle their own libamdhip64; two HIP runtimes in one process leave the
    # second one without devices.  Import torch first (when present) so libgas_amd.so binds to the
    # runtime torch already loaded (same soname) and streams/pointers can be shared with it.
    if os.environ.get("GAS_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(path)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    L.gas_abi_version.restype = i32
    L.gas_ctx_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.gas_ctx_destroy.argtypes = [vp]
    L.gas_ctx_destroy.restype = None
    L.gas_ctx_set_stream.argtypes = [vp, vp]
    L.gas_ctx_synchronize.argtypes = [vp]
    L.gas_ctx_join_outputs.argtypes = [vp]
    L.gas_ctx_get_config.argtypes = [vp, C.POINTER(Config)]
    L.gas_strerror.argtypes = [i32]
    L.gas_strerror.restype = C.c_char_p
    L.gas_last_device_error.argtypes = [vp]
    L.gas_last_device_error.restype = C.c_char_p
    L.gas_source_alloc.argtypes = [vp, i32, C.POINTER(C.c_int32), u32, C.POINTER(u32)]
    L.gas_source_free.argtypes = [vp, u32]
    L.gas_source_reset.argtypes = [vp, u32]
    L.gas_source_set_draining.argtypes = [vp, u32, i32]
    L.gas_params_publish.argtypes = [vp, u32, vp]
    L.gas_fx_settings_publish.argtypes = [vp, vp, vp, u32]
    L.gas_fx_dyn_settings_publish.argtypes = [vp, vp, vp, u32]
    L.gas_sidechain_set.argtypes = [vp, u32, vp, u32, i32]
    L.gas_fx_line_settings_publish.argtypes = [vp, vp, vp, u32]
    L.gas_ctx_reserve_fx_lines.argtypes = [vp, u32, u32]
    L.gas_fx_eq_settings_publish.argtypes = [vp, vp, vp, u32]
    L.gas_ctx_reserve_fx_eq.argtypes = [vp, u32]
    L.gas_fx_mod_settings_publish.argtypes = [vp, vp, vp, u32]
    L.gas_ctx_reserve_fx_mod.argtypes = [vp, u32, u32]
    L.gas_fx_stereo_settings_publish.argtypes = [vp, vp, vp, u32]
    L.gas_ctx_reserve_fx_stereo.argtypes = [vp, u32]
    L.gas_fx_filter_settings_publish.argtypes = [vp, vp, vp, u32]
    L.gas_ctx_reserve_fx_filter.argtypes = [vp, u32]
    L.gas_params_publish_batch.argtypes = [vp, vp, vp, u32, i32]
    L.gas_hrtf_load.argtypes = [vp, vp, u32, u32]
    L.gas_hrtf_blend_publish.argtypes = [vp, vp, vp, u32]
    L.gas_hrtf_load_positions.argtypes = [vp, vp, vp, u32, u32, u32, u32, i32, vp]
    L.gas_stream_create.argtypes = [vp, vp, i32, u32, C.c_uint64, C.POINTER(u32)]
    L.gas_stream_destroy.argtypes = [vp, u32]
    L.gas_stream_positions.argtypes = [vp, u32, vp]
    L.gas_stream_get_info.argtypes = [vp, u32, C.POINTER(C.c_uint64), C.POINTER(u32), C.POINTER(i32)]
    L.gas_stream_set_resampled.argtypes = [vp, u32, i32]
    L.gas_stream_set_loop.argtypes = [vp, u32, i32, C.c_uint64, C.c_uint64]
    L.gas_stream_get_loop.argtypes = [vp, u32, C.POINTER(i32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.gas_source_bind_stream.argtypes = [vp, u32, u32, C.c_uint64]
    L.gas_process_block_streams.argtypes = [vp, vp, u32, u32, vp, vp, vp, i32]
    L.gas_process_block_streams_buses.argtypes = [vp, vp, u32, u32, vp, u32, vp, vp, i32]
    L.gas_source_feed_rows.argtypes = [vp, vp, vp, i32, u32, u32, u32, i32]
    L.gas_stream_last_fused.argtypes = [vp]
    L.gas_calc_spatialization.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, u32, vp, i32]
    L.gas_calc_spatialization_areas.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, i32]
    L.gas_calc_early_reflections.argtypes = [vp, vp, u32, vp, vp, vp, vp, u32, vp, i32]
    L.gas_process_block.argtypes = [vp, vp, vp, u32, u32, vp, vp, i32]
    L.gas_bus_routes_publish.argtypes = [vp, vp, vp, u32]
    L.gas_process_block_buses.argtypes = [vp, vp, vp, u32, u32, vp, u32, vp, i32]
    L.gas_ctx_reserve_conv.argtypes = [vp, u32, u32]
    L.gas_conv_ir_load.argtypes = [vp, vp, u32, u32, C.POINTER(u32)]
    L.gas_conv_ir_free.argtypes = [vp, u32]
    L.gas_conv_ir_get_info.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32)]
    L.gas_conv_ir_from_room.argtypes = [vp, vp, u32, u32, vp, C.POINTER(u32)]
    L.gas_conv_ir_from_planes.argtypes = [vp, vp, u32, u32, vp, C.POINTER(u32)]
    L.gas_conv_ir_from_room_hrtf.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, C.POINTER(u32)]
    L.gas_conv_ir_from_room_bands.argtypes = [vp, vp, vp, u32, u32, vp, C.POINTER(u32)]
    L.gas_conv_ir_from_room_hrtf_bands.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, vp, C.POINTER(u32)]
    L.gas_conv_ir_from_room_diffuse.argtypes = [vp, vp, vp, vp, u32, u32, vp, C.POINTER(u32)]
    L.gas_conv_ir_from_room_hrtf_diffuse.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, vp, C.POINTER(u32)]
    L.gas_conv_create.argtypes = [vp, u32, C.POINTER(u32)]
    L.gas_conv_destroy.argtypes = [vp, u32]
    L.gas_conv_reset.argtypes = [vp, u32]
    L.gas_conv_set_ir.argtypes = [vp, u32, u32]
    L.gas_conv_set_levels.argtypes = [vp, u32, C.c_float, C.c_float]
    L.gas_conv_fade_to.argtypes = [vp, u32, u32, C.c_float, C.c_float, u32]
    L.gas_conv_fade_remaining.argtypes = [vp, u32, C.POINTER(u32)]
    L.gas_conv_process.argtypes = [vp, vp, u32, vp, vp, u32, i32]
    L.gas_process_frames_1.argtypes = [vp, u32, vp, vp, i32]
    L.gas_mix_channel_1.argtypes = [vp, u32, i32, vp, vp, i32]
    L.gas_profile_enable.argtypes = [vp, i32]
    L.gas_profile_read.argtypes = [vp, C.POINTER(Profile), i32]
    L.gas_bandwidth_probe.argtypes = [vp, C.c_uint64, C.c_uint64, u32, u32, u32, C.POINTER(C.c_double)]
    L.gas_ctx_read_hrtf_order.argtypes = [vp, vp, u32]
    L.gas_tune_uni12_min.argtypes = [u32]
    L.gas_tune_uni12_min.restype = u32
    L.gas_tune_nt_hist_min.argtypes = [u32]
    L.gas_tune_nt_hist_min.restype = u32
    L.gas_ctx_set_batch_depth.argtypes = [vp, u32]
    _lib = L
    return L


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class SpatializerContext:
    """Thin object wrapper over one gas_ctx (one GPU)."""

    def __init__(self, max_sources, frames=512, channel_count=1, mix_rate=48000.0, er_ring_frames=0, device=0, flags=0):
        self.lib = load_library()
        self.frames = int(frames)
        self.channel_count = int(channel_count)
        self.max_sources = int(max_sources)
        cfg = Config(C.sizeof(Config), device, max_sources, frames, channel_count, mix_rate, er_ring_frames, flags)
        h = C.c_void_p()
        rc = self.lib.gas_ctx_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise GasError(rc, "gas_ctx_create", self.lib.gas_strerror(rc).decode())
        self.h = h

    def _check(self, rc, where):
        if rc != 0:
            detail = self.lib.gas_strerror(rc).decode()
            if rc == -7:
                detail += ": " + self.lib.gas_last_device_error(self.h).decode()
            raise GasError(rc, where, detail)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gas_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- slots ----
    def source_alloc(self, kind, effects=()):
        fx = (C.c_int32 * max(1, len(effects)))(*effects)
        slot = C.c_uint32()
        self._check(self.lib.gas_source_alloc(self.h, kind, fx, len(effects), C.byref(slot)), "gas_source_alloc")
        return slot.value

    def source_alloc_many(self, n, kind, effects=()):
        return np.array([self.source_alloc(kind, effects) for _ in range(n)], dtype=np.uint32)

    def source_free(self, slot):
        self._check(self.lib.gas_source_free(self.h, int(slot)), "gas_source_free")

    def source_set_draining(self, slot, draining=True):
        self._check(self.lib.gas_source_set_draining(self.h, int(slot), int(draining)), "gas_source_set_draining")

    def source_reset(self, slot):
        self._check(self.lib.gas_source_reset(self.h, int(slot)), "gas_source_reset")

    # ---- parameters ----
    def params_publish(self, slot, params):
        p = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        self._check(self.lib.gas_params_publish(self.h, int(slot), _np_ptr(p)), "gas_params_publish")

    @staticmethod
    def fx_settings_defaults(n):
        d = np.zeros(n, FX_SETTINGS_DTYPE)
        d["filter_cutoff_hz"], d["filter_resonance"], d["filter_gain"] = 2000.0, 0.5, 1.0
        return d

    def fx_settings_publish(self, slots, settings):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        f = np.ascontiguousarray(settings, dtype=FX_SETTINGS_DTYPE)
        assert s.shape == f.shape
        self._check(self.lib.gas_fx_settings_publish(self.h, _np_ptr(s), _np_ptr(f), len(s)), "gas_fx_settings_publish")

    @staticmethod
    def fx_dyn_settings_defaults(n):
        return fx_dyn_settings_defaults(n)

    def fx_dyn_settings_publish(self, slots, settings):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        f = np.ascontiguousarray(settings, dtype=FX_DYN_SETTINGS_DTYPE)
        assert s.shape == f.shape
        self._check(self.lib.gas_fx_dyn_settings_publish(self.h, _np_ptr(s), _np_ptr(f), len(s)), "gas_fx_dyn_settings_publish")

    def sidechain_set(self, key, frames):
        """Replace sidechain key block `key` (0 .. MAX_SIDECHAINS - 1) from host memory: frames float32 [F][2], or None for
        a silent key.  Compressors whose compressor_sidechain is key + 1 detect on it from the next callback on.  A block
        of another length than the context's frames raises GAS_ERR_FRAME_COUNT, a key out of range
        GAS_ERR_INVALID_ARGUMENT."""
        if frames is None:
            self._check(self.lib.gas_sidechain_set(self.h, int(key), None, self.frames, MEM_HOST), "gas_sidechain_set")
            return
        f = np.ascontiguousarray(frames, dtype=np.float32)
        assert f.ndim == 2 and f.shape[1] == 2
        self._check(self.lib.gas_sidechain_set(self.h, int(key), _np_ptr(f), f.shape[0], MEM_HOST), "gas_sidechain_set")

    def sidechain_set_raw(self, key, ptr, mem, frames=None):
        """Raw pointer (device or host, 0 / None: a silent key); returns the status.  With MEM_DEVICE the copy is only
        enqueued on the context's stream.  `frames` (default: the context's) is the frame count handed to the library."""
        return self.lib.gas_sidechain_set(self.h, int(key), C.c_void_p(ptr) if ptr else None, self.frames if frames is None else int(frames), mem)

    @staticmethod
    def fx_line_settings_defaults(n):
        return fx_line_settings_defaults(n)

    def fx_line_settings_publish(self, slots, settings):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        f = np.ascontiguousarray(settings, dtype=FX_LINE_SETTINGS_DTYPE)
        assert s.shape == f.shape
        self._check(self.lib.gas_fx_line_settings_publish(self.h, _np_ptr(s), _np_ptr(f), len(s)), "gas_fx_line_settings_publish")

    def reserve_fx_lines(self, delay_lines, reverb_lines):
        """Size the GAS_FX_DELAY / GAS_FX_REVERB line pools (main thread, not during a callback); (0, 0) releases them."""
        self._check(self.lib.gas_ctx_reserve_fx_lines(self.h, int(delay_lines), int(reverb_lines)), "gas_ctx_reserve_fx_lines")

    @staticmethod
    def fx_eq_settings_defaults(n):
        return fx_eq_settings_defaults(n)

    def fx_eq_settings_publish(self, slots, settings):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        f = np.ascontiguousarray(settings, dtype=FX_EQ_SETTINGS_DTYPE)
        assert s.shape == f.shape
        self._check(self.lib.gas_fx_eq_settings_publish(self.h, _np_ptr(s), _np_ptr(f), len(s)), "gas_fx_eq_settings_publish")

    def reserve_fx_eq(self, eq_banks):
        """Size the GAS_FX_EQ6 / _EQ10 / _EQ21 bank pool (main thread, not during a callback); 0 releases it."""
        self._check(self.lib.gas_ctx_reserve_fx_eq(self.h, int(eq_banks)), "gas_ctx_reserve_fx_eq")

    @staticmethod
    def fx_mod_settings_defaults(n):
        return fx_mod_settings_defaults(n)

    def fx_mod_settings_publish(self, slots, settings):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        f = np.ascontiguousarray(settings, dtype=FX_MOD_SETTINGS_DTYPE)
        assert s.shape == f.shape
        self._check(self.lib.gas_fx_mod_settings_publish(self.h, _np_ptr(s), _np_ptr(f), len(s)), "gas_fx_mod_settings_publish")

    def reserve_fx_mod(self, chorus_lines, phaser_banks):
        """Size the GAS_FX_CHORUS line and GAS_FX_PHASER bank pools (main thread, not during a callback); (0, 0) releases them."""
        self._check(self.lib.gas_ctx_reserve_fx_mod(self.h, int(chorus_lines), int(phaser_banks)), "gas_ctx_reserve_fx_mod")

    @staticmethod
    def fx_stereo_settings_defaults(n):
        return fx_stereo_settings_defaults(n)

    def fx_stereo_settings_publish(self, slots, settings):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        f = np.ascontiguousarray(settings, dtype=FX_STEREO_SETTINGS_DTYPE)
        assert s.shape == f.shape
        self._check(self.lib.gas_fx_stereo_settings_publish(self.h, _np_ptr(s), _np_ptr(f), len(s)), "gas_fx_stereo_settings_publish")

    def reserve_fx_stereo(self, enhance_rings):
        """Size the GAS_FX_STEREO_ENHANCE ring pool (main thread, not during a callback); 0 releases it."""
        self._check(self.lib.gas_ctx_reserve_fx_stereo(self.h, int(enhance_rings)), "gas_ctx_reserve_fx_stereo")

    @staticmethod
    def fx_filter_settings_defaults(n):
        return fx_filter_settings_defaults(n)

    def fx_filter_settings_publish(self, slots, settings):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        f = np.ascontiguousarray(settings, dtype=FX_FILTER_SETTINGS_DTYPE)
        assert s.shape == f.shape
        self._check(self.lib.gas_fx_filter_settings_publish(self.h, _np_ptr(s), _np_ptr(f), len(s)), "gas_fx_filter_settings_publish")

    def reserve_fx_filter(self, banks):
        """Size the GAS_FX_FILTER bank pool (main thread, not during a callback); 0 releases it."""
        self._check(self.lib.gas_ctx_reserve_fx_filter(self.h, int(banks)), "gas_ctx_reserve_fx_filter")

    def publish_hrtf_blend(self, slots, blends):
        """FLAG_HRTF_INTERPOLATE: the HRIR rows (HRTF_BLEND_DTYPE) the slots' HRTF stages blend from the next callback on."""
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        b = np.ascontiguousarray(blends, dtype=HRTF_BLEND_DTYPE)
        assert s.shape == b.shape
        self._check(self.lib.gas_hrtf_blend_publish(self.h, _np_ptr(s), _np_ptr(b), len(s)), "gas_hrtf_blend_publish")

    def params_publish_batch(self, slots, params):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        p = np.ascontiguousarray(params, dtype=PARAMS_DTYPE)
        assert s.shape == p.shape
        self._check(self.lib.gas_params_publish_batch(self.h, _np_ptr(s), _np_ptr(p), len(s), MEM_HOST), "gas_params_publish_batch")

    def params_publish_device(self, params_dev_ptr, n, slots=None):
        sp = None
        if slots is not None:
            s = np.ascontiguousarray(slots, dtype=np.uint32)
            sp = _np_ptr(s)
        self._check(self.lib.gas_params_publish_batch(self.h, sp, C.c_void_p(params_dev_ptr), n, MEM_DEVICE), "gas_params_publish_batch")

    def calc_spatialization(self, cfgs, poses, listeners, slots, cfg_index=None, want_params=True):
        """Host-array form of gas_calc_spatialization; returns the generated gas_params rows (or None)."""
        cfgs = np.ascontiguousarray(cfgs, dtype=SPAT3D_CONFIG_DTYPE)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        listeners = np.ascontiguousarray(listeners, dtype=LISTENER_DTYPE)
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        ci = np.ascontiguousarray(cfg_index, dtype=np.uint32) if cfg_index is not None else None
        out = np.zeros(len(slots), PARAMS_DTYPE) if want_params else None
        rc = self.lib.gas_calc_spatialization(self.h, _np_ptr(cfgs), len(cfgs), _np_ptr(ci) if ci is not None else None, _np_ptr(poses), _np_ptr(listeners), len(listeners), _np_ptr(slots), len(slots), _np_ptr(out) if want_params else None, MEM_HOST)
        self._check(rc, "gas_calc_spatialization")
        return out

    def calc_spatialization_areas(self, cfgs, poses, listeners, slots, areas, listener_area_pos, cfg_index=None):
        """Host-array form of gas_calc_spatialization_areas; returns (gas_params rows, reverb volumes [n][4][2])."""
        cfgs = np.ascontiguousarray(cfgs, dtype=SPAT3D_CONFIG_DTYPE)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        listeners = np.ascontiguousarray(listeners, dtype=LISTENER_DTYPE)
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        areas = np.ascontiguousarray(areas, dtype=AREA_SEND_DTYPE)
        lap = np.ascontiguousarray(listener_area_pos, dtype=np.float32) if listener_area_pos is not None else None
        ci = np.ascontiguousarray(cfg_index, dtype=np.uint32) if cfg_index is not None else None
        n = len(slots)
        assert len(areas) == n and (lap is None or lap.shape == (n, len(listeners), 3))
        out = np.zeros(n, PARAMS_DTYPE)
        reverb = np.full((n, 4, 2), np.nan, np.float32)
        rc = self.lib.gas_calc_spatialization_areas(self.h, _np_ptr(cfgs), len(cfgs), _np_ptr(ci) if ci is not None else None, _np_ptr(poses), _np_ptr(listeners), len(listeners), _np_ptr(slots), n, _np_ptr(areas), _np_ptr(lap) if lap is not None else None, _np_ptr(out), _np_ptr(reverb), MEM_HOST)
        self._check(rc, "gas_calc_spatialization_areas")
        return out, reverb

    def calc_early_reflections(self, rooms, poses, listener, slots=None, room_index=None):
        """Host-array form of gas_calc_early_reflections; returns the generated taps (ER_TAPS_DTYPE [n]).  slots=None: the
        pure generator (nothing in the context changes); else the taps also go into the slots' parameter rows."""
        rooms = np.ascontiguousarray(rooms, dtype=ROOM_DTYPE).reshape(-1)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE).reshape(-1)
        listener = np.ascontiguousarray(listener, dtype=LISTENER_DTYPE).reshape(-1)
        assert len(listener) == 1
        n = len(poses)
        sl = np.ascontiguousarray(slots, dtype=np.uint32) if slots is not None else None
        ri = np.ascontiguousarray(room_index, dtype=np.uint32) if room_index is not None else None
        assert (sl is None or len(sl) == n) and (ri is None or len(ri) == n)
        out = np.zeros(n, ER_TAPS_DTYPE)
        rc = self.lib.gas_calc_early_reflections(self.h, _np_ptr(rooms), len(rooms), _np_ptr(ri) if ri is not None else None, _np_ptr(poses), _np_ptr(listener), _np_ptr(sl) if sl is not None else None, n, _np_ptr(out), MEM_HOST)
        self._check(rc, "gas_calc_early_reflections")
        return out

    # ---- device-resident streams ----
    def stream_create(self, pcm, format=None, channels=None, frames=None):
        """pcm: int16 or float32 array [frames] (mono) or [frames][2] (stereo); or, with format, channels and frames, uint8
        data as include/gas_amd.h lays them out: PCM_IMA_ADPCM the codes (((frames + 1) // 2) * channels bytes), PCM_QOA
        the whole QOA file (qoa_file_bytes(frames, channels) bytes).  ValueError only for fewer bytes than the library
        would read; what the bytes hold is the library's to judge (GasError)."""
        a = np.ascontiguousarray(pcm)
        sid = C.c_uint32()
        if format is not None or a.dtype == np.uint8:
            if a.dtype != np.uint8 or format is None or channels is None or frames is None:
                raise ValueError("encoded data are a uint8 array passed with format, channels and frames")
            if int(format) == PCM_QOA:
                if a.size < 4 or (int(channels) in (1, 2) and int(frames) > 0 and bytes(a[:4]) == b"qoaf" and a.size < qoa_file_bytes(int(frames), int(channels))):
                    raise ValueError("fewer bytes than the QOA file of these frames and channels")
            elif int(channels) > 0 and a.size < ((int(frames) + 1) // 2) * int(channels):
                raise ValueError("fewer bytes than ((frames + 1) // 2) * channels")
            self._check(self.lib.gas_stream_create(self.h, _np_ptr(a), int(format), int(channels), int(frames), C.byref(sid)), "gas_stream_create")
            return sid.value
        fmt = PCM_S16 if a.dtype == np.int16 else PCM_F32
        if fmt == PCM_F32:
            a = a.astype(np.float32)
        ch = 1 if a.ndim == 1 else a.shape[1]
        self._check(self.lib.gas_stream_create(self.h, _np_ptr(a), fmt, ch, a.shape[0], C.byref(sid)), "gas_stream_create")
        return sid.value

    def stream_set_resampled(self, sid, on=True):
        self._check(self.lib.gas_stream_set_resampled(self.h, sid, int(on)), "gas_stream_set_resampled")

    def stream_set_loop(self, sid, mode, begin=0, end=0):
        """Loop [begin, end) of the stream (end 0 = its length) for playbacks bound from now on; mode is a LOOP_* constant."""
        self._check(self.lib.gas_stream_set_loop(self.h, int(sid), int(mode), int(begin), int(end)), "gas_stream_set_loop")

    def stream_get_loop(self, sid):
        """(mode, begin, end) as set; (LOOP_DISABLED, 0, 0) for a stream that plays once."""
        mode, b, e = C.c_int32(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.gas_stream_get_loop(self.h, int(sid), C.byref(mode), C.byref(b), C.byref(e)), "gas_stream_get_loop")
        return mode.value, b.value, e.value

    def stream_get_info(self, sid):
        """(frames, channels, format) of a stream; format is a PCM_* constant."""
        n, ch, fmt = C.c_uint64(), C.c_uint32(), C.c_int32()
        self._check(self.lib.gas_stream_get_info(self.h, int(sid), C.byref(n), C.byref(ch), C.byref(fmt)), "gas_stream_get_info")
        return n.value, ch.value, fmt.value

    def stream_destroy(self, sid):
        self._check(self.lib.gas_stream_destroy(self.h, sid), "gas_stream_destroy")

    def source_bind_stream(self, slot, sid, start_frame=0):
        self._check(self.lib.gas_source_bind_stream(self.h, int(slot), int(sid), int(start_frame)), "gas_source_bind_stream")

    def stream_positions(self, n):
        """Stream frame each playback of the last process_block_streams / process_block_streams_buses list (n entries) takes next."""
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._check(self.lib.gas_stream_positions(self.h, n, _np_ptr(out)), "gas_stream_positions")
        return out[:n]

    def process_block_streams(self, slots):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        n = len(s)
        out = np.full((self.channel_count, self.frames, 2), np.nan, dtype=np.float32)
        peaks = np.zeros((max(n, 1), 2), dtype=np.float32)
        hf = np.zeros(max(n, 1), dtype=np.uint8)
        rc = self.lib.gas_process_block_streams(self.h, _np_ptr(s) if n else None, n, self.frames, _np_ptr(out), _np_ptr(peaks), _np_ptr(hf), MEM_HOST)
        self._check(rc, "gas_process_block_streams")
        return out, peaks[:n], hf[:n].astype(bool)

    def process_block_streams_buses(self, slots, n_buses):
        """Stream callback over several buses: -> (mix [n_buses][C][F][2], peaks [n][2], has_frames [n])."""
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        n = len(s)
        out = np.full((max(n_buses, 1), self.channel_count, self.frames, 2), np.nan, dtype=np.float32)
        peaks = np.zeros((max(n, 1), 2), dtype=np.float32)
        hf = np.zeros(max(n, 1), dtype=np.uint8)
        rc = self.lib.gas_process_block_streams_buses(self.h, _np_ptr(s) if n else None, n, self.frames, _np_ptr(out), n_buses, _np_ptr(peaks), _np_ptr(hf), MEM_HOST)
        self._check(rc, "gas_process_block_streams_buses")
        return out[:n_buses], peaks[:n], hf[:n].astype(bool)

    def source_feed_rows(self, slots, rows):
        """Window rows of playbacks that are not bound to a stream, for the next stream callback: rows int16 or float32,
        [n][F] (mono) or [n][F][2] (stereo)."""
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        r = np.ascontiguousarray(rows)
        assert r.dtype in (np.int16, np.float32) and r.ndim in (2, 3) and r.shape[0] == len(s)
        fmt = PCM_S16 if r.dtype == np.int16 else PCM_F32
        ch = 1 if r.ndim == 2 else r.shape[2]
        frames = r.shape[1]
        rc = self.lib.gas_source_feed_rows(self.h, _np_ptr(s) if len(s) else None, _np_ptr(r) if len(s) else None, fmt, ch, len(s), frames, MEM_HOST)
        self._check(rc, "gas_source_feed_rows")

    def stream_last_fused(self):
        """Whether the last stream callback sampled its windows inside the HRTF kernel (else: rows first)."""
        return bool(self.lib.gas_stream_last_fused(self.h))

    def hrtf_load(self, hrir):
        h = np.ascontiguousarray(hrir, dtype=np.float32)
        assert h.ndim == 3 and h.shape[1] == 2
        self._check(self.lib.gas_hrtf_load(self.h, _np_ptr(h), h.shape[0], h.shape[2]), "gas_hrtf_load")

    def hrtf_load_positions(self, positions, hrir, az_steps, el_steps, interpolation=0):
        """positions [m][2] (azimuth, elevation) radians, hrir [m][2][taps]; returns the gridded set [dirs][2][256]."""
        pos = np.ascontiguousarray(positions, dtype=np.float32)
        h = np.ascontiguousarray(hrir, dtype=np.float32)
        assert pos.ndim == 2 and pos.shape[1] == 2 and h.ndim == 3 and h.shape[:2] == (pos.shape[0], 2)
        out = np.zeros((az_steps * el_steps, 2, HRTF_TAPS), np.float32)
        self._check(self.lib.gas_hrtf_load_positions(self.h, _np_ptr(pos), _np_ptr(h), pos.shape[0], h.shape[2], az_steps, el_steps, int(interpolation), _np_ptr(out)), "gas_hrtf_load_positions")
        return out

    # ---- hot path ----
    def process_block(self, src, slots):
        """Host-memory callback: src float32 [n][F][2], slots uint32 [n] -> (mix [C][F][2], peaks [n][2])."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        n = src.shape[0] if src.ndim == 3 else 0
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        assert len(s) == n
        out = np.full((self.channel_count, self.frames, 2), np.nan, dtype=np.float32)
        peaks = np.zeros((max(n, 1), 2), dtype=np.float32)
        frames = src.shape[1] if src.ndim == 3 else self.frames
        rc = self.lib.gas_process_block(self.h, _np_ptr(src) if n else None, _np_ptr(s) if n else None, n, frames, _np_ptr(out), _np_ptr(peaks), MEM_HOST)
        self._check(rc, "gas_process_block")
        return out, peaks[:n]

    def bus_routes_publish(self, slots, routes):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        r = np.ascontiguousarray(routes, dtype=BUS_ROUTE_DTYPE)
        assert s.shape == r.shape
        self._check(self.lib.gas_bus_routes_publish(self.h, _np_ptr(s), _np_ptr(r), len(s)), "gas_bus_routes_publish")

    def process_block_buses(self, src, slots, n_buses):
        """Host-memory callback over several buses: -> (mix [n_buses][C][F][2], peaks [n][2])."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        n = src.shape[0] if src.ndim == 3 else 0
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.full((n_buses, self.channel_count, self.frames, 2), np.nan, dtype=np.float32)
        peaks = np.zeros((max(n, 1), 2), dtype=np.float32)
        rc = self.lib.gas_process_block_buses(self.h, _np_ptr(src) if n else None, _np_ptr(s) if n else None, n, self.frames, _np_ptr(out), n_buses, _np_ptr(peaks), MEM_HOST)
        self._check(rc, "gas_process_block_buses")
        return out, peaks[:n]

    # ---- bus convolvers (gas_conv_*) ----
    def reserve_conv(self, convolvers, max_ir_taps):
        """Size the convolver pool (main thread): `convolvers` instances for IRs of up to max_ir_taps taps; (0, 0) releases."""
        self._check(self.lib.gas_ctx_reserve_conv(self.h, int(convolvers), int(max_ir_taps)), "gas_ctx_reserve_conv")

    def conv_ir_load(self, ir):
        """ir float32 [taps] or [channels][taps], channels 1, 2 or 4 (true stereo: LL, LR, RL, RR) -> IR id."""
        h = np.ascontiguousarray(np.atleast_2d(np.asarray(ir, dtype=np.float32)))
        assert h.ndim == 2
        out = C.c_uint32()
        self._check(self.lib.gas_conv_ir_load(self.h, _np_ptr(h), h.shape[0], h.shape[1], C.byref(out)), "gas_conv_ir_load")
        return out.value

    def conv_ir_free(self, ir):
        self._check(self.lib.gas_conv_ir_free(self.h, int(ir)), "gas_conv_ir_free")

    def conv_ir_get_info(self, ir):
        """-> (channels, taps) as the IR was loaded."""
        ch, taps = C.c_uint32(), C.c_uint32()
        self._check(self.lib.gas_conv_ir_get_info(self.h, int(ir), C.byref(ch), C.byref(taps)), "gas_conv_ir_get_info")
        return ch.value, taps.value

    def _conv_ir_generate(self, fn_name, structs, hrir, n_az, n_el, channels, taps, want_taps, load):
        """The common body of the conv_ir_from_* methods.  structs: (value, dtype) pairs in call order, each narrowed to
        one entry.  hrir None: the library's function takes `channels`; otherwise it takes the HRIR set in their place,
        writes two channels, and `channels` is not read."""
        args = [_np_ptr(np.ascontiguousarray(np.asarray(v, dtype=dt).reshape(-1)[:1])) for v, dt in structs]
        if hrir is None:
            args.append(int(channels))
        else:
            h = np.ascontiguousarray(np.asarray(hrir, dtype=np.float32))
            assert h.ndim == 3 and h.shape[0] == int(n_az) * int(n_el) and h.shape[1] == 2, h.shape
            args += [_np_ptr(h), int(n_az), int(n_el), h.shape[2]]
        taps_out = np.zeros((int(channels) if hrir is None else 2, int(taps)), dtype=np.float32) if want_taps else None
        out = C.c_uint32()
        rc = getattr(self.lib, fn_name)(self.h, *args, int(taps), _np_ptr(taps_out) if want_taps else None, C.byref(out) if load else None)
        self._check(rc, fn_name)
        if load and want_taps:
            return out.value, taps_out
        return out.value if load else taps_out

    def conv_ir_from_room(self, desc, channels, taps, want_taps=False, load=True):
        """An impulse response built on the device from a box room (desc: one ROOM_IR_DTYPE entry).  load: it becomes an
        IR of this context (a reserve is needed); want_taps: the float32 taps [channels][taps] are read back.  Returns
        the IR id, the taps, or (id, taps) when both are asked for; load=False and want_taps=False is refused by the
        library, like every other bad descriptor."""
        return self._conv_ir_generate("gas_conv_ir_from_room", [(desc, ROOM_IR_DTYPE)], None, 0, 0, channels, taps, want_taps, load)

    def conv_ir_from_planes(self, desc, channels, taps, want_taps=False, load=True):
        """conv_ir_from_room for a room bounded by planes (desc: one ROOM_PLANES_DTYPE entry, see default_room_planes and
        planes_from_box): image sources over plane sequences up to desc's max_order.  Returns as conv_ir_from_room does."""
        return self._conv_ir_generate("gas_conv_ir_from_planes", [(desc, ROOM_PLANES_DTYPE)], None, 0, 0, channels, taps, want_taps, load)

    def conv_ir_from_room_hrtf(self, desc, hrir, n_az, n_el, taps, want_taps=False, load=True):
        """conv_ir_from_room heard through an HRIR set: hrir float32 [n_az * n_el][2][hrir_taps] (what hrtf_load was
        given), one direction per image, always two channels (left, right).  Returns as conv_ir_from_room does; the
        taps are [2][taps]."""
        return self._conv_ir_generate("gas_conv_ir_from_room_hrtf", [(desc, ROOM_IR_DTYPE)], hrir, n_az, n_el, None, taps, want_taps, load)

    def conv_ir_from_room_bands(self, desc, bands, channels, taps, want_taps=False, load=True):
        """conv_ir_from_room with per-band wall reflectances and air absorption (bands: one ROOM_BANDS_DTYPE entry, see
        default_room_bands); desc's own room.reflectance is validated but not used.  Returns as conv_ir_from_room does."""
        return self._conv_ir_generate("gas_conv_ir_from_room_bands", [(desc, ROOM_IR_DTYPE), (bands, ROOM_BANDS_DTYPE)], None, 0, 0, channels, taps, want_taps, load)

    def conv_ir_from_room_hrtf_bands(self, desc, bands, hrir, n_az, n_el, taps, want_taps=False, load=True):
        """conv_ir_from_room_hrtf with per-band wall reflectances and air absorption; arguments as conv_ir_from_room_bands
        and conv_ir_from_room_hrtf, the taps are [2][taps]."""
        return self._conv_ir_generate("gas_conv_ir_from_room_hrtf_bands", [(desc, ROOM_IR_DTYPE), (bands, ROOM_BANDS_DTYPE)], hrir, n_az, n_el, None, taps, want_taps, load)

    def conv_ir_from_room_diffuse(self, desc, bands, tail, channels, taps, want_taps=False, load=True):
        """conv_ir_from_room_bands with a diffuse late tail: image sources up to tail's mixing time, then a cross-fade into
        noise that decays per band as the room's mean absorption says (tail: one ROOM_TAIL_DTYPE entry, see
        default_room_tail).  Returns as conv_ir_from_room does."""
        return self._conv_ir_generate("gas_conv_ir_from_room_diffuse", [(desc, ROOM_IR_DTYPE), (bands, ROOM_BANDS_DTYPE), (tail, ROOM_TAIL_DTYPE)], None, 0, 0, channels, taps, want_taps, load)

    def conv_ir_from_room_hrtf_diffuse(self, desc, bands, tail, hrir, n_az, n_el, taps, want_taps=False, load=True):
        """conv_ir_from_room_hrtf_bands with a diffuse late tail; arguments as conv_ir_from_room_diffuse and
        conv_ir_from_room_hrtf, the taps are [2][taps]."""
        return self._conv_ir_generate("gas_conv_ir_from_room_hrtf_diffuse", [(desc, ROOM_IR_DTYPE), (bands, ROOM_BANDS_DTYPE), (tail, ROOM_TAIL_DTYPE)], hrir, n_az, n_el, None, taps, want_taps, load)

    def conv_create(self, ir):
        out = C.c_uint32()
        self._check(self.lib.gas_conv_create(self.h, int(ir), C.byref(out)), "gas_conv_create")
        return out.value

    def conv_destroy(self, conv):
        self._check(self.lib.gas_conv_destroy(self.h, int(conv)), "gas_conv_destroy")

    def conv_reset(self, conv):
        self._check(self.lib.gas_conv_reset(self.h, int(conv)), "gas_conv_reset")

    def conv_set_ir(self, conv, ir):
        self._check(self.lib.gas_conv_set_ir(self.h, int(conv), int(ir)), "gas_conv_set_ir")

    def conv_set_levels(self, conv, dry, wet):
        self._check(self.lib.gas_conv_set_levels(self.h, int(conv), float(dry), float(wet)), "gas_conv_set_levels")

    def conv_fade_to(self, conv, ir, dry, wet, fade_blocks):
        """Fade linearly to (ir, dry, wet) over the instance's next fade_blocks calls; 0 is a hard switch.  During a
        fade the target is kept pending (the latest wins) and starts when the fade in progress has ended."""
        self._check(self.lib.gas_conv_fade_to(self.h, int(conv), int(ir), float(dry), float(wet), int(fade_blocks)), "gas_conv_fade_to")

    def conv_fade_remaining(self, conv):
        """Calls left in the fade in progress plus a pending fade's; 0: settled, the old IR may be freed."""
        out = C.c_uint32(0)
        self._check(self.lib.gas_conv_fade_remaining(self.h, int(conv), C.byref(out)), "gas_conv_fade_remaining")
        return out.value

    def conv_process(self, convs, x, out=None):
        """Instances convs [n] over x [n][F][2].  A host array gives a new host array (the call returns when it is
        complete); a torch device tensor is only enqueued on the context's stream and gives `out` (a device tensor of
        x's shape; default: x itself, in place)."""
        s = np.ascontiguousarray(convs, dtype=np.uint32)
        n = len(s)
        if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
            a = np.ascontiguousarray(x, dtype=np.float32)
            assert a.ndim == 3 and a.shape[0] == n and a.shape[2] == 2
            res = np.full_like(a, np.nan)
            self._check(self.lib.gas_conv_process(self.h, _np_ptr(s), n, _np_ptr(a), _np_ptr(res), a.shape[1], MEM_HOST), "gas_conv_process")
            return res
        out = x if out is None else out
        assert x.is_contiguous() and out.is_contiguous() and tuple(x.shape) == tuple(out.shape) and x.shape[0] == n and x.shape[2] == 2
        self._check(self.lib.gas_conv_process(self.h, _np_ptr(s), n, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.shape[1], MEM_DEVICE), "gas_conv_process")
        return out

    def conv_process_raw(self, convs, n, in_ptr, out_ptr, frames, mem):
        """Raw pointers (device or host); returns the status."""
        sp = None
        if convs is not None:
            s = np.ascontiguousarray(convs, dtype=np.uint32)
            sp = _np_ptr(s)
        return self.lib.gas_conv_process(self.h, sp, int(n), C.c_void_p(in_ptr) if in_ptr else None, C.c_void_p(out_ptr) if out_ptr else None, int(frames), mem)

    def process_block_raw(self, src_ptr, slots, n, frames, out_ptr, peaks_ptr, mem):
        """Raw pointers (device or host). slots: numpy uint32 array or None (reuse the previous list)."""
        sp = None
        if slots is not None:
            s = np.ascontiguousarray(slots, dtype=np.uint32)
            sp = _np_ptr(s)
        return self.lib.gas_process_block(self.h, C.c_void_p(src_ptr), sp, n, frames, C.c_void_p(out_ptr), C.c_void_p(peaks_ptr) if peaks_ptr else None, mem)

    def process_frames_1(self, slot, src):
        src = np.ascontiguousarray(src, dtype=np.float32)
        out = np.full_like(src, np.nan)
        self._check(self.lib.gas_process_frames_1(self.h, int(slot), _np_ptr(out), _np_ptr(src), src.shape[0]), "gas_process_frames_1")
        return out

    def mix_channel_1(self, slot, channel, src):
        src = np.ascontiguousarray(src, dtype=np.float32)
        out = np.full_like(src, np.nan)
        self._check(self.lib.gas_mix_channel_1(self.h, int(slot), int(channel), _np_ptr(out), _np_ptr(src), src.shape[0]), "gas_mix_channel_1")
        return out

    def set_stream(self, hip_stream):
        self._check(self.lib.gas_ctx_set_stream(self.h, C.c_void_p(hip_stream)), "gas_ctx_set_stream")

    def synchronize(self):
        self._check(self.lib.gas_ctx_synchronize(self.h), "gas_ctx_synchronize")

    def join_outputs(self):
        """FLAG_PIPELINED_MIX: order the context's stream behind every `out` written so far (non-blocking)."""
        self._check(self.lib.gas_ctx_join_outputs(self.h), "gas_ctx_join_outputs")

    def profile_enable(self, on=1):
        self._check(self.lib.gas_profile_enable(self.h, int(on)), "gas_profile_enable")

    def bandwidth_probe(self, read_bytes, write_bytes, workgroups=2048, unroll=4, iters=50):
        """Span (us) of one pure streaming launch over the given byte counts, timed like the dominant kernel."""
        us = C.c_double()
        self._check(self.lib.gas_bandwidth_probe(self.h, int(read_bytes), int(write_bytes), int(workgroups), int(unroll), int(iters), C.byref(us)), "gas_bandwidth_probe")
        return us.value

    def set_batch_depth(self, depth):
        """FLAG_BATCHED_LAUNCH: callbacks per k_hrtf_multi launch (1 .. 16)."""
        self._check(self.lib.gas_ctx_set_batch_depth(self.h, int(depth)), "gas_ctx_set_batch_depth")

    def read_hrtf_order(self, n):
        """Diagnostic: the XCD-affine processing order of the last callback's plain [HRTF] sources."""
        out = np.zeros(int(n), np.uint32)
        self._check(self.lib.gas_ctx_read_hrtf_order(self.h, out.ctypes.data, int(n)), "gas_ctx_read_hrtf_order")
        return out

    def profile_read(self, reset=True):
        p = Profile()
        self._check(self.lib.gas_profile_read(self.h, C.byref(p), int(reset)), "gas_profile_read")
        return {"launches": p.launches, "kernel_ms": p.kernel_ms, "bytes_per_launch": p.bytes_per_launch, "kernel": p.kernel_name.decode(), "callbacks_per_launch": p.callbacks_per_launch, "bytes_per_callback_formula": p.bytes_per_callback_formula}


class BatchedSpatializerHost:
    """ctypes view of include/gas_amd_host.h: the CPU-side half of AudioSpatializerInstance
    (source window, fade-out, latch, silence gate, list GC) over one gas_process_block per callback."""

    def __init__(self, ctx, kind, effects=()):
        self.ctx = ctx
        L = self.lib = ctx.lib
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
        L.gas_host_create.argtypes = [vp, i32, C.POINTER(C.c_int32), u32, C.POINTER(vp)]
        L.gas_host_destroy.argtypes = [vp]
        L.gas_host_destroy.restype = None
        L.gas_host_start_playback_array.argtypes = [vp, vp, C.c_int64, C.POINTER(u32)]
        L.gas_host_stop_playback.argtypes = [vp, u32]
        L.gas_host_start_playback_device_stream.argtypes = [vp, u32, C.c_uint64, C.POINTER(u32)]
        L.gas_host_set_spatializer_parameters.argtypes = [vp, u32, vp]
        L.gas_host_set_playback_disable_threshold_db.argtypes = [vp, C.c_float]
        L.gas_host_set_playback_disable_threshold_db.restype = None
        L.gas_host_is_playback_active.argtypes = [vp, u32]
        L.gas_host_playback_count.argtypes = [vp]
        L.gas_host_set_playback_paused.argtypes = [vp, u32, i32]
        L.gas_host_is_playback_paused.argtypes = [vp, u32]
        L.gas_host_get_playback_position.argtypes = [vp, u32, C.POINTER(C.c_uint64)]
        L.gas_host_get_mixed_frames.argtypes = [vp, i32, vp, i32]
        L.gas_host_set_effect_settings.argtypes = [vp, u32, vp]
        L.gas_host_set_effect_settings_dyn.argtypes = [vp, u32, vp]
        L.gas_host_set_effect_settings_line.argtypes = [vp, u32, vp]
        L.gas_host_set_sidechain.argtypes = [vp, u32, vp, i32]
        L.gas_host_set_effect_settings_eq.argtypes = [vp, u32, vp]
        L.gas_host_set_effect_settings_mod.argtypes = [vp, u32, vp]
        L.gas_host_set_effect_settings_stereo.argtypes = [vp, u32, vp]
        L.gas_host_set_effect_settings_filter.argtypes = [vp, u32, vp]
        L.gas_host_set_hrtf_blend.argtypes = [vp, u32, vp]
        L.gas_host_set_release_fn.argtypes = [vp, vp, vp]
        L.gas_host_collect_released.argtypes = [vp]
        L.gas_host_set_process_effects_fn.argtypes = [vp, vp, vp]
        L.gas_host_start_playback.argtypes = [vp, vp, vp, C.POINTER(u32)]
        L.gas_host_set_mixed.argtypes = [vp, i32]
        self._callbacks = []  # ctypes trampolines must outlive their registration
        fx = (C.c_int32 * max(1, len(effects)))(*effects)
        h = C.c_void_p()
        ctx._check(L.gas_host_create(ctx.h, kind, fx, len(effects), C.byref(h)), "gas_host_create")
        self.h = h
        self._streams = []

    def close(self):
        if self.h:
            self.lib.gas_host_destroy(self.h)
            self.h = None

    def set_mixed(self, on=True):
        """Opt in to array / callback playbacks next to device-stream playbacks (before the first playback starts)."""
        return self.lib.gas_host_set_mixed(self.h, int(on))

    def start_playback_array(self, stream):
        s = np.ascontiguousarray(stream, dtype=np.float32)
        self._streams.append(s)  # the host reads it on every callback: keep it alive
        pid = C.c_uint32()
        self.ctx._check(self.lib.gas_host_start_playback_array(self.h, _np_ptr(s), s.shape[0], C.byref(pid)), "gas_host_start_playback_array")
        return pid.value

    def start_playback_device_stream(self, stream_id, start_frame=0):
        pid = C.c_uint32()
        self.ctx._check(self.lib.gas_host_start_playback_device_stream(self.h, int(stream_id), int(start_frame), C.byref(pid)), "gas_host_start_playback_device_stream")
        return pid.value

    STREAM_MIX_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int)
    RELEASE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_void_p)
    PROCESS_EFFECTS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p)

    def start_playback(self, mix, user=0):
        """mix(buffer: float32 [frames, 2] view, rate_scale, frames) -> frames mixed: the engine's
        AudioStreamPlayback::mix as a Python callable (tests only; it runs on whichever thread mixes)."""

        def tramp(u, buf, rate, frames):
            view = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_float)), shape=(frames, 2))
            return int(mix(view, rate, frames))

        cb = self.STREAM_MIX_FN(tramp)
        self._callbacks.append(cb)
        pid = C.c_uint32()
        self.ctx._check(self.lib.gas_host_start_playback(self.h, C.cast(cb, C.c_void_p), C.c_void_p(user), C.byref(pid)), "gas_host_start_playback")
        return pid.value

    def set_release_fn(self, fn):
        """fn(id, user) for every playback the host has finished with (control thread)."""
        cb = self.RELEASE_FN(lambda _u, pid, user: fn(pid, user or 0)) if fn else None
        self._callbacks.append(cb)
        return self.lib.gas_host_set_release_fn(self.h, C.cast(cb, C.c_void_p) if cb else None, None)

    def collect_released(self):
        return self.lib.gas_host_collect_released(self.h)

    def set_process_effects_fn(self, fn):
        """fn(id, params: one-element PARAMS_DTYPE view) -> truthy when it edited the row (audio thread)."""

        def tramp(_u, pid, p):
            row = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(PARAMS_DTYPE.itemsize,)).view(PARAMS_DTYPE)
            return int(bool(fn(pid, row)))

        cb = self.PROCESS_EFFECTS_FN(tramp) if fn else None
        self._callbacks.append(cb)
        return self.lib.gas_host_set_process_effects_fn(self.h, C.cast(cb, C.c_void_p) if cb else None, None)

    def stop_playback(self, pid):
        return self.lib.gas_host_stop_playback(self.h, pid)

    def set_spatializer_parameters(self, pid, params):
        """Returns GAS_OK, or GAS_ERR_BAD_SLOT when the playback has ended and been reaped meanwhile (not an error for a
        control thread: the reference's update_spatializer_parameters has nothing to address then either)."""
        p = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        rc = self.lib.gas_host_set_spatializer_parameters(self.h, pid, _np_ptr(p))
        if rc != -3:
            self.ctx._check(rc, "gas_host_set_spatializer_parameters")
        return rc

    def set_effect_settings(self, pid, settings):
        f = np.ascontiguousarray(settings, dtype=FX_SETTINGS_DTYPE).reshape(1)
        return self.lib.gas_host_set_effect_settings(self.h, pid, _np_ptr(f))

    def set_effect_dyn_settings(self, pid, settings):
        f = np.ascontiguousarray(settings, dtype=FX_DYN_SETTINGS_DTYPE).reshape(1)
        return self.lib.gas_host_set_effect_settings_dyn(self.h, pid, _np_ptr(f))

    def set_sidechain(self, key, frames):
        """Audio thread, before get_mixed_frames: key block `key` of the host's context from float32 [F][2], or None."""
        if frames is None:
            return self.lib.gas_host_set_sidechain(self.h, int(key), None, self.ctx.frames)
        f = np.ascontiguousarray(frames, dtype=np.float32)
        return self.lib.gas_host_set_sidechain(self.h, int(key), _np_ptr(f), f.shape[0])

    def set_effect_line_settings(self, pid, settings):
        f = np.ascontiguousarray(settings, dtype=FX_LINE_SETTINGS_DTYPE).reshape(1)
        return self.lib.gas_host_set_effect_settings_line(self.h, pid, _np_ptr(f))

    def set_effect_settings_eq(self, pid, settings):
        f = np.ascontiguousarray(settings, dtype=FX_EQ_SETTINGS_DTYPE).reshape(1)
        return self.lib.gas_host_set_effect_settings_eq(self.h, pid, _np_ptr(f))

    def set_effect_settings_mod(self, pid, settings):
        f = np.ascontiguousarray(settings, dtype=FX_MOD_SETTINGS_DTYPE).reshape(1)
        return self.lib.gas_host_set_effect_settings_mod(self.h, pid, _np_ptr(f))

    def set_effect_settings_stereo(self, pid, settings):
        f = np.ascontiguousarray(settings, dtype=FX_STEREO_SETTINGS_DTYPE).reshape(1)
        return self.lib.gas_host_set_effect_settings_stereo(self.h, pid, _np_ptr(f))

    def set_effect_settings_filter(self, pid, settings):
        f = np.ascontiguousarray(settings, dtype=FX_FILTER_SETTINGS_DTYPE).reshape(1)
        return self.lib.gas_host_set_effect_settings_filter(self.h, pid, _np_ptr(f))

    def set_hrtf_blend(self, pid, blend):
        b = np.ascontiguousarray(blend, dtype=HRTF_BLEND_DTYPE).reshape(1)
        return self.lib.gas_host_set_hrtf_blend(self.h, pid, _np_ptr(b))

    def is_playback_active(self, pid):
        return bool(self.lib.gas_host_is_playback_active(self.h, pid))

    def playback_count(self):
        return self.lib.gas_host_playback_count(self.h)

    def set_playback_paused(self, pid, paused=True):
        return self.lib.gas_host_set_playback_paused(self.h, pid, int(paused))

    def is_playback_paused(self, pid):
        return bool(self.lib.gas_host_is_playback_paused(self.h, pid))

    def get_playback_position(self, pid):
        """Frames of the stream consumed so far (0 for an unknown id)."""
        f = C.c_uint64()
        self.lib.gas_host_get_playback_position(self.h, pid, C.byref(f))
        return f.value

    def get_mixed_frames(self, channel, frame_count):
        out = np.full((frame_count, 2), np.nan, dtype=np.float32)
        rc = self.lib.gas_host_get_mixed_frames(self.h, channel, _np_ptr(out), frame_count)
        return rc, out


class MultiContext:
    """ctypes view of gas_multi_* (include/gas_amd_host.h): several per-device contexts in one process."""

    def __init__(self, devices, max_sources, frames=512, channel_count=1, mix_rate=48000.0, er_ring_frames=0, flags=0):
        L = self.lib = load_library()
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
        L.gas_multi_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_int32), u32, C.POINTER(vp)]
        L.gas_multi_destroy.argtypes = [vp]
        L.gas_multi_destroy.restype = None
        L.gas_multi_shards.argtypes = [vp]
        L.gas_multi_shards.restype = u32
        L.gas_multi_shard.argtypes = [vp, u32]
        L.gas_multi_shard.restype = vp
        L.gas_multi_least_loaded.argtypes = [vp]
        L.gas_multi_least_loaded.restype = u32
        L.gas_multi_note_alloc.argtypes = [vp, u32, i32]
        L.gas_multi_note_alloc.restype = None
        L.gas_multi_process_block.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u32), u32, vp, C.POINTER(vp)]
        L.gas_multi_process_block_mem.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u32), u32, vp, C.POINTER(vp), i32]
        L.gas_multi_synchronize.argtypes = [vp]
        L.gas_multi_root_stream.argtypes = [vp]
        L.gas_multi_root_stream.restype = vp
        self.frames, self.channel_count = frames, channel_count
        cfg = Config(C.sizeof(Config), 0, max_sources, frames, channel_count, mix_rate, er_ring_frames, flags)
        dev = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        rc = L.gas_multi_create(C.byref(cfg), dev, len(devices), C.byref(h))
        if rc != 0:
            raise GasError(rc, "gas_multi_create", L.gas_strerror(rc).decode())
        self.h = h
        self.shards = []
        for g in range(len(devices)):
            ctx = SpatializerContext.__new__(SpatializerContext)  # a view: the multi-context owns the handle
            ctx.lib, ctx.frames, ctx.channel_count, ctx.max_sources = L, frames, channel_count, max_sources
            ctx.h = C.c_void_p(L.gas_multi_shard(h, g))
            ctx.close = lambda: None
            self.shards.append(ctx)

    def close(self):
        if self.h:
            for s in self.shards:
                s.h = None
            self.lib.gas_multi_destroy(self.h)
            self.h = None

    def process_block_device(self, src_ptrs, slots_per_shard, out_ptr, peaks_ptrs=None):
        """Device-memory callback: src_ptrs[g] / peaks_ptrs[g] are device addresses on shard g's device, out_ptr on the
        root device; only enqueues (gas_multi_synchronize / the root stream order the result)."""
        G = len(self.shards)
        sls = [np.ascontiguousarray(s, dtype=np.uint32) for s in slots_per_shard]
        vp = C.c_void_p
        a_src = (vp * G)(*src_ptrs)
        a_sl = (vp * G)(*[s.ctypes.data for s in sls])
        a_pk = (vp * G)(*(peaks_ptrs if peaks_ptrs is not None else [None] * G))
        a_n = (C.c_uint32 * G)(*[len(s) for s in sls])
        rc = self.lib.gas_multi_process_block_mem(self.h, a_src, a_sl, a_n, self.frames, C.c_void_p(out_ptr), a_pk, MEM_DEVICE)
        if rc != 0:
            raise GasError(rc, "gas_multi_process_block_mem", self.lib.gas_strerror(rc).decode())

    def synchronize(self):
        rc = self.lib.gas_multi_synchronize(self.h)
        if rc != 0:
            raise GasError(rc, "gas_multi_synchronize", self.lib.gas_strerror(rc).decode())

    def process_block(self, src_per_shard, slots_per_shard):
        G = len(self.shards)
        srcs = [np.ascontiguousarray(s, dtype=np.float32) for s in src_per_shard]
        sls = [np.ascontiguousarray(s, dtype=np.uint32) for s in slots_per_shard]
        pks = [np.zeros((max(len(s), 1), 2), np.float32) for s in sls]
        vp = C.c_void_p
        a_src = (vp * G)(*[s.ctypes.data for s in srcs])
        a_sl = (vp * G)(*[s.ctypes.data for s in sls])
        a_pk = (vp * G)(*[p.ctypes.data for p in pks])
        a_n = (C.c_uint32 * G)(*[len(s) for s in sls])
        out = np.full((self.channel_count, self.frames, 2), np.nan, np.float32)
        rc = self.lib.gas_multi_process_block(self.h, a_src, a_sl, a_n, self.frames, _np_ptr(out), a_pk)
        if rc != 0:
            raise GasError(rc, "gas_multi_process_block", self.lib.gas_strerror(rc).decode())
        return out, [p[: len(s)] for p, s in zip(pks, sls)]
