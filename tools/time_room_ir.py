"""Dev aid: gas_conv_ir_from_room and gas_conv_ir_from_room_hrtf, one shape per run.

  python tools/time_room_ir.py default      the room of capi.default_rooms, 48 000 taps, two channels
  python tools/time_room_ir.py long         the same room, 2^20 taps, two channels, max_order 256 (513^3 cells < 2^28)
  python tools/time_room_ir.py test         the largest shape of tests/test_gpu_room_ir.py (16 384 taps)
  python tools/time_room_ir.py --hrtf SHAPE the same shape through gas_conv_ir_from_room_hrtf, with synth.synthetic_hrir's
                                            1024 directions of 256 taps as a 64 x 16 grid
  python tools/time_room_ir.py --bands B --filter-taps L [--hrtf] SHAPE
                                            the same shape through gas_conv_ir_from_room_bands (or _hrtf_bands): B bands
                                            split at 500 Hz and 4 kHz (B = 3) or at B - 1 points from 125 Hz to 8 kHz,
                                            walls that absorb more per band, air on all bands but the lowest
  python tools/time_room_ir.py --diffuse MIX_MS FADE_MS [--bands B --filter-taps L] [--hrtf] SHAPE
                                            the same shape through gas_conv_ir_from_room_diffuse (or _hrtf_diffuse):
                                            image sources for MIX_MS after the direct sound, FADE_MS of cross-fade, the
                                            diffuse tail behind them; without --bands one broadband band

  python tools/time_room_ir.py --planes     gas_conv_ir_from_planes for four rooms, 8192 taps, two channels: a box as six
                                            planes at max_order 4 and 8 next to gas_conv_ir_from_room of the same box and
                                            orders, an attic of 7 planes at order 6, a room of 12 planes at order 5; one
                                            JSON line per room with the times as below, the reference's candidate, void
                                            and valid counts, the share of sequences a lane may leave early, and parity

Prints one JSON line: the wall clock of a whole loading call (tables, allocations, launches, transform, synchronise) as
the median of STEPS calls, the span of the generator's launches from the library's HIP-event bracket
(gas_profile_enable; zeroing, k_room_ir or k_room_ir_hrtf and the scaling kernel, not the transform), the numpy
reference's time on the same inputs, and the parity of the read-back taps against it (relative RMS and max-abs over
max|h|, worst channel).  With --hrtf also the 8-byte adds the reference counts (non-zero products that land on a tap),
their bytes and the rate over the generator's span, and near_edge: the images whose cell two atan2 may choose
differently (tests/room_brir_ref.py); the long shape's reference takes minutes and is skipped unless --reference is
given.  With --bands the reference is tests/room_bands_ref.py (B passes of the one above plus the float64 combine), and
the line also holds the float64 multiply-adds of the combine, channels taps B L, and the plain call timed in the same
process, so that "B lattice passes plus the combine" can be read off one line.  With --diffuse the reference is
tests/room_tail_ref.py, the line holds the marks K0 and K1 and the cells of the lattice for K1 taps, and the *_bands call
of the same shape is timed in the same process (bands_call_ms, bands_generator_launches_ms), so that what the tail saves
can be read off one line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402
import room_bands_ref as BD  # noqa: E402
import room_brir_ref as BR  # noqa: E402
import room_ir_ref as R  # noqa: E402
import room_planes_ref as PL  # noqa: E402
import room_tail_ref as T  # noqa: E402

K = gas.capi
WARMUP, STEPS = 2, 7
N_AZ, N_EL = 64, 16
SHAPES = {
    "default": (dict(), 2, 48000),
    "long": (dict(max_order=256), 2, 1 << 20),
    "test": (dict(room=K.default_rooms(half_extent=(2.5, 2.0, 1.5), reflectance=(0.9, 0.85, 0.8, 0.75, 0.7, 0.95)), source=(1.0, 0.5, 0.25), listener_origin=(-1.0, 0.25, -0.5)), 2, 16384),
}


def parity(h, ref_h):
    ch = range(h.shape[0])
    rms = max(float(np.sqrt(np.mean((h[e].astype(np.float64) - ref_h[e]) ** 2)) / np.sqrt(np.mean(ref_h[e].astype(np.float64) ** 2))) for e in ch)
    mx = max(float(np.abs(h[e].astype(np.float64) - ref_h[e]).max() / np.abs(ref_h[e]).max()) for e in ch)
    return {"rel_rms": rms, "max_abs_over_max": mx, "bitwise": bool(np.array_equal(h, ref_h))}


def count_adds(ref, hrir, taps):
    """The adds k_room_ir_hrtf issues: per image, ear and j a non-zero quantised product whose tap is in range."""
    v, pos = ref.mono.v[0], ref.mono.pos[0]
    k = np.floor(pos)
    f = pos - k
    k = k.astype(np.int64)
    a0, a1 = v * (1.0 - f), v * f
    T = hrir.shape[2]
    H = np.zeros((hrir.shape[0], 2, T + 2))
    H[:, :, 1 : T + 1] = hrir
    adds = 0
    for e in range(2):
        He = H[ref.dirs, e]
        for j in range(T + 1):
            t = k + j
            q = np.rint((a0 * He[:, j + 1] + a1 * He[:, j]) * BR.ONE)
            adds += int(np.count_nonzero((t >= 0) & (t < taps) & (q != 0)))
    return adds


def make_bands(d, n_bands, filter_taps):
    """B bands over the descriptor's own walls: band b reflects 1 - 0.05 b of what they do and loses 0.01 b dB a metre."""
    xo = {1: (), 2: (1000.0,), 3: (500.0, 4000.0)}.get(n_bands) or tuple(float(v) for v in np.geomspace(125.0, 8000.0, n_bands - 1))
    walls = d["room"]["reflectance"][0].astype(np.float64)
    return K.default_room_bands(xo, [walls * (1.0 - 0.05 * b) for b in range(n_bands)], [0.01 * b for b in range(n_bands)], filter_taps)


def timed_calls(ctx, call):
    """-> (call_ms dict, generator's launches ms, bracketed calls): WARMUP + STEPS loading calls, the last STEPS profiled."""
    ts = []
    for i in range(WARMUP + STEPS):
        if i == WARMUP:
            ctx.profile_enable(1)
        t0 = time.perf_counter()
        ir = call()
        t1 = time.perf_counter()
        ctx.conv_ir_free(ir)
        if i >= WARMUP:
            ts.append((t1 - t0) * 1e3)
    p = ctx.profile_read()
    ctx.profile_enable(0)
    return {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}, round(p["kernel_ms"] / max(p["launches"], 1), 3), p["launches"]


def twelve_planes():
    """A floor, a ceiling at 3.2 m and ten walls at uneven angles and distances of 3.5 to 4.5 m."""
    rng = np.random.default_rng(1)
    rows = [((0, 1, 0), 0.0, 0.8), ((0, -1, 0), -3.2, 0.8)]
    for i in range(10):
        th = 2 * np.pi * (i + rng.uniform(-0.2, 0.2)) / 10
        rows.append(((-np.cos(th), 0.0, -np.sin(th)), -rng.uniform(3.5, 4.5), 0.7 + 0.02 * i))
    return rows


def planes_main():
    channels, taps = 2, 8192
    box = K.default_rooms(half_extent=(2.5, 2.0, 1.5), reflectance=(0.9, 0.85, 0.8, 0.75, 0.7, 0.95))
    src, lis = (1.0, 0.5, 0.25), (-1.0, 0.25, -0.5)
    attic_src, attic_lis = (1.1, 1.2, 0.5), (-0.9, 1.45, -0.8)
    rooms = [
        ("box as 6 planes, max_order 4", K.default_room_planes(K.planes_from_box(box), src, lis, max_order=4), K.default_room_ir(box, src, lis, max_order=4)),
        ("box as 6 planes, max_order 8", K.default_room_planes(K.planes_from_box(box), src, lis, max_order=8), K.default_room_ir(box, src, lis, max_order=8)),
        ("attic of 7 planes, max_order 6", K.default_room_planes(None, attic_src, attic_lis, max_order=6), None),
        ("12 planes, max_order 5", PL.describe(twelve_planes(), attic_src, attic_lis, ear_spacing=0.18, max_order=5), None),
    ]
    ctx = gas.SpatializerContext(max_sources=4, frames=512)
    ctx.reserve_conv(1, taps)
    for name, d, box_desc in rooms:
        out = {"room": name, "channels": channels, "taps": taps}
        out["call_ms"], out["generator_launches_ms"], out["bracketed_calls"] = timed_calls(ctx, lambda: ctx.conv_ir_from_planes(d, channels, taps))
        h = ctx.conv_ir_from_planes(d, channels, taps, want_taps=True, load=False)
        if box_desc is not None:
            out["box_call_ms"], out["box_generator_launches_ms"], _ = timed_calls(ctx, lambda: ctx.conv_ir_from_room(box_desc, channels, taps))
            out["parity_with_the_box_call"] = parity(h, ctx.conv_ir_from_room(box_desc, channels, taps, want_taps=True, load=False))
        t0 = time.perf_counter()
        ref = PL.ir(d, channels, taps, 48000.0)
        out["numpy_reference_s"] = round(time.perf_counter() - t0, 3)
        out["candidates"], out["void"], out["valid"] = ref.candidates, ref.void, ref.valid
        out["left_early"], out["left_early_share"] = ref.left_early, round(ref.left_early / max(ref.candidates, 1), 4)
        out["margin_m"], out["smallest_v"] = ref.margin, ref.v_min
        out["parity"] = parity(h, ref.h)
        print(json.dumps(out), flush=True)
    ctx.close()


def main(shape, hrtf, want_reference, n_bands=0, filter_taps=0, diffuse=None):
    kw, channels, taps = SHAPES[shape]
    d = K.default_room_ir(**kw)
    if diffuse and not n_bands:
        n_bands = 1
    bands = make_bands(d, n_bands, filter_taps) if n_bands else None
    tail = K.default_room_tail(seed=1, mix_time_s=diffuse[0] * 1e-3, fade_s=diffuse[1] * 1e-3) if diffuse else None
    hrir = synth.synthetic_hrir(np.random.default_rng(0), dirs=N_AZ * N_EL) if hrtf else None
    ctx = gas.SpatializerContext(max_sources=4, frames=512)
    ctx.reserve_conv(1, taps)

    def plain_call(**how):
        if hrtf:
            return ctx.conv_ir_from_room_hrtf(d, hrir, N_AZ, N_EL, taps, **how)
        return ctx.conv_ir_from_room(d, channels, taps, **how)

    def bands_call(**how):
        if hrtf:
            return ctx.conv_ir_from_room_hrtf_bands(d, bands, hrir, N_AZ, N_EL, taps, **how)
        return ctx.conv_ir_from_room_bands(d, bands, channels, taps, **how)

    def call(**how):
        if bands is None:
            return plain_call(**how)
        if tail is None:
            return bands_call(**how)
        if hrtf:
            return ctx.conv_ir_from_room_hrtf_diffuse(d, bands, tail, hrir, N_AZ, N_EL, taps, **how)
        return ctx.conv_ir_from_room_diffuse(d, bands, tail, channels, taps, **how)

    n, cells = R.box(d, 1 if hrtf else channels, taps, 48000.0)
    out = {"shape": shape, "hrtf": hrtf, "channels": channels, "taps": taps, "N": n, "cells": cells}
    if bands is not None:
        L = 1 if n_bands == 1 else filter_taps
        out["bands"], out["filter_taps"], out["combine_fma"] = n_bands, L, (2 if hrtf else channels) * taps * n_bands * L
        out["plain_call_ms"], out["plain_generator_launches_ms"], _ = timed_calls(ctx, plain_call)
    if tail is not None:
        k0, k1 = T.marks(tail, taps, 48000.0)
        out["diffuse"] = {"mix_ms": diffuse[0], "fade_ms": diffuse[1], "K0": k0, "K1": k1, "cells_for_K1": R.box(d, 1 if hrtf else channels, k1, 48000.0)[1] if k1 else 0}
        out["bands_call_ms"], out["bands_generator_launches_ms"], _ = timed_calls(ctx, bands_call)
    out["call_ms"], out["generator_launches_ms"], out["bracketed_calls"] = timed_calls(ctx, call)
    if bands is not None and tail is None:
        out["generator_minus_B_plain_ms"] = round(out["generator_launches_ms"] - n_bands * out["plain_generator_launches_ms"], 3)
    t0 = time.perf_counter()
    h = call(want_taps=True, load=False)
    out["pure_generator_with_read_back_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    ctx.close()
    if hrtf and shape == "long" and not want_reference:
        out["reference"] = "skipped"
        print(json.dumps(out))
        return
    if shape == "long" and bands is not None and not want_reference:
        out["reference"] = "skipped"
        print(json.dumps(out))
        return
    t0 = time.perf_counter()
    if tail is not None:
        ref = T.brir(d, bands, tail, hrir, N_AZ, N_EL, taps, 48000.0) if hrtf else T.ir(d, bands, tail, channels, taps, 48000.0)
        out["numpy_reference_s"] = round(time.perf_counter() - t0, 3)
        out["parity"] = parity(h, ref.h)
        print(json.dumps(out))
        return
    if bands is not None:
        ref = BD.brir(d, bands, hrir, N_AZ, N_EL, taps, 48000.0) if hrtf else BD.ir(d, bands, channels, taps, 48000.0)
        out["numpy_reference_s"] = round(time.perf_counter() - t0, 3)
        out["parity"] = parity(h, ref.h)
        print(json.dumps(out))
        return
    if hrtf:
        ref = BR.brir(d, hrir, N_AZ, N_EL, taps, 48000.0)
        mono = ref.mono
    else:
        ref = mono = R.ir(d, channels, taps, 48000.0)
    out["numpy_reference_s"] = round(time.perf_counter() - t0, 3)
    out["candidates"], out["in_range_ch0"] = mono.candidates, mono.in_range
    if hrtf:
        adds = count_adds(ref, hrir, taps)
        out["near_edge"] = ref.near_edge
        out["adds"], out["added_bytes"] = adds, 8 * adds
        out["added_TB_per_s_over_generator_span"] = round(8 * adds / (out["generator_launches_ms"] * 1e-3) / 1e12, 3)
    out["parity"] = parity(h, ref.h)
    print(json.dumps(out))


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--planes" in argv:
        planes_main()
        sys.exit(0)
    valued = {}
    for flag in ("--bands", "--filter-taps"):
        if flag in argv:
            i = argv.index(flag)
            valued[flag] = int(argv[i + 1])
            del argv[i : i + 2]
    diffuse = None
    if "--diffuse" in argv:
        i = argv.index("--diffuse")
        diffuse = (float(argv[i + 1]), float(argv[i + 2]))
        del argv[i : i + 3]
    args = [a for a in argv if not a.startswith("--")]
    main(args[0] if args else "default", "--hrtf" in argv, "--reference" in argv, valued.get("--bands", 0), valued.get("--filter-taps", 255), diffuse)
