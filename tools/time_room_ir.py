"""Dev aid: gas_conv_ir_from_room, one shape per run.

  python tools/time_room_ir.py default      the room of capi.default_rooms, 48 000 taps, two channels
  python tools/time_room_ir.py long         the same room, 2^20 taps, two channels, max_order 256 (513^3 cells < 2^28)
  python tools/time_room_ir.py test         the largest shape of tests/test_gpu_room_ir.py (16 384 taps)

Prints one JSON line: the wall clock of a whole loading call (tables, allocations, launches, transform, synchronise) as
the median of STEPS calls, the span of the generator's launches from the library's HIP-event bracket
(gas_profile_enable; zeroing, k_room_ir and the scaling kernel, not the transform), the numpy reference's time on the
same inputs, and the parity of the read-back taps against it (relative RMS and max-abs over max|h|, worst channel)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import godot_audio_spatializer_amd as gas  # noqa: E402
import room_ir_ref as R  # noqa: E402

K = gas.capi
WARMUP, STEPS = 2, 7
SHAPES = {
    "default": (dict(), 2, 48000),
    "long": (dict(max_order=256), 2, 1 << 20),
    "test": (dict(room=K.default_rooms(half_extent=(2.5, 2.0, 1.5), reflectance=(0.9, 0.85, 0.8, 0.75, 0.7, 0.95)), source=(1.0, 0.5, 0.25), listener_origin=(-1.0, 0.25, -0.5)), 2, 16384),
}


def main(shape):
    kw, channels, taps = SHAPES[shape]
    d = K.default_room_ir(**kw)
    ctx = gas.SpatializerContext(max_sources=4, frames=512)
    ctx.reserve_conv(1, taps)
    n, cells = R.box(d, channels, taps, 48000.0)
    out = {"shape": shape, "channels": channels, "taps": taps, "N": n, "cells": cells}
    ts = []
    for i in range(WARMUP + STEPS):
        if i == WARMUP:
            ctx.profile_enable(1)
        t0 = time.perf_counter()
        ir = ctx.conv_ir_from_room(d, channels, taps)
        t1 = time.perf_counter()
        ctx.conv_ir_free(ir)
        if i >= WARMUP:
            ts.append((t1 - t0) * 1e3)
    p = ctx.profile_read()
    out["call_ms"] = {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
    out["generator_launches_ms"] = round(p["kernel_ms"] / max(p["launches"], 1), 3)
    out["bracketed_calls"] = p["launches"]
    ctx.profile_enable(0)
    t0 = time.perf_counter()
    h = ctx.conv_ir_from_room(d, channels, taps, want_taps=True, load=False)
    out["pure_generator_with_read_back_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    ctx.close()
    t0 = time.perf_counter()
    ref = R.ir(d, channels, taps, 48000.0)
    out["numpy_reference_s"] = round(time.perf_counter() - t0, 3)
    out["candidates"], out["in_range_ch0"] = ref.candidates, ref.in_range
    rms = max(float(np.sqrt(np.mean((h[e].astype(np.float64) - ref.h[e]) ** 2)) / np.sqrt(np.mean(ref.h[e].astype(np.float64) ** 2))) for e in range(channels))
    mx = max(float(np.abs(h[e].astype(np.float64) - ref.h[e]).max() / np.abs(ref.h[e]).max()) for e in range(channels))
    out["parity"] = {"rel_rms": rms, "max_abs_over_max": mx, "bitwise": bool(np.array_equal(h, ref.h))}
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "default")
