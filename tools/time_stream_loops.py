"""Dev aid: what gas_stream_set_loop costs per callback, 8192 plain [HRTF] stream playbacks (s16 mono) x 512 frames.

Three cases on the same parameter list: unlooped (streams long enough not to end), FORWARD with L much larger than F
(one conditional subtract per frame) and FORWARD with L = 37 (a seam every 37 frames, the 32-bit remainder per lane),
each through the fused prologue (the route the library takes) and through the rows-first route
(GAS_STREAM_ROWS_FIRST=1, read when a context is created: k_sample_sources, then the row form of the HRTF kernel).
Every callback is timed by its own pair of events in device memory; a figure is the median over the callbacks of one
repeat, and the line shows the median, smallest and largest of REPEATS repeats.  Run it on the parent commit too
(there only the unlooped case exists: --unlooped-only) to compare the unlooped callback across the change.

  python tools/time_stream_loops.py [--unlooped-only] [n]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
REPEATS = 5
WARMUP, STEPS = 10, 100


def callback_us(n, loop_len, rows_first, frames=512, dirs=64):
    os.environ["GAS_STREAM_ROWS_FIRST"] = "1" if rows_first else "0"
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames, flags=K.FLAG_PEAKS_DRAINING_ONLY)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.hrtf_load(synth.synthetic_hrir(np.random.default_rng(7), dirs=dirs))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=dirs, frames=frames))
    total = (WARMUP + REPEATS * STEPS + 2) * frames
    length = total if loop_len is None else max(loop_len, 64)
    sids = []
    for i in range(16):  # a few streams shared by all playbacks, every playback at its own start
        sid = ctx.stream_create((rng.uniform(-0.5, 0.5, length + 4096) * 32767).astype(np.int16))
        if loop_len is not None:
            ctx.stream_set_loop(sid, K.LOOP_FORWARD, 0, loop_len)
        sids.append(sid)
    for i, s in enumerate(slots):
        ctx.source_bind_stream(s, sids[i % len(sids)], start_frame=int(rng.integers(0, 4096)))
    out = torch.zeros(1, frames, 2, device="cuda")
    pk = torch.zeros(n, 2, device="cuda")
    sl = np.ascontiguousarray(slots, dtype=np.uint32)
    ptr = sl.ctypes.data_as(C.c_void_p)

    def callback():
        rc = ctx.lib.gas_process_block_streams(ctx.h, ptr, n, frames, C.c_void_p(out.data_ptr()), C.c_void_p(pk.data_ptr()), None, K.MEM_DEVICE)
        assert rc == 0, rc

    for _ in range(WARMUP):
        callback()
    torch.cuda.synchronize()
    got = []
    for _ in range(REPEATS):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
        for e0, e1 in ev:
            e0.record()
            callback()
            e1.record()
        torch.cuda.synchronize()
        got.append(float(np.median([1e3 * e0.elapsed_time(e1) for e0, e1 in ev])))
    ctx.close()
    return np.array(got)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 8192
    cases = [("unlooped", None)]
    if "--unlooped-only" not in sys.argv and hasattr(K, "LOOP_FORWARD"):
        cases += [("forward_L_1e6", 1000000), ("forward_L_37", 37)]
    for name, L in cases:
        for rows_first in (False, True):
            us = callback_us(n, L, rows_first)
            print(json.dumps({"n": n, "case": name, "route": "rows_first" if rows_first else "fused", "callback_us_median": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}))


if __name__ == "__main__":
    main()
