"""Dev aid: time of the GAS_FX_FILTER stage (k_fx_filter) by slope and type, F = 512, next to what it replaces.

A stage alone is the difference of a chain with the kind twice and once ([K, K] - [K]: the same callback plus one more
launch); AMPLIFY is timed the same way in the same run as the drift yardstick.  The workaround the kind replaces is
timed as [LP, LP, LP, LP] - [] and [LP, LP] - [LP] (run with GAS_SHELF_SCAN=0 for the engine-order kernel).  Every
figure is the median of REPEATS measurements of 100 callbacks, with the smallest and largest next to it.
Bytes per source and block, against the 8 TB/s roof: 16 F (the rows in and out; bank and settings are noise).

  python tools/time_fx_filter.py [--old-only] [sizes ...]     (--old-only: the chains a library without kind 24 has)"""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
LP, AMP = K.FX_LOWPASS, K.FX_AMPLIFY
FILTER = getattr(K, "FX_FILTER", None)
ROOF = 8e12
REPEATS = 5


def callback_us(chain, n, frames=512, steps=100, db=0, ftype=0):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n_flt = sum(k == FILTER for k in chain)
    if n_flt:
        ctx.reserve_fx_filter(n * n_flt)
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=8, frames=frames))
    if n_flt:
        s = K.fx_filter_settings_defaults(n)
        s["type"], s["db"] = ftype, db
        s["cutoff_hz"] = rng.uniform(200, 8000, s["cutoff_hz"].shape)
        s["gain"] = rng.uniform(0.5, 2.0, s["gain"].shape)
        ctx.fx_filter_settings_publish(slots, s)
    src = torch.rand(n, frames, 2, device="cuda") - 0.5
    out = torch.zeros(1, frames, 2, device="cuda")
    pk = torch.zeros(n, 2, device="cuda")
    for _ in range(10):
        ctx.process_block_raw(src.data_ptr(), slots, n, frames, out.data_ptr(), pk.data_ptr(), K.MEM_DEVICE)
    torch.cuda.synchronize()
    got = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            ctx.process_block_raw(src.data_ptr(), None, n, frames, out.data_ptr(), pk.data_ptr(), K.MEM_DEVICE)
        e1.record()
        torch.cuda.synchronize()
        got.append(1e3 * e0.elapsed_time(e1) / steps)
    ctx.close()
    return np.array(got)


def report(what, n, F, longer, shorter, stages_of_bytes=1):
    d = np.median(longer) - np.median(shorter)
    lo, hi = longer.min() - shorter.max(), longer.max() - shorter.min()
    b = 16 * F * n * stages_of_bytes
    print(json.dumps({"what": what, "n": n, "frames": F, "callback_us": round(float(np.median(shorter)), 2), "stage_us": round(float(d), 2), "stage_us_min_max": [round(float(lo), 2), round(float(hi), 2)], "roof_fraction": round(b / (d * 1e-6) / ROOF, 3) if d > 0 else None}), flush=True)


def main():
    args = sys.argv[1:]
    old_only = "--old-only" in args or FILTER is None
    sizes = [int(a) for a in args if not a.startswith("--")] or [256, 8192, 65536]
    F = 512
    for n in sizes:
        report("amplify stage", n, F, callback_us((AMP, AMP), n, F), callback_us((AMP,), n, F))
        empty = callback_us((), n, F)
        one = callback_us((LP,), n, F)
        report("[LP] stage ([LP, LP] - [LP])", n, F, callback_us((LP, LP), n, F), one)
        report("[LP, LP, LP, LP] - []", n, F, callback_us((LP, LP, LP, LP), n, F), empty, 4)
        if old_only:
            continue
        for db in range(4):
            report(f"filter stage lowpass {6 * (db + 1)} dB", n, F, callback_us((FILTER, FILTER), n, F, db=db), callback_us((FILTER,), n, F, db=db))
        report("[FILTER 24 dB] - []", n, F, callback_us((FILTER,), n, F, db=3), empty)
        for name, ftype in (("highshelf", K.FILTER_HIGHSHELF), ("bandpass", K.FILTER_BANDPASS), ("bandlimit", K.FILTER_BANDLIMIT)):
            report(f"filter stage {name} 24 dB", n, F, callback_us((FILTER, FILTER), n, F, db=3, ftype=ftype), callback_us((FILTER,), n, F, db=3, ftype=ftype))


if __name__ == "__main__":
    main()
