"""Dev aid: what GAS_FLAG_HRTF_INTERPOLATE costs per callback, 8192 plain [HRTF] sources x 512 frames by default.

Timed on the same parameter list (directions drawn over the whole set, so the list has no runs):
  - the flagged kernel (k_hrtf_ols_blend) with 1, 2 and 4 non-zero weights per source;
  - k_hrtf_ols without the blend, reached with GAS_FLAG_DIRECTION_RUNS on this list without runs;
  - k_hrtf_uni (no flags).
Frequency-domain sums (GAS_FLAG_PEAKS_DRAINING_ONLY, nothing draining) unless --peaks.  Every figure is the median of
REPEATS measurements of 100 device-memory callbacks after 10 warm-up callbacks, with the smallest and largest next to it;
the ratios are of the medians.

--fade times GAS_FLAG_HRTF_BLEND_FADE instead: four-weight rows, every source's row replaced every --every K callbacks
(2 by default) and never, next to GAS_FLAG_HRTF_INTERPOLATE alone driven the same way.  Publishing 8192 rows from the
host costs far more than the kernel, so here every callback is timed by its own pair of events, recorded after the
publish (the callback's upload of the rows, inside gas_process_block, is in the figure for all three alike).

  python tools/time_hrtf_blend.py [--peaks] [--dirs D] [--fade [--every K]] [sizes ...]"""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
REPEATS = 5


def callback_us(n, flags, rows, dirs, frames=512, steps=100):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames, flags=flags)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.hrtf_load(synth.synthetic_hrir(np.random.default_rng(7), dirs=dirs))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=dirs, frames=frames))
    if rows:
        b = np.zeros(n, K.HRTF_BLEND_DTYPE)
        b["dir"][:, :rows] = rng.integers(0, dirs, (n, rows))
        b["weight"][:, :rows] = 1.0 / rows
        ctx.publish_hrtf_blend(slots, b)
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


def fade_callback_us(n, flags, every, dirs, frames=512, steps=40):
    """Per-callback event times; every `every` callbacks (0 = never) all sources get the other of two row sets."""
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames, flags=flags)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.hrtf_load(synth.synthetic_hrir(np.random.default_rng(7), dirs=dirs))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=dirs, frames=frames))
    sets = []
    for _ in range(2):
        b = np.zeros(n, K.HRTF_BLEND_DTYPE)
        b["dir"] = rng.integers(0, dirs, (n, 4))
        b["weight"] = 0.25
        sets.append(b)
    ctx.publish_hrtf_blend(slots, sets[0])
    src = torch.rand(n, frames, 2, device="cuda") - 0.5
    out = torch.zeros(1, frames, 2, device="cuda")
    pk = torch.zeros(n, 2, device="cuda")
    for _ in range(10):
        ctx.process_block_raw(src.data_ptr(), slots, n, frames, out.data_ptr(), pk.data_ptr(), K.MEM_DEVICE)
    torch.cuda.synchronize()
    got, which = [], 0
    for _ in range(REPEATS):
        pairs = []
        for step in range(steps):
            if every and step % every == 0:
                which ^= 1
                ctx.publish_hrtf_blend(slots, sets[which])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.process_block_raw(src.data_ptr(), slots, n, frames, out.data_ptr(), pk.data_ptr(), K.MEM_DEVICE)
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        got.append(1e3 * float(np.mean([a.elapsed_time(b) for a, b in pairs])))
    ctx.close()
    return np.array(got)


def main_fade(n, base, dirs, every, peaks):
    blend = K.FLAG_HRTF_INTERPOLATE
    ref = None
    for what, flags, ev in (("INTERPOLATE alone, rows replaced", blend, every), ("BLEND_FADE, no row changed", blend | K.FLAG_HRTF_BLEND_FADE, 0), (f"BLEND_FADE, every row changed every {every} callbacks", blend | K.FLAG_HRTF_BLEND_FADE, every)):
        t = fade_callback_us(n, base | flags, ev, dirs)
        m = float(np.median(t))
        ref = m if ref is None else ref
        print(json.dumps({"what": what, "n": n, "dirs": dirs, "exact_peaks": peaks, "callback_us": round(m, 2), "min_max": [round(float(t.min()), 2), round(float(t.max()), 2)], "ratio_to_interpolate": round(m / ref, 3)}), flush=True)


def main():
    args = sys.argv[1:]
    peaks = "--peaks" in args
    dirs = int(args[args.index("--dirs") + 1]) if "--dirs" in args else 1024
    skip = {args.index("--dirs") + 1} if "--dirs" in args else set()
    every = 2
    if "--every" in args:
        every = int(args[args.index("--every") + 1])
        skip.add(args.index("--every") + 1)
    sizes = [int(a) for i, a in enumerate(args) if not a.startswith("--") and i not in skip] or [8192]
    base = 0 if peaks else K.FLAG_PEAKS_DRAINING_ONLY
    if "--fade" in args:
        for n in sizes:
            main_fade(n, base, dirs, every, peaks)
        return
    for n in sizes:
        uni = callback_us(n, base, 0, dirs)
        ols = callback_us(n, base | K.FLAG_DIRECTION_RUNS, 0, dirs)
        for what, t in (("k_hrtf_uni", uni), ("k_hrtf_ols (DIRECTION_RUNS, no runs)", ols)):
            print(json.dumps({"what": what, "n": n, "dirs": dirs, "exact_peaks": peaks, "callback_us": round(float(np.median(t)), 2), "min_max": [round(float(t.min()), 2), round(float(t.max()), 2)]}), flush=True)
        for rows in (1, 2, 4):
            t = callback_us(n, base | K.FLAG_HRTF_INTERPOLATE, rows, dirs)
            m = float(np.median(t))
            print(json.dumps({"what": f"k_hrtf_ols_blend, {rows} non-zero weight(s)", "n": n, "dirs": dirs, "exact_peaks": peaks, "callback_us": round(m, 2), "min_max": [round(float(t.min()), 2), round(float(t.max()), 2)], "ratio_to_ols": round(m / float(np.median(ols)), 3), "ratio_to_uni": round(m / float(np.median(uni)), 3)}), flush=True)


if __name__ == "__main__":
    main()
