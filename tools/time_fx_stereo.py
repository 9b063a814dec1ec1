"""Dev aid: time of the GAS_FX_PANNER / GAS_FX_STEREO_ENHANCE / GAS_FX_LIMITER stages (k_fx_stereo) at F = 512, with
the GAS_FX_AMPLIFY stage measured the same way in the same run as the yardstick (pointwise, the same bytes).

A stage alone is the difference of a chain with the kind twice and once ([K, K] - [K]: the same callback plus one more
launch of the stage).  Bytes per source and block, against the 8 TB/s roof: 16 F for the rows in and out (the stereo
enhance adds 4 F written into its ring and up to 4 F read back from it; not counted, so its fraction is a lower
bound).  Every figure is the median of --repeats runs of 100 callbacks; the spread (min .. max) is printed with it.
The limiter is timed twice: on the quiet input of the other stages (|x| < 0.5: no sample above the default soft-clip
level, no log / exp) and on a loud one (|x| < 2: about 60 % of the samples take the soft-clip branch)."""
import argparse
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
KINDS = (("amplify", K.FX_AMPLIFY, 0.5), ("panner", K.FX_PANNER, 0.5), ("stereo enhance", K.FX_STEREO_ENHANCE, 0.5), ("limiter (quiet)", K.FX_LIMITER, 0.5), ("limiter (loud)", K.FX_LIMITER, 2.0))
ROOF = 8e12


def callback_us(chain, n, frames=512, steps=100, amp=0.5):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rings = n * sum(k == K.FX_STEREO_ENHANCE for k in chain)
    if rings:
        ctx.reserve_fx_stereo(rings)
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=8, frames=frames))
    s = K.fx_stereo_settings_defaults(n)
    s["panner_pan"] = 0.3
    s["enhance_pan_pullout"] = 1.5
    s["enhance_time_pullout_ms"] = 10.0  # 480 frames back: most reads of a block come from the ring
    s["enhance_surround"] = 0.5
    ctx.fx_stereo_settings_publish(slots, s)
    src = (torch.rand(n, frames, 2, device="cuda") - 0.5) * (2.0 * amp)
    out = torch.zeros(1, frames, 2, device="cuda")
    pk = torch.zeros(n, 2, device="cuda")
    for _ in range(10):
        ctx.process_block_raw(src.data_ptr(), slots, n, frames, out.data_ptr(), pk.data_ptr(), K.MEM_DEVICE)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        ctx.process_block_raw(src.data_ptr(), None, n, frames, out.data_ptr(), pk.data_ptr(), K.MEM_DEVICE)
    e1.record()
    torch.cuda.synchronize()
    ctx.close()
    return 1e3 * e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[256, 8192, 65536])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    F = 512
    for n in a.sizes:
        for name, kind, amp in KINDS:
            t1 = [callback_us((kind,), n, F, amp=amp) for _ in range(a.repeats)]
            t2 = [callback_us((kind, kind), n, F, amp=amp) for _ in range(a.repeats)]
            stages = sorted(y - x for x, y in zip(t1, t2))
            stage = statistics.median(stages)
            line = {"what": f"{name} stage", "n": n, "frames": F, "callback_us": round(statistics.median(t1), 2), "stage_us": round(stage, 2), "stage_us_min_max": [round(stages[0], 2), round(stages[-1], 2)]}
            line["roof_fraction"] = round(16 * F * n / (stage * 1e-6) / ROOF, 3) if stage > 0 else None
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
