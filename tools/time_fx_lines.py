"""Dev aid: time of the GAS_FX_DELAY / GAS_FX_REVERB stages (k_fx_line) and of [REVERB, HRTF], F = 512.

A stage alone is the difference of a chain with the kind twice and once ([K, K] - [K]: the same callback plus one more
k_fx_line launch).  At 65 536 sources the delay is [DELAY, AMPLIFY] - [AMPLIFY] instead (two delay lines per source
would be 200 GB).  Bytes per source and block, against the 8 TB/s roof: delay 56 F (rows in and out, ring write, two
tap reads, feedback read and write), reverb 224 F (rows in and out; per ear the echo, 8 combs and 4 allpasses, each
read and written)."""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
DELAY, REVERB, HRTF, AMP = K.FX_DELAY, K.FX_REVERB, K.FX_HRTF, K.FX_AMPLIFY
ROOF = 8e12
BYTES = {DELAY: 56, REVERB: 224}


def callback_us(chain, n, frames=512, steps=100):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.reserve_fx_lines(n * chain.count(DELAY), n * chain.count(REVERB))
    ctx.hrtf_load(synth.synthetic_hrir(rng, dirs=1024))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=1024, frames=frames))
    s = K.fx_line_settings_defaults(n)
    s["delay_feedback_active"] = 1  # the engine's defaults otherwise (taps 250 / 500 ms, feedback 340 ms; reverb)
    ctx.fx_line_settings_publish(slots, s)
    src = torch.rand(n, frames, 2, device="cuda") - 0.5
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
    sizes = [int(a) for a in sys.argv[1:]] or [256, 8192, 65536]
    F = 512
    for n in sizes:
        for name, kind in (("delay", DELAY), ("reverb", REVERB)):
            once, twice = ((kind,), (kind, kind)) if not (kind == DELAY and n > 32768) else ((AMP,), (DELAY, AMP))
            try:
                t1 = callback_us(once, n, F)
                t2 = callback_us(twice, n, F)
            except gas.GasError as e:
                print(json.dumps({"what": f"{name} stage", "n": n, "error": str(e)}))
                continue
            stage = t2 - t1
            b = BYTES[kind] * F * n
            print(json.dumps({"what": f"{name} stage", "n": n, "frames": F, "chains": [list(once), list(twice)], "callback_us": round(t1, 2), "stage_us": round(stage, 2), "roof_fraction": round(b / (stage * 1e-6) / ROOF, 3) if stage > 0 else None}))
        t = callback_us((REVERB, HRTF), n, F)
        print(json.dumps({"what": "[REVERB, HRTF] callback", "n": n, "frames": F, "callback_us": round(t, 2)}))


if __name__ == "__main__":
    main()
