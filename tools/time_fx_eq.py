"""Dev aid: time of the GAS_FX_EQ6 / _EQ10 / _EQ21 stages (k_fx_eq) and of [EQ10, HRTF], F = 512.

A stage alone is the difference of a chain with the kind twice and once ([K, K] - [K]: the same callback plus one more
k_fx_eq launch).  Bytes per source and block, against the 8 TB/s roof: 16 F (the rows in and out; the 672-byte bank
and the settings row are noise)."""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
HRTF = K.FX_HRTF
EQS = (("eq6", K.FX_EQ6), ("eq10", K.FX_EQ10), ("eq21", K.FX_EQ21))
ROOF = 8e12


def callback_us(chain, n, frames=512, steps=100):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.reserve_fx_eq(n * sum(k in K.EQ_BANDS for k in chain))
    ctx.hrtf_load(synth.synthetic_hrir(rng, dirs=1024))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=1024, frames=frames))
    s = K.fx_eq_settings_defaults(n)
    s["band_gain_db"] = rng.uniform(-60, 24, s["band_gain_db"].shape)
    ctx.fx_eq_settings_publish(slots, s)
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
        for name, kind in EQS:
            once, twice = (kind,), (kind, kind)
            t1 = callback_us(once, n, F)
            t2 = callback_us(twice, n, F)
            stage = t2 - t1
            b = 16 * F * n
            print(json.dumps({"what": f"{name} stage", "n": n, "frames": F, "callback_us": round(t1, 2), "stage_us": round(stage, 2), "roof_fraction": round(b / (stage * 1e-6) / ROOF, 3) if stage > 0 else None}))
        t = callback_us((K.FX_EQ10, HRTF), n, F)
        print(json.dumps({"what": "[EQ10, HRTF] callback", "n": n, "frames": F, "callback_us": round(t, 2)}))


if __name__ == "__main__":
    main()
