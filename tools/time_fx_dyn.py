"""Dev aid: time of the GAS_FX_DISTORTION / GAS_FX_COMPRESSOR stage (k_fx_dyn) and of [DISTORTION, HRTF], F = 512.

The stage alone is the difference of a chain with the kind twice and once ([K, K] - [K]: the same callback plus one
more k_fx_dyn launch); its row bytes are 16 F per source (read + write), against the 8 TB/s roof."""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
DIST, COMP, HRTF = K.FX_DISTORTION, K.FX_COMPRESSOR, K.FX_HRTF
ROOF = 8e12


def callback_us(chain, n, frames=512, steps=100, mode=K.DISTORTION_CLIP):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.hrtf_load(synth.synthetic_hrir(rng, dirs=1024))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=1024, frames=frames))
    s = K.fx_dyn_settings_defaults(n)
    s["distortion_mode"] = mode
    s["distortion_drive"] = 0.5
    s["distortion_pre_gain_db"] = 12.0
    s["compressor_threshold_db"] = -20.0
    ctx.fx_dyn_settings_publish(slots, s)
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
        for name, kind, mode in (("distortion CLIP", DIST, K.DISTORTION_CLIP), ("distortion OVERDRIVE", DIST, K.DISTORTION_OVERDRIVE), ("compressor", COMP, 0)):
            once = callback_us((kind,), n, F, mode=mode)
            twice = callback_us((kind, kind), n, F, mode=mode)
            stage = twice - once
            row_bytes = 16 * F * n
            print(json.dumps({"what": f"{name} stage", "n": n, "frames": F, "callback_us": round(once, 2), "stage_us": round(stage, 2), "roof_fraction": round(row_bytes / (stage * 1e-6) / ROOF, 3) if stage > 0 else None}))
        t = callback_us((DIST, HRTF), n, F)
        print(json.dumps({"what": "[DISTORTION, HRTF] callback", "n": n, "frames": F, "callback_us": round(t, 2)}))


if __name__ == "__main__":
    main()
