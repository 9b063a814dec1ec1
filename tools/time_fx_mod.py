"""Dev aid: time of the GAS_FX_CHORUS / GAS_FX_PHASER stages (k_fx_mod) and of [CHORUS, HRTF], F = 512.

A stage alone is the difference of a chain with the kind twice and once ([K, K] - [K]: the same callback plus one more
k_fx_mod launch).  Bytes per source and block, against the 8 TB/s roof: 16 F for the rows in and out, plus for the
chorus 8 F written into its ring and up to 8 F per voice read back from it (the ring reads of a block cover about the
block's length per voice, most of them older than the block)."""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
HRTF = K.FX_HRTF
KINDS = (("chorus", K.FX_CHORUS), ("phaser", K.FX_PHASER))
ROOF = 8e12


def callback_us(chain, n, frames=512, steps=100):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.reserve_fx_mod(n * sum(k == K.FX_CHORUS for k in chain), n * sum(k == K.FX_PHASER for k in chain))
    ctx.hrtf_load(synth.synthetic_hrir(rng, dirs=1024))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=1024, frames=frames))
    ctx.fx_mod_settings_publish(slots, K.fx_mod_settings_defaults(n))  # the engine's defaults: 2 chorus voices
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
    sizes = [int(a) for a in sys.argv[1:]] or [1, 64, 1024, 8192]
    F = 512
    for n in sizes:
        for name, kind in KINDS:
            t1 = callback_us((kind,), n, F)
            t2 = callback_us((kind, kind), n, F)
            stage = t2 - t1
            b = (16 * F + (8 * F + 2 * 8 * F if kind == K.FX_CHORUS else 0)) * n
            print(json.dumps({"what": f"{name} stage", "n": n, "frames": F, "callback_us": round(t1, 2), "stage_us": round(stage, 2), "roof_fraction": round(b / (stage * 1e-6) / ROOF, 3) if stage > 0 else None}), flush=True)
        t = callback_us((K.FX_CHORUS, HRTF), n, F)
        print(json.dumps({"what": "[CHORUS, HRTF] callback", "n": n, "frames": F, "callback_us": round(t, 2)}), flush=True)


if __name__ == "__main__":
    main()
