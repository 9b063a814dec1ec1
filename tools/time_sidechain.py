"""Dev aid: time of the GAS_FX_COMPRESSOR stage (k_fx_dyn) without and with sidechain keys, F = 512.

Measured like tools/time_fx_dyn.py: the stage alone is the difference of a chain with the compressor twice and once
([K, K] - [K]: the same callback plus one more k_fx_dyn launch), device-memory callbacks on the torch stream, HIP events
around 100 callbacks.  --keyed puts source i on key i % 8 at both positions (every source keyed, all eight keys in every
workgroup) and fills the keys with noise; the stage then moves the same row bytes plus 8 F bytes per key and workgroup.
--tree DIR imports the package (and its library) from another checkout, for an A/B against an older commit: such a
tree may lack the sidechain, so only the keyless case runs there.  --reps N repeats every figure in the process."""
import argparse
import json
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[256, 8192, 65536])
ap.add_argument("--keyed", action="store_true")
ap.add_argument("--tree", default=".")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()

sys.path.insert(0, args.tree)
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
COMP = K.FX_COMPRESSOR
ROOF = 8e12


def callback_us(chain, n, frames=512, steps=100, keyed=False):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=8, frames=frames))
    s = K.fx_dyn_settings_defaults(n)
    s["compressor_threshold_db"] = -20.0
    if keyed:
        s["compressor_sidechain"] = (1 + np.arange(n) % K.MAX_SIDECHAINS)[:, None]
        for k in range(K.MAX_SIDECHAINS):
            ctx.sidechain_set(k, rng.uniform(-0.5, 0.5, (frames, 2)).astype(np.float32))
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
    F = 512
    for n in args.sizes:
        for rep in range(args.reps):
            once = callback_us((COMP,), n, F, keyed=args.keyed)
            twice = callback_us((COMP, COMP), n, F, keyed=args.keyed)
            stage = twice - once
            row_bytes = 16 * F * n
            print(json.dumps({"what": "compressor stage", "label": args.label, "keyed": args.keyed, "n": n, "frames": F, "rep": rep, "callback_us": round(once, 2), "stage_us": round(stage, 2), "roof_fraction": round(row_bytes / (stage * 1e-6) / ROOF, 3) if stage > 0 else None}), flush=True)


if __name__ == "__main__":
    main()
