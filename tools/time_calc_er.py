"""Dev aid: k_calc_er next to k_calc_spatialization, one source count per run.

  python tools/time_calc_er.py 8192          (and 65536)

Every call is the device-memory form: poses and results stay in HBM, the rooms / configs / slot list are the small
host uploads each call makes anyway.  Prints the wall clock of a whole call (uploads, launch, synchronise) as the median
of STEPS calls; the kernels' own times come from running this under `rocprofv3 --kernel-trace --stats` in a run of its
own, where both kernels then appear with STEPS + WARMUP dispatches each at this one source count."""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
WARMUP, STEPS = 5, 50
F, RING = 256, 512  # the smallest ring: 65536 rings of it are 256 MiB
vp = C.c_void_p


def main(n):
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=F, er_ring_frames=RING)
    slots = np.ascontiguousarray(ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_EARLY_REFLECTIONS,)), np.uint32)
    rooms, room_index, poses, listener = synth.draw_room_scene(rng, n)
    cfgs = K.default_spat3d_config()
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    d_taps = torch.zeros(n * K.ER_TAPS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_rows = torch.zeros(n * K.PARAMS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda a: a.ctypes.data_as(vp)  # noqa: E731

    def spat():
        return ctx.lib.gas_calc_spatialization(ctx.h, ptr(cfgs), 1, None, vp(d_poses.data_ptr()), ptr(listener), 1, ptr(slots), n, vp(d_rows.data_ptr()), K.MEM_DEVICE)

    def er():
        return ctx.lib.gas_calc_early_reflections(ctx.h, ptr(rooms), len(rooms), ptr(room_index), vp(d_poses.data_ptr()), ptr(listener), ptr(slots), n, vp(d_taps.data_ptr()), K.MEM_DEVICE)

    out = {"n": n}
    for name, call in (("gas_calc_spatialization", spat), ("gas_calc_early_reflections", er)):
        ts = []
        for i in range(WARMUP + STEPS):
            t0 = time.perf_counter()
            rc = call()
            t1 = time.perf_counter()
            assert rc == 0, (name, rc)
            if i >= WARMUP:
                ts.append((t1 - t0) * 1e6)
        out[name + "_call_us"] = {"median": round(float(np.median(ts)), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
    taps = d_taps.cpu().numpy().view(K.ER_TAPS_DTYPE)
    out["taps_nonzero_share"] = round(float((taps["gain"] > 0).mean()), 3)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8192)
