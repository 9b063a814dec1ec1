"""Dev aid: what GAS_FLAG_ER_TAP_FADE costs, one shape and one list of cases per run.

  python tools/time_er_fade.py 4096 256 4096 er_plain er_hrtf_plain er_fade_same        (cfg5's shape; and 8192 512 4096)
  python tools/time_er_fade.py 4096 256 4096 er_fade_changed

Cases: er_* is the chain [ER] (k_er_only, summed); er_hrtf_* the chain [ER, HRTF] under GAS_FLAG_PEAKS_DRAINING_ONLY with
one playback in 64 draining (the benchmark's arrangement); er_hrtfpk_* the same chain with every peak exact.  *_plain: a
context without the flag (k_er_only; the fused k_hrtf_uni<ER>; for er_hrtfpk the split k_hrtf_ols<ER>).  *_fade_same: a
flagged context whose taps never change -- the cost of the compare (and, for [ER, HRTF], of two launches and the row
round trip).  *_fade_changed: every source's taps change in every
callback -- the doubled gathers.  Every case republishes its rows before every callback (the same rows, or two draws in
turn), so the host's share is the same in all of them; callbacks are the device-memory form and name their list once.

Prints the wall clock per callback (publish, launches, synchronise; median of STEPS).  The kernels' own times come from
running this under `rocprofv3 --kernel-trace --stats` in a run of its own: a flagged k_er_only is one kernel name in
both of its forms (summed and rows_out) and whether or not taps changed, so cases that would share a name go into
separate runs.  A tree without the flag (an older checkout, for comparison) runs the *_plain cases."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
WARMUP, STEPS = 10, 100
DIRS = 1024


def run(case, n, F, ring):
    chain = (K.FX_EARLY_REFLECTIONS, K.FX_HRTF) if case.startswith("er_hrtf") else (K.FX_EARLY_REFLECTIONS,)
    draining_only = case.startswith("er_hrtf_")
    flags = (K.FLAG_ER_TAP_FADE if "_fade_" in case else 0) | (K.FLAG_PEAKS_DRAINING_ONLY if draining_only else 0)
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=F, er_ring_frames=ring, flags=flags)
    if K.FX_HRTF in chain:
        ctx.hrtf_load(synth.synthetic_hrir(rng, dirs=DIRS))
    slots = np.ascontiguousarray(ctx.source_alloc_many(n, K.KIND_EFFECT, chain), np.uint32)
    if draining_only:
        for s in slots[::64]:
            ctx.source_set_draining(int(s), True)
    draws = [synth.draw_params(rng, n, dirs=DIRS, ring_frames=ring, frames=F) for _ in range(2)]
    assert (draws[0]["er_delay"] != draws[1]["er_delay"]).any(axis=1).all()
    if not case.endswith("_changed"):
        draws[1] = draws[0]
    src = torch.from_numpy(synth.draw_sources(rng, n, F)).cuda()
    out = torch.zeros((1, F, 2), dtype=torch.float32, device="cuda")
    peaks = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ts = []
    for i in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        ctx.params_publish_batch(slots, draws[i & 1])
        rc = ctx.process_block_raw(src.data_ptr(), slots if i == 0 else None, n, F, out.data_ptr(), peaks.data_ptr(), K.MEM_DEVICE)  # the list is named once
        assert rc == 0, (case, rc)
        ctx.synchronize()
        t1 = time.perf_counter()
        if i >= WARMUP:
            ts.append((t1 - t0) * 1e6)
    mix = out.cpu().numpy()
    assert np.isfinite(mix).all() and np.abs(mix).max() > 0
    ctx.close()
    return {"callback_us": {"median": round(float(np.median(ts)), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}, "mix_abs_max": round(float(np.abs(mix).max()), 4)}


def main(argv):
    n, F, ring = (int(v) for v in argv[:3])
    out = {"n": n, "frames": F, "ring": ring, "steps": STEPS}
    for case in argv[3:]:
        out[case] = run(case, n, F, ring)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
