"""Dev aid: callback time of gas_process_block_streams_buses, 8192 plain [HRTF] stream playbacks (s16 mono) x 512 frames
onto 2 and 4 buses, half the sources carrying a send.

Per bus count three figures on the same parameters and routes:
  fused       the route the library takes: k_hrtf_uni<SRC_PCM, BUS2> samples the streams itself, one launch per pair of buses
  rows_first  GAS_STREAM_ROWS_FIRST=1 (read when a context is created): k_sample_sources, then k_hrtf_uni<BUS2> over the rows
  float_rows  for orientation: gas_process_block_buses over float rows already in HBM (what tools/time_buses.py times,
              with this tool's routes and its event-per-callback method)
Every callback is timed by its own pair of events; a figure is the median over the callbacks of one repeat.  The three
contexts live side by side and the repeats alternate between them, so that drift of the machine hits all alike; the
line shows the median, smallest and largest of REPEATS repeats (the spread to hold a difference against).

  python tools/time_stream_buses.py [n]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402
from godot_audio_spatializer_amd import synth  # noqa: E402

K = gas.capi
REPEATS = 7
WARMUP, STEPS = 10, 100
F, DIRS = 512, 64


def make_routes(n, n_buses):
    """Dry buses in rotation; every second source sends onto the next bus."""
    r = K.bus_routes(n)
    i = np.arange(n)
    r["dry_bus"] = (i // 2) % n_buses
    r["send_bus"] = np.where(i % 2 == 0, (r["dry_bus"] + 1) % n_buses, K.BUS_NONE)
    r["send"][:, 0, :] = 0.3
    return r


class Case:
    def __init__(self, route, n, n_buses):
        os.environ["GAS_STREAM_ROWS_FIRST"] = "1" if route == "rows_first" else "0"
        rng = np.random.default_rng(0)
        self.n, self.n_buses, self.route = n, n_buses, route
        self.ctx = ctx = gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PEAKS_DRAINING_ONLY)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.hrtf_load(synth.synthetic_hrir(np.random.default_rng(7), dirs=DIRS))
        self.slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
        ctx.params_publish_batch(self.slots, synth.draw_params(rng, n, dirs=DIRS, frames=F))
        ctx.bus_routes_publish(self.slots, make_routes(n, n_buses))
        self.src = None
        if route == "float_rows":
            self.src = torch.rand(n, F, 2, device="cuda") - 0.5
        else:
            length = (WARMUP + REPEATS * STEPS + 2) * F + 4096  # no playback ends while the clock runs
            sids = [ctx.stream_create((rng.uniform(-0.5, 0.5, length + 4096) * 32767).astype(np.int16)) for _ in range(16)]
            for i, s in enumerate(self.slots):  # a few streams shared by all playbacks, every playback at its own start
                ctx.source_bind_stream(s, sids[i % len(sids)], start_frame=int(rng.integers(0, 4096)))
        self.out = torch.zeros(n_buses, 1, F, 2, device="cuda")
        self.pk = torch.zeros(n, 2, device="cuda")
        self.sl = np.ascontiguousarray(self.slots, dtype=np.uint32)
        self.first = True

    def callback(self):
        ctx, ptr = self.ctx, self.sl.ctypes.data_as(C.c_void_p)
        if self.src is None:
            rc = ctx.lib.gas_process_block_streams_buses(ctx.h, ptr, self.n, F, C.c_void_p(self.out.data_ptr()), self.n_buses, C.c_void_p(self.pk.data_ptr()), None, K.MEM_DEVICE)
        else:  # the fused bus form reuses the previous call's list
            rc = ctx.lib.gas_process_block_buses(ctx.h, C.c_void_p(self.src.data_ptr()), ptr if self.first else None, self.n, F, C.c_void_p(self.out.data_ptr()), self.n_buses, C.c_void_p(self.pk.data_ptr()), K.MEM_DEVICE)
        self.first = False
        assert rc == 0, rc

    def repeat_us(self):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
        for e0, e1 in ev:
            e0.record()
            self.callback()
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([1e3 * e0.elapsed_time(e1) for e0, e1 in ev]))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 8192
    for n_buses in (2, 4):
        cases = [Case(route, n, n_buses) for route in ("fused", "rows_first", "float_rows")]
        for c in cases:
            for _ in range(WARMUP):
                c.callback()
        torch.cuda.synchronize()
        got = {c.route: [] for c in cases}
        for _ in range(REPEATS):
            for c in cases:
                got[c.route].append(c.repeat_us())
        for c in cases:
            us = np.array(got[c.route])
            print(json.dumps({"n": n, "n_buses": n_buses, "route": c.route, "callback_us_median": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}), flush=True)
            c.ctx.close()


if __name__ == "__main__":
    main()
