"""Dev aid: what gas_source_feed_rows costs and saves, 8192 plain [HRTF] sources x 512 frames.

  python tools/time_stream_feed.py mixed   one mixed callback (4096 rows fed from device memory as f32 stereo + 4096 s16
                                           streams: gas_source_feed_rows + gas_process_block_streams) against what the
                                           same audio takes without the entry: gas_process_block over the 4096 rows in
                                           one context plus gas_process_block_streams over the 4096 streams in another
                                           (the CPU sum of the two mixes is not counted)
  python tools/time_stream_feed.py guard   the all-stream 8192-source callback, plain and onto two buses: run it for this
                                           build and for the build to compare with, alternating, in one session
  python tools/time_stream_feed.py host    8192 rows fed from host memory, f32 stereo (32 MiB) against s16 mono (8 MiB):
                                           gas_source_feed_rows(GAS_MEM_HOST) + gas_ctx_synchronize, wall clock (the
                                           callback that consumes the rows runs between two feeds, outside the clock)

mixed / guard: every callback is timed by its own pair of events; a figure is the median over the callbacks of one
repeat; the contexts of one comparison live side by side and the repeats alternate between them; a line shows the
median, smallest and largest of REPEATS repeats (the spread to hold a difference against)."""
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
REPEATS = 7
WARMUP, STEPS = 10, 100
N, F, DIRS = 8192, 512, 64
vp = C.c_void_p


def make_ctx(n):
    ctx = gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PEAKS_DRAINING_ONLY)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.hrtf_load(synth.synthetic_hrir(np.random.default_rng(7), dirs=DIRS))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
    ctx.params_publish_batch(slots, synth.draw_params(np.random.default_rng(0), n, dirs=DIRS, frames=F))
    return ctx, np.ascontiguousarray(slots, np.uint32)


def bind_streams(ctx, slots):
    """A few s16 mono streams shared by all playbacks, every playback at its own start; none ends while the clock runs."""
    rng = np.random.default_rng(1)
    length = (WARMUP + REPEATS * STEPS + 2) * F + 8192
    sids = [ctx.stream_create((rng.uniform(-0.5, 0.5, length) * 32767).astype(np.int16)) for _ in range(16)]
    for i, s in enumerate(slots):
        ctx.source_bind_stream(s, sids[i % len(sids)], start_frame=int(rng.integers(0, 4096)))


class Mixed:
    name = "mixed: feed_rows + process_block_streams, one context"

    def __init__(self):
        self.ctx, self.sl = make_ctx(N)
        bind_streams(self.ctx, self.sl[1::2])
        self.fed = np.ascontiguousarray(self.sl[0::2])
        self.rows = torch.rand(N // 2, F, 2, device="cuda") - 0.5
        self.out = torch.zeros(1, F, 2, device="cuda")
        self.pk = torch.zeros(N, 2, device="cuda")

    def callback(self):
        ctx = self.ctx
        rc = ctx.lib.gas_source_feed_rows(ctx.h, self.fed.ctypes.data_as(vp), vp(self.rows.data_ptr()), K.PCM_F32, 2, len(self.fed), F, K.MEM_DEVICE)
        assert rc == 0, rc
        rc = ctx.lib.gas_process_block_streams(ctx.h, self.sl.ctypes.data_as(vp), N, F, vp(self.out.data_ptr()), vp(self.pk.data_ptr()), None, K.MEM_DEVICE)
        assert rc == 0, rc

    def close(self):
        self.ctx.close()


class TwoCallbacks:
    name = "two callbacks: process_block (rows) + process_block_streams (streams), two contexts"

    def __init__(self):
        self.ca, self.sa = make_ctx(N // 2)
        self.cb, self.sb = make_ctx(N // 2)
        bind_streams(self.cb, self.sb)
        self.rows = torch.rand(N // 2, F, 2, device="cuda") - 0.5
        self.out = torch.zeros(2, 1, F, 2, device="cuda")
        self.pk = torch.zeros(2, N // 2, 2, device="cuda")
        self.first = True

    def callback(self):
        ca, cb = self.ca, self.cb
        rc = ca.lib.gas_process_block(ca.h, vp(self.rows.data_ptr()), self.sa.ctypes.data_as(vp) if self.first else None, N // 2, F, vp(self.out[0].data_ptr()), vp(self.pk[0].data_ptr()), K.MEM_DEVICE)
        assert rc == 0, rc
        rc = cb.lib.gas_process_block_streams(cb.h, self.sb.ctypes.data_as(vp), N // 2, F, vp(self.out[1].data_ptr()), vp(self.pk[1].data_ptr()), None, K.MEM_DEVICE)
        assert rc == 0, rc
        self.first = False

    def close(self):
        self.ca.close()
        self.cb.close()


class AllStream:
    def __init__(self, n_buses):
        self.name = "all-stream" + (f", {n_buses} buses" if n_buses else "")
        self.n_buses = n_buses
        self.ctx, self.sl = make_ctx(N)
        bind_streams(self.ctx, self.sl)
        if n_buses:
            r = K.bus_routes(N)
            r["dry_bus"] = np.arange(N) % n_buses
            self.ctx.bus_routes_publish(self.sl, r)
        self.out = torch.zeros(max(n_buses, 1), 1, F, 2, device="cuda")
        self.pk = torch.zeros(N, 2, device="cuda")

    def callback(self):
        ctx, ptr = self.ctx, self.sl.ctypes.data_as(vp)
        if self.n_buses:
            rc = ctx.lib.gas_process_block_streams_buses(ctx.h, ptr, N, F, vp(self.out.data_ptr()), self.n_buses, vp(self.pk.data_ptr()), None, K.MEM_DEVICE)
        else:
            rc = ctx.lib.gas_process_block_streams(ctx.h, ptr, N, F, vp(self.out.data_ptr()), vp(self.pk.data_ptr()), None, K.MEM_DEVICE)
        assert rc == 0, rc

    def close(self):
        self.ctx.close()


def repeat_us(case):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for e0, e1 in ev:
        e0.record()
        case.callback()
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([1e3 * e0.elapsed_time(e1) for e0, e1 in ev]))


def compare(cases, what):
    for c in cases:
        for _ in range(WARMUP):
            c.callback()
    torch.cuda.synchronize()
    got = {c.name: [] for c in cases}
    for _ in range(REPEATS):
        for c in cases:
            got[c.name].append(repeat_us(c))
    for c in cases:
        us = np.array(got[c.name])
        print(json.dumps({"what": what, "case": c.name, "lib": gas.capi.library_path(), "callback_us_median": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}), flush=True)
        c.close()


def host_feed():
    ctx, sl = make_ctx(N)
    rng = np.random.default_rng(2)
    rows = {"f32_stereo": (rng.uniform(-0.5, 0.5, (N, F, 2)).astype(np.float32), K.PCM_F32, 2), "s16_mono": ((rng.uniform(-0.5, 0.5, (N, F)) * 32767).astype(np.int16), K.PCM_S16, 1)}
    out = torch.zeros(1, F, 2, device="cuda")
    pk = torch.zeros(N, 2, device="cuda")
    got = {k: [] for k in rows}
    for rep in range(REPEATS + 1):  # the first repeat sizes the staging and is dropped
        for k, (data, fmt, ch) in rows.items():
            times = []
            for _ in range(20):
                t0 = time.perf_counter()
                rc = ctx.lib.gas_source_feed_rows(ctx.h, sl.ctypes.data_as(vp), data.ctypes.data_as(vp), fmt, ch, N, F, K.MEM_HOST)
                ctx.synchronize()
                times.append(time.perf_counter() - t0)
                assert rc == 0, rc
                rc = ctx.lib.gas_process_block_streams(ctx.h, sl.ctypes.data_as(vp), N, F, vp(out.data_ptr()), vp(pk.data_ptr()), None, K.MEM_DEVICE)
                ctx.synchronize()  # the callback that consumes the rows, outside the clock
                assert rc == 0, rc
            if rep:
                got[k].append(1e6 * float(np.median(times)))
    for k, (data, _, _) in rows.items():
        us = np.array(got[k])
        print(json.dumps({"what": "host", "case": k, "bytes": int(data.nbytes), "feed_us_median": round(float(np.median(us)), 1), "min": round(float(us.min()), 1), "max": round(float(us.max()), 1)}), flush=True)
    ctx.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "mixed"
    if mode == "mixed":
        compare([Mixed(), TwoCallbacks()], "mixed")
    elif mode == "guard":
        compare([AllStream(0), AllStream(2)], "guard")
    elif mode == "host":
        host_feed()
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
