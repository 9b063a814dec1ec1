"""Dev aid: what gas_conv_process costs, one shape per run.

  python tools/time_conv.py 6 2.0 512        (instances, IR seconds at 48 kHz, frames)

Every instance has its own two-channel IR, so the multiply-accumulate stage's bytes are compulsory: per instance and
ear k_ir spectra of the ring and k_ir of the IR, 4 KiB each, read once, and one 4 KiB partial sum per chunk written.
Prints the wall clock per device-memory call (enqueue, three launches, synchronise; median of STEPS) and, from the same
run, gas_bandwidth_probe's time for a pure streaming launch over the same byte counts (its reads come from an arena
larger than the Infinity Cache: the HBM ceiling).  The kernels' own times (k_conv_forward, k_conv_mac, k_conv_inverse)
come from running this under `rocprofv3 --kernel-trace --stats` in a run of its own, the program after `--`; pass
`noprobe` as a fourth argument there to keep the probe's launches out of the trace's totals.

  python tools/time_conv.py 6 2.0 512 --fading

Every instance is mid-fade (gas_conv_fade_to) between two IRs of the same length in every call of the run, the fill
included: one 4096-call fade started before the first call.  The multiply-accumulate stage then walks the ring once per
IR (k_conv_mac<true>: twice the reads and twice the partial sums) and the inverse stage is k_conv_inverse_fade.

  python tools/time_conv.py 6 2.0 512 --true-stereo        (combines with --fading)

Every instance gets a four-channel IR of its own (LL, LR, RL, RR).  The multiply-accumulate stage is k_conv_mac_ts: per
instance and output ear it reads 2 k_ir spectra of the rings (both input ears') and 2 k_ir of the IR, twice the
two-channel bytes, and writes the same partial sums."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import godot_audio_spatializer_amd as gas  # noqa: E402

WARMUP, STEPS = 20, 200
RATE = 48000


def chunks(k_ir):  # gas_conv_chunks (gas_internal.h)
    per = max(16, -(-k_ir // 32))
    return -(-k_ir // per)


def main(argv):
    n, seconds, F = int(argv[0]), float(argv[1]), int(argv[2])
    probe = "noprobe" not in argv[3:]
    fading = "--fading" in argv[3:]
    channels = 4 if "--true-stereo" in argv[3:] else 2
    taps = int(round(seconds * RATE))
    k_ir = -(-taps // F)
    assert not fading or WARMUP + STEPS + k_ir <= 4096  # GAS_CONV_MAX_FADE_BLOCKS: the fade outlasts the run
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=4, frames=F, mix_rate=float(RATE))
    ctx.reserve_conv(n, taps)
    env = np.exp(-6.0 * np.arange(taps) / taps)
    convs = [ctx.conv_create(ctx.conv_ir_load((rng.standard_normal((channels, taps)) * env / np.sqrt(taps)).astype(np.float32))) for _ in range(n)]
    if fading:
        for k in convs:
            ctx.conv_fade_to(k, ctx.conv_ir_load((rng.standard_normal((channels, taps)) * env / np.sqrt(taps)).astype(np.float32)), 0.25, 0.75, 4096)
    x = torch.from_numpy(rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)).cuda()
    y = torch.zeros_like(x)
    torch.cuda.synchronize()
    ts = []
    for i in range(WARMUP + STEPS + k_ir):  # the rings fill first: every timed call multiplies real spectra
        t0 = time.perf_counter()
        ctx.conv_process(convs, x, out=y)
        ctx.synchronize()
        t1 = time.perf_counter()
        if i >= WARMUP + k_ir:
            ts.append((t1 - t0) * 1e6)
    out = y.cpu().numpy()
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    sums = 2 if fading else 1  # walks over the ring: one per IR
    rd = sums * n * 2 * (channels // 2) * k_ir * 2 * 4096  # per output ear: ring and IR spectra of every input ear it hears
    wr = sums * n * 2 * chunks(k_ir) * 4096
    res = {"instances": n, "ir_seconds": seconds, "frames": F, "fading": fading, "true_stereo": channels == 4, "taps": taps, "k_ir": k_ir, "steps": STEPS, "mac_read_bytes": rd, "mac_write_bytes": wr, "state_bytes": n * (8192 * k_ir + 4096) + sums * n * channels * k_ir * 4096, "call_us": {"median": round(float(np.median(ts)), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}}
    if probe:
        us = ctx.bandwidth_probe(rd, wr)
        res["probe_us"] = round(us, 2)
        res["probe_GBps"] = round((rd + wr) / us / 1e3, 1)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
