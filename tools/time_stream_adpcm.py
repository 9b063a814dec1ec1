"""Dev aid: what GAS_PCM_IMA_ADPCM and GAS_PCM_QOA streams cost per callback, 8192 mono playbacks with [HRTF] chains x 512
frames, all through the rows-first route (the route a list with a compressed playback takes):

  s16            GAS_PCM_S16 with GAS_STREAM_ROWS_FIRST=1: k_sample_sources, then the row form of the HRTF kernel.  Run
                 it against the parent commit's library as well (GAS_AMD_LIB=<that build>, --s16-only): the two figures
                 show what k_sample_sources' early exit on compressed rows costs the uncompressed formats.
  adpcm_span     the same audio as IMA-ADPCM, k_sample_adpcm.hip's span decode (the default)
  adpcm_perload  ... with GAS_ADPCM_SPAN=0: every load decodes from its checkpoint
  qoa_span       a QOA file of random slices, k_sample_qoa.hip's span decode (the default)
  qoa_perload    ... with GAS_QOA_SPAN=0: every load decodes from its record

Every callback is timed by its own pair of events on the GPU timeline; a figure is the median over the callbacks of one
repeat, and the line shows the median, smallest and largest of REPEATS repeats -- the spread to judge a difference by.
The streams are long enough not to end.

  python tools/time_stream_adpcm.py [--s16-only | --cases=s16,adpcm_span,...] [n]"""
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
REPEATS = 5
WARMUP, STEPS = 10, 100


def random_qoa_file(rng, frames):
    """A mono QOA file (include/gas_amd.h) of random slices under random state in every frame header: the decoder's work
    does not depend on the values."""
    out = [b"qoaf" + int(frames).to_bytes(4, "big")]
    for at in range(0, frames, 5120):
        fsamples = min(5120, frames - at)
        slices = (fsamples + 19) // 20
        out.append(bytes([1, 0, 0xBB, 0x80]) + fsamples.to_bytes(2, "big") + (8 + 16 + 8 * slices).to_bytes(2, "big"))
        out.append(rng.integers(0, 256, 16 + 8 * slices).astype(np.uint8).tobytes())
    return np.frombuffer(b"".join(out), np.uint8)


def callback_us(n, case, frames=512, dirs=64):
    os.environ["GAS_STREAM_ROWS_FIRST"] = "1"
    os.environ["GAS_ADPCM_SPAN"] = "0" if case == "adpcm_perload" else "1"
    os.environ["GAS_QOA_SPAN"] = "0" if case == "qoa_perload" else "1"
    rng = np.random.default_rng(0)
    ctx = gas.SpatializerContext(max_sources=n, frames=frames, flags=K.FLAG_PEAKS_DRAINING_ONLY)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.hrtf_load(synth.synthetic_hrir(np.random.default_rng(7), dirs=dirs))
    slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
    ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=dirs, frames=frames))
    length = (WARMUP + REPEATS * STEPS + 2) * frames + 4096
    sids = []
    for i in range(16):  # a few streams shared by all playbacks, every playback at its own start
        if case == "s16":
            sids.append(ctx.stream_create((rng.uniform(-0.5, 0.5, length) * 32767).astype(np.int16)))
        elif case.startswith("qoa"):
            sids.append(ctx.stream_create(random_qoa_file(rng, length), K.PCM_QOA, 1, length))
        else:  # random codes: the decoder's work does not depend on the values
            sids.append(ctx.stream_create(rng.integers(0, 256, (length + 1) // 2).astype(np.uint8), K.PCM_IMA_ADPCM, 1, length))
    for i, s in enumerate(slots):
        ctx.source_bind_stream(s, sids[i % len(sids)], start_frame=int(rng.integers(0, 4096)))
    out = torch.zeros(1, frames, 2, device="cuda")
    pk = torch.zeros(n, 2, device="cuda")
    sl = np.ascontiguousarray(slots, dtype=np.uint32)
    ptr = sl.ctypes.data_as(C.c_void_p)

    def callback():
        rc = ctx.lib.gas_process_block_streams(ctx.h, ptr, n, frames, C.c_void_p(out.data_ptr()), C.c_void_p(pk.data_ptr()), None, K.MEM_DEVICE)
        assert rc == 0, rc

    for _ in range(WARMUP):
        callback()
    torch.cuda.synchronize()
    got = []
    for _ in range(REPEATS):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
        for e0, e1 in ev:
            e0.record()
            callback()
            e1.record()
        torch.cuda.synchronize()
        got.append(float(np.median([1e3 * e0.elapsed_time(e1) for e0, e1 in ev])))
    ctx.close()
    return np.array(got)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 8192
    cases = ["s16"]
    if "--s16-only" not in sys.argv:
        cases += ["adpcm_span", "adpcm_perload", "qoa_span", "qoa_perload"]
    for a in sys.argv[1:]:
        if a.startswith("--cases="):  # a library without GAS_PCM_QOA: --cases=s16,adpcm_span
            cases = a[len("--cases="):].split(",")
    for case in cases:
        us = callback_us(n, case)
        print(json.dumps({"n": n, "case": case, "lib": os.environ.get("GAS_AMD_LIB", "in-tree"), "callback_us_median": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}), flush=True)


if __name__ == "__main__":
    main()
