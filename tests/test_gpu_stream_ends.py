"""The three device forms of the source window at stream ends, against tests/stream_window_ref.py (which
test_stream_window_reference.py pins to the oracle's mixer bit for bit):

(a), (b)  k_sample_sources, plain and 16.16 cubic: one [] playback, so the mix is the row -- bitwise, with has_frames and
          gas_stream_positions, over the case table.
(c)       the fused prologues (load_window<true> / bcast_meta<true>) of k_hrtf_uni (no flag), k_hrtf_ols (cross-fade) and
          k_hrtf_ols_blend (interpolate) with several playbacks per wave, against a second context that samples rows
          first and against the oracle's HRTF stage fed the restatement's windows (test_fused_prologues says which
          comparison is bitwise and which has a band).
(d)       gas_process_block_streams(GAS_MEM_DEVICE) against the host form, bitwise.

Sources per wave in (c).  k_hrtf_uni runs min(ceil(n / 8), 256) workgroups of 8 waves (gas_hrtf_uni_partials); k_hrtf_ols
and k_hrtf_ols_blend share 256 workgroups of 8 waves between their frequency-domain and exact-peak groups
(gas_hrtf_plan), each raised only past 64 sources per wave.  With at most 2048 waves whichever way a list splits,
n = 2049 is the first size at which a wave carries two sources in all three forms, so no further size is needed.  A
list shrinks as ended playbacks are gated off: n = 2049 has two per wave in its first callback.  The large sizes keep
lists of 4500 / 3383 / 2643 and 9000 / 6713 / 4360 playbacks (F = 512; much the same at 256) over their three
callbacks: k_hrtf_uni and the all-peaks group of the other two carry up to 3 / 2 / 2 and 5 / 4 / 3 per wave; with
GAS_FLAG_PEAKS_DRAINING_ONLY the frequency-domain group carries up to 4 / 3 / 3 and 8 / 6 / 4 and the exact-peak group
(the ended playbacks) up to 2 / 2 / 2 and 4 / 3 / 2."""
import ctypes as C

import numpy as np
import pytest

import stream_window_ref as wref
from helpers import mix_matches
from test_gpu_stream_loops import rebind

pytestmark = pytest.mark.gpu

GATE = 1e-4  # db_to_linear(-80 dB), audio_spatializer.cpp:465


@pytest.mark.parametrize("F", [128, 256, 384, 512])
@pytest.mark.parametrize("fmt", wref.FORMATS)
def test_rows_bitwise(gas, fmt, F):
    K = gas.capi
    rng = np.random.default_rng(41)
    with gas.SpatializerContext(max_sources=1, frames=F) as ctx:
        slot = ctx.source_alloc(K.KIND_EFFECT)  # empty chain, zero params: the mix is the row
        ctx.params_publish(slot, np.zeros(1, K.PARAMS_DTYPE))
        sid = None
        for n, start in wref.cases(F):
            pcm = wref.make_pcm(rng, n, fmt)
            sid = rebind(ctx, slot, pcm, sid, start=start)
            pb = wref.Playback(pcm, start)
            for cb, row in wref.run_to_end(pb, F):
                got, _, hf = ctx.process_block_streams([slot])
                where = f"len {n} start {start} callback {cb}"
                assert np.array_equal(got[0], row), where
                assert bool(hf[0]) == pb.has_frames and int(ctx.stream_positions(1)[0]) == pb.position, where


RESAMPLED_STARTS = (0, -10)  # the second counted from the end


@pytest.mark.parametrize("F", [128, 512])
@pytest.mark.parametrize("pitch", wref.PITCHES + ["moving"])
def test_resampled_bitwise(gas, pitch, F):
    """Held pitches, the ends of the doppler clamp among them, and one sequence that changes every block, so also in
    the block in which the stream ends (the lookahead is regenerated at the previous block's increment)."""
    K = gas.capi
    rng = np.random.default_rng(42)
    pitch_at = wref.moving_pitch if pitch == "moving" else (lambda cb: pitch)
    with gas.SpatializerContext(max_sources=1, frames=F) as ctx:
        slot = ctx.source_alloc(K.KIND_EFFECT)
        sid = None
        for fmt in ("s16_mono", "f32_stereo"):
            for n in (1, 2, 3, 4, 5, 64, F, 2 * F + 1):
                for start in sorted({max(n + s, 0) if s < 0 else s for s in RESAMPLED_STARTS}):
                    pcm = wref.make_pcm(rng, n, fmt)
                    sid = rebind(ctx, slot, pcm, sid, start=start, resampled=True)
                    pb = wref.Playback(pcm, start, resampled=True)
                    for cb, row in wref.run_to_end(pb, F, pitch_at):
                        p = np.zeros(1, K.PARAMS_DTYPE)
                        p["pitch_scale"] = pitch_at(cb)
                        ctx.params_publish(slot, p)
                        got, _, hf = ctx.process_block_streams([slot])
                        where = f"{fmt} len {n} start {start} callback {cb}"
                        assert np.array_equal(got[0], row), where
                        assert bool(hf[0]) == pb.has_frames and int(ctx.stream_positions(1)[0]) == pb.position, where


def test_resampled_pitch_zero_holds(gas):
    """Increment 0: the playback never ends and its position holds (one block in motion first, so that what is held
    is not the silence in front of the start)."""
    K = gas.capi
    F = 128
    pcm = wref.make_pcm(np.random.default_rng(43), 300, "s16_stereo")
    with gas.SpatializerContext(max_sources=1, frames=F) as ctx:
        slot = ctx.source_alloc(K.KIND_EFFECT)
        rebind(ctx, slot, pcm, None, start=17, resampled=True)
        pb = wref.Playback(pcm, 17, resampled=True)
        for cb, pitch in enumerate((1.0, 0.0, 0.0, 0.0)):
            p = np.zeros(1, K.PARAMS_DTYPE)
            p["pitch_scale"] = pitch
            ctx.params_publish(slot, p)
            got, _, hf = ctx.process_block_streams([slot])
            assert np.array_equal(got[0], pb.block(F, pitch)), cb
            assert hf[0] and pb.has_frames and int(ctx.stream_positions(1)[0]) == pb.position == 17 + F, cb
        assert got.any() and np.all(got[0] == got[0, 0])


# ---- (c) ----

FLAG_NAMES = ["plain", "crossfade", "interpolate"]


def scene(n, F):
    """About two dozen streams of all four formats, lengths from the case table and on to 6 F; n playbacks over them
    whose starts are drawn from the case table's (0, 1, 63, 64, the last frames, clamped) or anywhere in the stream, so
    that in every callback some playbacks end next to list neighbours that continue, have ended, or -- in the first --
    still sit in the silence in front of their start."""
    rng = np.random.default_rng(50 + n + F)
    lens = sorted(set(wref.lengths(F)) | {F + 64, 2 * F + 1, 3 * F, 4 * F, 4 * F + 1, 5 * F - 1, 5 * F, 5 * F + 64, 6 * F - 65, 6 * F})
    pcms = [wref.make_pcm(rng, L, wref.FORMATS[(i + i // 4) % 4]) for i, L in enumerate(lens)]
    which = rng.integers(0, len(pcms), n) if n > 1 else np.array([len(pcms) // 2])
    starts = np.zeros(n, np.int64)
    for i in range(n):
        L = lens[which[i]]
        table = wref.starts(L)
        starts[i] = table[rng.integers(len(table))] if rng.random() < 0.25 else rng.integers(0, L + 1)
    starts[0] = 0
    return pcms, which, starts


class LiveOracle:
    """ob.BatchOracle's HRTF stage over the playbacks still in the list: the per-source states of the live subset are
    handed to gaso_batch_block and taken back.  Large lists are split over threads (the sum is in float64)."""

    def __init__(self, ob, n, F, hrir, crossfade):
        self.ob, self.F = ob, F
        self.o = ob.BatchOracle(ob.KIND_EFFECT, n, F, chain=(ob.FX_HRTF,), hrir=hrir, crossfade=crossfade)
        self.raw = np.frombuffer(self.o.states, np.uint8).reshape(n, C.sizeof(ob.BatchState))

    def _part(self, live, params, windows):
        ob, F, m = self.ob, self.F, len(live)
        sub = np.ascontiguousarray(self.raw[live])
        states = (ob.BatchState * m).from_buffer(sub)
        params = np.ascontiguousarray(params, ob.PARAMS_DTYPE)
        windows = np.ascontiguousarray(windows, np.float32)
        mix, mix64, peaks = np.zeros((1, F, 2), np.float32), np.zeros((1, F, 2), np.float64), np.zeros((m, 2), np.float32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        ob.lib().gaso_batch_block(ob.KIND_EFFECT, 1, vp(params), states, C.byref(self.o.hrtf), vp(windows), m, F, 48000.0, vp(mix), vp(mix64), vp(peaks))
        del states
        self.raw[live] = sub
        return mix64[0], peaks

    def block(self, live, params, windows):
        from concurrent.futures import ThreadPoolExecutor

        parts = np.array_split(np.arange(len(live)), 8 if len(live) >= 512 else 1)
        with ThreadPoolExecutor(len(parts)) as ex:
            out = list(ex.map(lambda k: self._part(live[k], params[k], windows[k]), parts))
        return sum(m for m, _ in out), np.concatenate([p for _, p in out])


_references = {}


def reference(ob, hrir, n, F, xf, callbacks):
    """The composed reference of one (n, F, cross-fade) scene, computed once and shared by the flag variants: per
    callback the live list, the parameters, the float64 mix, every live playback's peak, has_frames and position.  A
    playback leaves the list once it has ended and its peak is at or below the gate (audio_spatializer.cpp:464-469);
    every source moves to another direction in every odd callback.  The last callback is the one in which the last
    playback still playing ends: every callback has frames of a playing stream in its mix, which is what
    helpers.mix_matches' relative measure is made for (see test_fused_prologues)."""
    from godot_audio_spatializer_amd import synth

    key = (n, F, xf, callbacks)
    if key in _references:
        return _references[key]
    pcms, which, starts = scene(n, F)
    floats = [wref.to_float_stereo(p) for p in pcms]
    pbs = [wref.Playback(floats[which[i]], starts[i]) for i in range(n)]
    params = synth.draw_params(np.random.default_rng(60 + n), n, dirs=8)
    oracle = LiveOracle(ob, n, F, hrir, xf)
    live = np.arange(n)
    steps = []
    for cb in range(callbacks):
        if cb % 2 == 1:
            params["hrtf_dir"] = (params["hrtf_dir"] + 1 + cb) % 8
        windows = np.stack([pbs[i].block(F) for i in live])
        hf = np.array([pbs[i].has_frames for i in live])
        mix64, peaks = oracle.block(live, params[live].astype(ob.PARAMS_DTYPE), windows)
        steps.append(dict(live=live, params=params.copy(), mix=mix64, peaks=peaks, hf=hf, pos=np.array([pbs[i].position for i in live])))
        live = live[hf | (peaks.max(axis=1) > GATE)]
        if not hf.any():
            break
    _references[key] = (pcms, which, starts, steps)
    return _references[key]


def band_misses(got, want, rtol=2e-5, atol=1e-7):
    """The entries of got outside |got - want| <= atol + rtol |want| (np.allclose's rule), as (got, want) pairs."""
    bad = ~np.isclose(got, want, rtol=rtol, atol=atol)
    return [(float(g), float(w)) for g, w in zip(got[bad], want[bad])]


def run_fused(gas, ob, monkeypatch, n, F, flags_name, draining, callbacks):
    from godot_audio_spatializer_amd import synth
    from helpers import rel_rms

    K = gas.capi
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=8)
    pcms, which, starts, steps = reference(ob, hrir, n, F, flags_name == "crossfade", callbacks)
    flags = {"plain": 0, "crossfade": K.FLAG_HRTF_CROSSFADE, "interpolate": K.FLAG_HRTF_INTERPOLATE}[flags_name] | (K.FLAG_PEAKS_DRAINING_ONLY if draining else 0)
    bitwise = flags_name != "interpolate"
    misses = []  # the banded comparisons report every miss of a run, with its figures
    with gas.SpatializerContext(max_sources=n, frames=F, flags=flags) as fused:
        monkeypatch.setenv("GAS_STREAM_ROWS_FIRST", "1")  # read at context creation
        with gas.SpatializerContext(max_sources=n, frames=F, flags=flags) as rows:
            monkeypatch.delenv("GAS_STREAM_ROWS_FIRST")
            slots = []
            for ctx in (fused, rows):
                ctx.hrtf_load(hrir)
                sids = [ctx.stream_create(p) for p in pcms]
                s = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
                for i in range(n):
                    ctx.source_bind_stream(s[i], sids[which[i]], start_frame=int(starts[i]))
                slots.append(s)
            for cb, st in enumerate(steps):
                live, ended = st["live"], ~st["hf"]
                if cb == 0 or cb % 2 == 1:  # whenever the directions moved (a publish also makes the host fold its row mirror back)
                    for ctx, s in zip((fused, rows), slots):
                        ctx.params_publish_batch(s, st["params"])
                got, gp, ghf = fused.process_block_streams(slots[0][live])
                want, wp, whf = rows.process_block_streams(slots[1][live])
                where = f"callback {cb}, {len(live)} playbacks"
                assert np.array_equal(ghf, whf) and np.array_equal(ghf, st["hf"]), where
                assert np.array_equal(fused.stream_positions(len(live)), st["pos"]) and np.array_equal(rows.stream_positions(len(live)), st["pos"]), where
                if draining:
                    assert np.all(np.isposinf(gp[~ended])) and np.all(np.isposinf(wp[~ended])), where
                if bitwise:  # the fused prologue hands the kernel the frames the rows-first form reads back from memory
                    assert np.array_equal(got, want), where
                    assert np.array_equal(gp, wp), where
                else:
                    if not mix_matches(got[0], want[0]):
                        misses.append((where, "mix, rows first", rel_rms(got[0], want[0])))
                    fin = np.isfinite(wp)
                    assert np.array_equal(np.isfinite(gp), fin), where
                    misses += [(where, "peak, rows first", m) for m in band_misses(gp[fin], wp[fin])]
                if not mix_matches(got[0], st["mix"]):
                    misses.append((where, "mix, oracle", rel_rms(got[0], st["mix"]), float(np.sqrt(np.mean((got[0] - st["mix"]) ** 2)))))
                checked = ended if draining else np.ones(len(live), bool)
                misses += [(where, "peak, oracle", m) for m in band_misses(gp[checked], st["peaks"][checked])]
    print(f"n {n} F {F} {flags_name}: {len(steps)} callbacks, lists of {[len(s['live']) for s in steps]}, ending or ended {[int((~s['hf']).sum()) for s in steps]}, misses {misses}")
    assert not misses
    return steps


@pytest.mark.parametrize("draining", [False, True], ids=["all_peaks", "draining_only"])
@pytest.mark.parametrize("flags_name", FLAG_NAMES)
@pytest.mark.parametrize("F", [128, 256, 384, 512])
@pytest.mark.parametrize("n", [1, 70, 2049])
def test_fused_prologues(gas, ob, monkeypatch, n, F, flags_name, draining):
    """Every list runs until the callback in which its last playing stream ends; playbacks that ended earlier ring out
    and are gated off on the way, so the list changes in mid-run.

    Against the rows-first context: has_frames and positions equal in all forms.  k_hrtf_uni (no flag) and k_hrtf_ols
    (cross-fade): mix and peaks bitwise.  k_hrtf_ols_blend (interpolate): the band of test_gpu_streams.py
    (helpers.mix_matches, peaks rtol 2e-5 / atol 1e-7) -- its stream-sampling and its float-row instantiation agree
    bit for bit at F = 384 and 512 and differ in the last bits (relative 1e-7, from the first callback on, a single
    playing stream enough) at F = 128 and 256.  k_hrtf_ols.hip fixes no contraction, so each instantiation's products
    and sums are fused as the compiler finds them (built with contraction off, the two agree bit for bit at every F);
    k_hrtf_uni.hip writes its FMAs out, which is why its claim holds.
    Against the oracle's HRTF stage (hrtf.crossfade = 1 for cross-fade, what test_oracle_mixer.Rig sets), fed the
    restatement's windows: helpers.mix_matches on the float64 mix, peaks within rtol 2e-5 / atol 1e-7 -- of every
    playback, or with GAS_FLAG_PEAKS_DRAINING_ONLY of the ended ones, the others reporting +inf.

    This test found the transforms taking in history that no kept output needs (hrtf_dead_regs in gas_hrtf_wave.h): at
    n = 2049, F = 128 two ended playbacks whose output is an exact 0 reported peaks of 1.30e-7 and 1.03e-7, outside atol
    1e-7, from the rounding of full-scale input three callbacks old; those registers now enter as zeros.

    Not compared: callbacks after the last stream's end, in which only HRIR tails of ended playbacks ring out and a
    relative measure of the mix means little (before that change: mix values around 3e-4 with errors of 1e-8 .. 7e-8 per
    frame at F = 128 and 256, above mix_matches' absolute floor of 1e-8 RMS, fused and rows-first bit-equal)."""
    steps = run_fused(gas, ob, monkeypatch, n, F, flags_name, draining, callbacks=40)
    assert not steps[-1]["hf"].any() and all(s["hf"].any() for s in steps[:-1])  # ran to the last end
    assert sum(int((~s["hf"]).sum()) for s in steps) > 0
    if n > 1:
        assert len({len(s["live"]) for s in steps}) > 2  # the list changed in mid-run


@pytest.mark.parametrize("draining", [False, True], ids=["all_peaks", "draining_only"])
@pytest.mark.parametrize("flags_name", FLAG_NAMES)
@pytest.mark.parametrize("F", [256, 512])
@pytest.mark.parametrize("n", [4500, 9000])
def test_fused_prologues_many_per_wave(gas, ob, monkeypatch, n, F, flags_name, draining):
    """Several playbacks in every wave; three callbacks, so that the CPU oracle stays within seconds -- the scene's
    starts put ends into each of them."""
    steps = run_fused(gas, ob, monkeypatch, n, F, flags_name, draining, callbacks=3)
    assert len(steps) == 3 and all(len(s["live"]) > 2048 for s in steps)  # more playbacks than waves throughout
    assert all(min((~s["hf"]).sum(), s["hf"].sum()) > 512 for s in steps)  # ended and continuing side by side


def test_device_memory_form(gas):
    """gas_process_block_streams(GAS_MEM_DEVICE) writes the mix and the peaks of the host form, bit for bit."""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F = 70, 256
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=8)
    pcms, which, starts = scene(n, F)
    params = synth.draw_params(np.random.default_rng(3), n, dirs=8)
    with gas.SpatializerContext(max_sources=n, frames=F) as host, gas.SpatializerContext(max_sources=n, frames=F) as dev:
        slots = []
        for ctx in (host, dev):
            ctx.hrtf_load(hrir)
            sids = [ctx.stream_create(p) for p in pcms]
            s = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
            ctx.params_publish_batch(s, params)
            for i in range(n):
                ctx.source_bind_stream(s[i], sids[which[i]], start_frame=int(starts[i]))
            slots.append(s)
        d_out = torch.full((1, F, 2), float("nan"), device="cuda")
        d_pk = torch.zeros(n, 2, device="cuda")
        torch.cuda.synchronize()
        ended, heard = False, 0
        for cb in range(8):
            want, wp, whf = host.process_block_streams(slots[0])
            hf = np.full(n, 7, np.uint8)
            s32 = np.ascontiguousarray(slots[1], np.uint32)
            rc = dev.lib.gas_process_block_streams(dev.h, s32.ctypes.data_as(C.c_void_p), n, F, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_pk.data_ptr()), hf.ctypes.data_as(C.c_void_p), K.MEM_DEVICE)
            assert rc == 0
            dev.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), want), cb
            heard += bool(want.any())
            assert np.array_equal(d_pk.cpu().numpy(), wp), cb
            assert np.array_equal(hf.astype(bool), whf), cb
            ended = ended or not whf.all()
        assert ended and heard >= 6 and not whf.any()
