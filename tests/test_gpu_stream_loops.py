"""gas_stream_set_loop (NEW, include/gas_amd.h): a looped device-resident stream in one context and its unrolled copy
(tests/stream_loop_ref.py) as an ordinary stream in a second context give the same callbacks, as long as the copy is
long enough that its end is never approached: start + callbacks * F * max_pitch + 64 + 4 + F frames.  That pins the
loops to the plain stream path, which test_gpu_streams.py holds against the oracle.

gas_process_block_buses has no stream form (it takes float rows), so there is no looped case of it here."""
import numpy as np
import pytest

import hrtf_blend_fade_ref as fref
import stream_loop_ref as lref
from helpers import mix_matches
from test_oracle_mixer import Rig

pytestmark = pytest.mark.gpu

MODES = [lref.LOOP_FORWARD, lref.LOOP_PINGPONG]
FORMATS = ["s16_mono", "s16_stereo", "f32_mono", "f32_stereo"]


def make_pcm(rng, frames, fmt):
    shape = (frames,) if fmt.endswith("mono") else (frames, 2)
    x = rng.uniform(-0.5, 0.5, shape)
    return (x * 32767).astype(np.int16) if fmt.startswith("s16") else x.astype(np.float32)


def to_float_stereo(pcm):
    f = pcm.astype(np.float32) / np.float32(32768.0) if pcm.dtype == np.int16 else pcm
    return np.stack([f, f], axis=1) if pcm.ndim == 1 else f


def unrolled_len(start, callbacks, F, max_pitch=1.0):
    return int(start + callbacks * F * max_pitch + 64 + 4 + F)


def rebind(ctx, slot, pcm, old, mode=lref.LOOP_DISABLED, b=0, e=0, start=0, resampled=False):
    """A fresh stream for the slot's next playback; the one it played before is destroyed once nothing is bound to it."""
    sid = ctx.stream_create(pcm)
    if resampled:
        ctx.stream_set_resampled(sid, True)
    if mode != lref.LOOP_DISABLED:
        ctx.stream_set_loop(sid, mode, b, e)
    ctx.source_bind_stream(slot, sid, start_frame=start)
    if old is not None:
        ctx.stream_destroy(old)
    return sid


def loop_cases():
    """(L, b, tail, start): seams in the lookahead, mid-row and many times per row; starts at 0, inside the loop and at
    or past loop_end on the unrolled timeline."""
    for L in (1, 37, 64, 100, 511, 513, 1500):
        for b in (0, 123):
            for tail in (0, 200):
                for start in (0, b + L // 2, b + L + 300):
                    yield L, b, tail, start


@pytest.mark.parametrize("F", [512, 256])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_bitwise(gas, fmt, mode, F):
    K = gas.capi
    rng = np.random.default_rng(11)
    callbacks = 6
    with gas.SpatializerContext(max_sources=1, frames=F) as lc, gas.SpatializerContext(max_sources=1, frames=F) as uc:
        slots = []
        for ctx in (lc, uc):
            slots.append(ctx.source_alloc(K.KIND_EFFECT))  # empty chain, zero params: the mix is the row
            ctx.params_publish(slots[-1], np.zeros(1, K.PARAMS_DTYPE))
        lsid = usid = None
        for L, b, tail, start in loop_cases():
            e = b + L
            pcm = make_pcm(rng, e + tail, fmt)
            lsid = rebind(lc, slots[0], pcm, lsid, mode, b, 0 if tail == 0 else e, start)
            usid = rebind(uc, slots[1], lref.unroll(pcm, b, e, mode, unrolled_len(start, callbacks, F)), usid, start=start)
            for cb in range(callbacks):
                got, gp, ghf = lc.process_block_streams([slots[0]])
                want, wp, whf = uc.process_block_streams([slots[1]])
                where = f"L {L} b {b} tail {tail} start {start} callback {cb}"
                assert np.array_equal(got, want), where
                assert np.array_equal(gp, wp) and np.array_equal(ghf, whf) and ghf[0], where
            assert got.any(), (L, b, tail, start)


@pytest.mark.parametrize("pitch", [0.5, 0.97, 1.0, 1.06, 2.0, "moving"])
def test_resampled_bitwise(gas, pitch):
    """Held pitches, and one that changes every block: the lookahead regenerated at the previous increment crosses seams."""
    K = gas.capi
    rng = np.random.default_rng(12)
    F, callbacks = 512, 8
    pitches = [pitch] * callbacks if pitch != "moving" else [1.0 + 0.4 * np.sin(1.0 + cb) for cb in range(callbacks)]
    with gas.SpatializerContext(max_sources=1, frames=F) as lc, gas.SpatializerContext(max_sources=1, frames=F) as uc:
        slots = [ctx.source_alloc(K.KIND_EFFECT) for ctx in (lc, uc)]
        lsid = usid = None
        for fmt in ("s16_mono", "f32_stereo"):
            for mode in MODES:
                for L in (2, 37, 513):
                    for b, tail, start in ((0, 0, 0), (123, 200, 123 + L + 50)):
                        e = b + L
                        pcm = make_pcm(rng, e + tail, fmt)
                        lsid = rebind(lc, slots[0], pcm, lsid, mode, b, e, start, resampled=True)
                        usid = rebind(uc, slots[1], lref.unroll(pcm, b, e, mode, unrolled_len(start, callbacks, F, max(pitches))), usid, start=start, resampled=True)
                        for cb in range(callbacks):
                            p = np.zeros(1, K.PARAMS_DTYPE)
                            p["pitch_scale"] = pitches[cb]
                            lc.params_publish(slots[0], p)
                            uc.params_publish(slots[1], p)
                            got, gp, ghf = lc.process_block_streams([slots[0]])
                            want, wp, whf = uc.process_block_streams([slots[1]])
                            where = f"{fmt} mode {mode} L {L} b {b} start {start} callback {cb}"
                            assert np.array_equal(got, want), where
                            assert np.array_equal(gp, wp) and np.array_equal(ghf, whf) and ghf[0], where
                        assert got.any()


class MovedDirectionFade:
    """hrtf_blend_fade_ref.py's composition for sources without a published blend row (effective row {hrtf_dir, 1}), in
    batched form: y = t * Y_new + (1 - t) * Y_old per source with the same ramp for all, and Y_old = Y_new for a source
    whose direction stayed, so the mix is t * mix(new directions) + (1 - t) * mix(previous directions).  The HRTF stage's
    carried state does not depend on the direction (that reference's premise), so two batched oracles fed the same
    windows stay in step.  Sums and lerp in float64, t in float32 as include/gas_amd.h states it."""

    def __init__(self, ob, n, frames, hrir):
        self.ob = ob
        self.new, self.old = (ob.BatchOracle(ob.KIND_EFFECT, n, frames, chain=(ob.FX_HRTF,), hrir=hrir) for _ in range(2))
        self.t, self.one_t = (x.astype(np.float64)[:, None] for x in fref.ramp(frames))
        self.prev = None

    def block(self, params, src):
        p = np.ascontiguousarray(params).astype(self.ob.PARAMS_DTYPE)
        q = p.copy()
        if self.prev is not None:
            q["hrtf_dir"] = self.prev
        new64 = self.new.block(p, src, want64=True)[2][0]
        old64 = self.old.block(q, src, want64=True)[2][0]
        self.prev = p["hrtf_dir"].copy()
        return self.t * new64 + self.one_t * old64


HRTF_FLAGS = ["plain", "crossfade", "interpolate", "blend_fade"]


@pytest.mark.parametrize("flags_name", HRTF_FLAGS)
@pytest.mark.parametrize("n", [1, 5, 70, 600])
def test_fused_hrtf(gas, ob, n, flags_name):
    """Plain [HRTF] playbacks, looped and unlooped streams in one list.  The fused prologue maps the looped indices
    itself, so both contexts take the same kernel form and agree bit for bit -- except with GAS_FLAG_HRTF_CROSSFADE,
    where lists with a looped playback sample rows first while the unrolled context stays fused: there
    helpers.mix_matches and the peak band of test_gpu_streams.py apply.  GAS_FLAG_HRTF_BLEND_FADE samples rows first in
    both.  The oracle's mixer, fed the unrolled floats, checks every variant; under GAS_FLAG_HRTF_BLEND_FADE a source
    whose direction moved is rendered with the old and the new direction and lerped across the block, which the mixer
    does not restate, so there the oracle's renders are composed as hrtf_blend_fade_ref.py composes them
    (MovedDirectionFade) and fed the same unrolled floats behind the 64-frame lookahead."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    rng = np.random.default_rng(21 + n)
    F, callbacks = 512, 6
    flags = {"plain": 0, "crossfade": K.FLAG_HRTF_CROSSFADE, "interpolate": K.FLAG_HRTF_INTERPOLATE, "blend_fade": K.FLAG_HRTF_INTERPOLATE | K.FLAG_HRTF_BLEND_FADE}[flags_name]
    xf = flags_name == "crossfade"
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=8)
    # a handful of streams, many playbacks at different starts: (pcm, mode, b, e)
    configs = [(make_pcm(rng, 4000, "s16_mono"), lref.LOOP_DISABLED, 0, 0)]
    for i, (L, mode) in enumerate((L, mode) for L in (37, 100, 1500) for mode in MODES):
        b = (0, 123)[i % 2]
        configs.append((make_pcm(rng, b + L + (0, 200)[(i // 2) % 2], FORMATS[i % 4]), mode, b, b + L))
    which = [(i + 1) % len(configs) if n > 1 else 1 for i in range(n)]
    starts = [int(rng.integers(0, 400)) for _ in range(n)]
    starts[0] = 0
    params = synth.draw_params(rng, n, dirs=8)
    with gas.SpatializerContext(max_sources=n, frames=F, flags=flags) as lc, gas.SpatializerContext(max_sources=n, frames=F, flags=flags) as uc:
        lsids, usids, floats = [], [], []
        for pcm, mode, b, e in configs:
            sid = lc.stream_create(pcm)
            if mode != lref.LOOP_DISABLED:
                lc.stream_set_loop(sid, mode, b, e)
                assert lc.stream_get_loop(sid) == (mode, b, e)
            lsids.append(sid)
            u = lref.unroll(pcm, b, e, mode, unrolled_len(400, callbacks, F))
            usids.append(uc.stream_create(u))
            floats.append(to_float_stereo(u))
        slots = []
        for ctx, sids in ((lc, lsids), (uc, usids)):
            ctx.hrtf_load(hrir)
            s = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
            ctx.params_publish_batch(s, params)
            for i in range(n):
                ctx.source_bind_stream(s[i], sids[which[i]], start_frame=starts[i])
            slots.append(s)
        fed = [floats[which[i]][starts[i]:] for i in range(n)]
        composed = None
        if flags_name == "blend_fade":
            composed = MovedDirectionFade(ob, n, F, hrir)
            fed = [np.concatenate([np.zeros((64, 2), np.float32), f]) for f in fed]  # the window the DSP sees
        else:
            rig = Rig(ob, ob.KIND_EFFECT, fed, F, chain=(ob.FX_HRTF,), hrir=hrir)
            if xf:
                rig.hrtf.crossfade = 1
            rig.params[:] = params.astype(ob.PARAMS_DTYPE)
        for cb in range(callbacks):
            if cb % 2 == 1:  # move every source
                params["hrtf_dir"] = (params["hrtf_dir"] + 1 + cb) % 8
                for ctx, s in zip((lc, uc), slots):
                    ctx.params_publish_batch(s, params)
                if composed is None:
                    rig.params[:] = params.astype(ob.PARAMS_DTYPE)
            got, gp, ghf = lc.process_block_streams(slots[0])
            want, wp, whf = uc.process_block_streams(slots[1])
            if composed is None:
                rc, oracle = rig.get_mixed_frames(0)
                assert rc == 0
            else:
                oracle = composed.block(params, np.stack([f[cb * F:(cb + 1) * F] for f in fed]))
            assert ghf.all() and whf.all(), cb
            if xf:
                assert mix_matches(got[0], want[0]), f"callback {cb}"
                np.testing.assert_allclose(gp, wp, rtol=2e-5, atol=1e-7)
            else:
                assert np.array_equal(got, want), f"callback {cb}"
                assert np.array_equal(gp, wp), f"callback {cb}"
            assert mix_matches(got[0], oracle), f"oracle, callback {cb}"


def test_never_ends(gas):
    K = gas.capi
    F = 512
    rng = np.random.default_rng(5)
    pcm = make_pcm(rng, 700, "s16_mono")
    with gas.SpatializerContext(max_sources=2, frames=F) as ctx, gas.SpatializerContext(max_sources=1, frames=F) as solo:
        looped, plain = ctx.stream_create(pcm), ctx.stream_create(pcm)
        ctx.stream_set_loop(looped, K.LOOP_FORWARD)
        a, b = ctx.source_alloc(K.KIND_EFFECT), ctx.source_alloc(K.KIND_EFFECT)
        for s in (a, b):
            ctx.params_publish(s, np.zeros(1, K.PARAMS_DTYPE))
        ctx.source_bind_stream(a, looped)
        ctx.source_bind_stream(b, plain)
        # the unlooped playback alone, as before
        s0 = solo.source_alloc(K.KIND_EFFECT)
        solo.params_publish(s0, np.zeros(1, K.PARAMS_DTYPE))
        solo.source_bind_stream(s0, solo.stream_create(pcm))
        u = to_float_stereo(lref.unroll(pcm, 0, 700, lref.LOOP_FORWARD, 21 * F))
        delayed = np.concatenate([np.zeros((64, 2), np.float32), u])
        for cb in range(20):
            mix, _, hf = ctx.process_block_streams([a, b])
            alone, _, hf0 = solo.process_block_streams([s0])
            assert hf[0] == 1 and hf[1] == hf0[0] == (cb == 0), cb  # 700 frames end in the second callback
            row = delayed[cb * F:(cb + 1) * F]
            assert row.any()
            # zero params copy each row into the mix: what is left after the unlooped playback's part is the loop
            np.testing.assert_allclose(mix[0] - alone[0], row, rtol=0, atol=2e-7, err_msg=f"callback {cb}")
            if cb >= 3:
                assert not alone.any() and np.array_equal(mix[0], row)  # the unlooped one ended, faded and is silent
        with pytest.raises(gas.GasError):
            ctx.stream_destroy(looped)  # still bound
        ctx.source_set_draining(a, True)
        ctx.source_free(a)
        ctx.source_free(b)
        ctx.process_block_streams([])  # block boundary: the frees take effect
        ctx.stream_destroy(looped)
        ctx.stream_destroy(plain)


@pytest.mark.parametrize("resampled", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_positions(gas, mode, resampled):
    K = gas.capi
    F = 512
    b, e, start = 123, 123 + 700, 40
    with gas.SpatializerContext(max_sources=1, frames=F) as ctx:
        sid = ctx.stream_create(make_pcm(np.random.default_rng(2), 1000, "s16_stereo"))
        if resampled:
            ctx.stream_set_resampled(sid, True)
        ctx.stream_set_loop(sid, mode, b, e)
        slot = ctx.source_alloc(K.KIND_EFFECT)
        p = np.zeros(1, K.PARAMS_DTYPE)
        p["pitch_scale"] = 1.5 if resampled else 1.0
        ctx.params_publish(slot, p)
        ctx.source_bind_stream(slot, sid, start_frame=start)
        inc = int(1.5 * 65536) if resampled else 65536
        for cb in range(10):
            ctx.process_block_streams([slot])
            consumed = ((start << 16) + (cb + 1) * F * inc) >> 16
            assert int(ctx.stream_positions(1)[0]) == int(lref.loop_map(consumed, b, e, mode)), cb


def test_refusals_and_lifecycle(gas):
    K = gas.capi
    F = 512
    rng = np.random.default_rng(8)
    pcm = make_pcm(rng, 2000, "f32_mono")
    with gas.SpatializerContext(max_sources=1, frames=F) as ctx:
        sid = ctx.stream_create(pcm)
        assert ctx.stream_get_loop(sid) == (K.LOOP_DISABLED, 0, 0)
        ctx.stream_set_loop(sid, K.LOOP_PINGPONG, 10, 1000)
        for args in ((3, 0, 0), (-1, 0, 0), (K.LOOP_FORWARD, 500, 500), (K.LOOP_FORWARD, 600, 500), (K.LOOP_FORWARD, 0, 2001), (K.LOOP_PINGPONG, 2000, 0)):
            with pytest.raises(gas.GasError) as ei:
                ctx.stream_set_loop(sid, *args)
            assert ei.value.status == -1, args  # GAS_ERR_INVALID_ARGUMENT
            assert ctx.stream_get_loop(sid) == (K.LOOP_PINGPONG, 10, 1000)  # nothing of a refused call is taken
        for call in (lambda: ctx.stream_set_loop(77, K.LOOP_FORWARD), lambda: ctx.stream_get_loop(77)):
            with pytest.raises(gas.GasError) as ei:
                call()
            assert ei.value.status == -3  # GAS_ERR_BAD_SLOT
        ctx.stream_set_loop(sid, K.LOOP_FORWARD)  # loop_end 0 = the stream's length
        assert ctx.stream_get_loop(sid) == (K.LOOP_FORWARD, 0, 2000)
        ctx.stream_set_loop(sid, K.LOOP_DISABLED, 5, 3)  # ignores the other two arguments
        assert ctx.stream_get_loop(sid) == (K.LOOP_DISABLED, 0, 0)
        slot = ctx.source_alloc(K.KIND_EFFECT)
        ctx.params_publish(slot, np.zeros(1, K.PARAMS_DTYPE))
        ctx.source_bind_stream(slot, sid, start_frame=5000)  # DISABLED: today's behaviour, the start clamps to the end
        mix, _, hf = ctx.process_block_streams([slot])
        assert not hf[0] and not mix.any()
        with pytest.raises(gas.GasError) as ei:
            ctx.stream_set_loop(sid, K.LOOP_FORWARD)  # bound
        assert ei.value.status == -1
        # a looped playback, re-bound: zeroed lookahead, the start honoured
        lsid = ctx.stream_create(pcm)
        ctx.stream_set_loop(lsid, K.LOOP_FORWARD, 100, 300)
        u = lref.unroll(pcm, 100, 300, lref.LOOP_FORWARD, 4000)
        for start in (0, 1234):
            ctx.source_bind_stream(slot, lsid, start_frame=start)
            mix, _, hf = ctx.process_block_streams([slot])
            assert hf[0] and not mix[0, :64].any()
            np.testing.assert_array_equal(mix[0, 64:, 0], u[start:start + F - 64])
            mix, _, _ = ctx.process_block_streams([slot])
            np.testing.assert_array_equal(mix[0, :, 1], u[start + F - 64:start + 2 * F - 64])
        # the slot recycled from a looped to an unlooped stream behaves as fresh
        ctx.source_free(slot)
        ctx.process_block_streams([])
        again = ctx.source_alloc(K.KIND_EFFECT)
        assert again == slot
        ctx.params_publish(again, np.zeros(1, K.PARAMS_DTYPE))
        mix, _, hf = ctx.process_block_streams([again])
        assert not hf[0] and not mix.any()  # nothing bound, no stale cursor
        short = ctx.stream_create(pcm[:600])
        ctx.source_bind_stream(again, short)
        mix, _, hf = ctx.process_block_streams([again])
        assert hf[0]
        np.testing.assert_array_equal(mix[0, 64:, 0], pcm[:F - 64])
        mix, _, hf = ctx.process_block_streams([again])
        assert not hf[0] and not mix[0, 88 + 64:].any()  # ends and fades at frame 600, no wrap


def test_two_contexts_agree(gas):
    """Determinism: the same looped [HRTF] list in two contexts, bit for bit."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, n = 512, 9
    rng = np.random.default_rng(4)
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=8)
    pcms = [make_pcm(rng, 300 + 97 * i, FORMATS[i % 4]) for i in range(n)]
    params = synth.draw_params(rng, n, dirs=8)
    outs = []
    for _ in range(2):
        with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
            ctx.hrtf_load(hrir)
            slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
            ctx.params_publish_batch(slots, params)
            for i in range(n):
                sid = ctx.stream_create(pcms[i])
                ctx.stream_set_loop(sid, MODES[i % 2], 7 * i, 0)
                ctx.source_bind_stream(slots[i], sid, start_frame=50 * i)
            outs.append([ctx.process_block_streams(slots)[:2] for _ in range(5)])
    for (m0, p0), (m1, p1) in zip(*outs):
        assert np.array_equal(m0, m1) and np.array_equal(p0, p1) and m0.any()


def test_host_layer(gas):
    """A looped device-stream playback through the host layer stays active, reports wrapped positions and is reaped
    after stop."""
    K = gas.capi
    F = 512
    b, e = 100, 700
    rng = np.random.default_rng(6)
    pcm = make_pcm(rng, 900, "s16_stereo")
    params = np.zeros(1, K.PARAMS_DTYPE)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, ())
        sid = ctx.stream_create(pcm)
        ctx.stream_set_loop(sid, K.LOOP_PINGPONG, b, e)
        pid = host.start_playback_device_stream(sid, start_frame=30)
        host.set_spatializer_parameters(pid, params[0])
        delayed = np.concatenate([np.zeros((64, 2), np.float32), to_float_stereo(lref.unroll(pcm, b, e, lref.LOOP_PINGPONG, 30 + 21 * F))[30:]])
        for cb in range(20):
            rc, got = host.get_mixed_frames(0, F)
            assert rc == 0 and np.array_equal(got, delayed[cb * F:(cb + 1) * F]), cb
            assert host.is_playback_active(pid)
            assert host.get_playback_position(pid) == int(lref.loop_map(30 + (cb + 1) * F, b, e, lref.LOOP_PINGPONG)), cb
        assert host.playback_count() == 1
        host.stop_playback(pid)
        for _ in range(2):
            rc, got = host.get_mixed_frames(0, F)
            assert rc == 0 and not got.any()
        assert not host.is_playback_active(pid) and host.playback_count() == 0  # reaped
        host.close()
