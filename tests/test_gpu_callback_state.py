"""A rejected callback leaves nothing behind for the next one.

Every callback entry of include/gas_amd.h validates on the host before its first launch.  Two contexts are set up
alike (configuration, slots, parameters, HRIR table, streams) and fed the same inputs.  Context A runs a sequence of
valid callbacks; context B runs the same sequence with rejected calls in front of the valid ones: a wrong frame count
(GAS_ERR_FRAME_COUNT), an unused slot (GAS_ERR_BAD_SLOT), a slot twice (GAS_ERR_INVALID_ARGUMENT) and, where the
entry has one, a list it does not support (GAS_ERR_UNSUPPORTED_CHAIN).  Every valid callback's mix and peaks -- and for
the stream entries has_frames and gas_stream_positions -- are then bit-equal between A and B.

All legs run at frames = 128 (the smallest k_hrtf_uni takes), one channel pair, 16 HRIR directions.  The valid calls
pass their slot list explicitly, with one exception: the callbacks of the batched leg that consume device-published
parameter rows or join a batch must reuse the previous list (slots == NULL is what selects both paths), and a rejected
list invalidates that list by contract -- so there B interleaves only the rejection that comes before the list is
looked at (the frame count), and the other rejections come in front of the callbacks that pass their list."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, DIRS = 128, 16
INVALID_ARGUMENT, BAD_SLOT, FRAME_COUNT, UNSUPPORTED_CHAIN = -1, -3, -4, -6


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def u32(slots):
    return np.ascontiguousarray(slots, np.uint32)


def hrir16():
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(7), dirs=DIRS)


def unused_slot(ctx_sources, taken):
    return next(s for s in range(ctx_sources) if s not in set(int(t) for t in taken))


def both(leg, gas):
    """Runs `leg(gas, fail)` for context A (fail False) and context B (fail True); the steps must be bit-equal."""
    a, b = leg(gas, False), leg(gas, True)
    assert len(a) == len(b) and len(a) > 0
    for t, (sa, sb) in enumerate(zip(a, b)):
        assert sa.keys() == sb.keys()
        for what in sa:
            assert np.array_equal(sa[what], sb[what]), f"{what}, valid callback {t}"
    return a


# ---- 1, 2: gas_process_block, device memory ----


def block_leg(gas, fail, n, flags, plan):
    """plan: per valid callback (explicit list?, device publish in front of it?, read the profile behind it?).  Rejected
    calls (B) come in front of every callback: the frame count always, the bad lists only where the callback passes its
    own list.  (Reading the profile runs whatever still waits for its batch, so the plan reads only where nothing does.)"""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    rng = np.random.default_rng(11)
    T = len(plan)
    ctx = gas.SpatializerContext(max_sources=n + 4, frames=F, flags=flags)
    try:
        ctx.hrtf_load(hrir16())
        ctx.set_batch_depth(2)
        slots = u32(ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,)))
        ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=DIRS, frames=F))
        free = unused_slot(n + 4, slots)
        srcs = [torch.from_numpy(synth.draw_sources(rng, n, F)).cuda() for _ in range(T)]
        pubs = [torch.from_numpy(synth.draw_params(rng, n, dirs=DIRS, frames=F).view(np.uint8).reshape(n, -1).copy()).cuda() for _ in range(T)]
        outs = torch.full((T, 1, F, 2), float("nan"), device="cuda")
        peaks = torch.zeros(T, n, 2, device="cuda")
        scratch = torch.zeros(1, F, 2, device="cuda")
        torch.cuda.synchronize()
        ctx.profile_enable(1)
        ctx.profile_read(reset=True)
        kernels = []
        for t, (explicit, publish, read) in enumerate(plan):
            if publish:
                ctx.params_publish_device(pubs[t].data_ptr(), n)
            if fail:
                call = lambda s, frames: ctx.process_block_raw(srcs[t].data_ptr(), s, len(s), frames, scratch.data_ptr(), 0, K.MEM_DEVICE)  # noqa: E731
                assert call(slots, F // 2) == FRAME_COUNT
                if explicit:
                    assert call(np.concatenate([slots[:-1], u32([free])]), F) == BAD_SLOT
                    assert call(np.concatenate([slots[:-1], slots[:1]]), F) == INVALID_ARGUMENT
            assert ctx.process_block_raw(srcs[t].data_ptr(), slots if explicit else None, n, F, outs[t].data_ptr(), peaks[t].data_ptr(), K.MEM_DEVICE) == 0
            if read:
                kernels.append(ctx.profile_read(reset=True)["kernel"])
        ctx.join_outputs()
        ctx.synchronize()
        res, pk = outs.cpu().numpy(), peaks.cpu().numpy()
        assert not np.isnan(res).any() and all(res[t].any() for t in range(T))
        return [{"mix": res[t], "peaks": pk[t]} for t in range(T)], kernels
    finally:
        ctx.close()


def test_process_block_pipelined(gas):
    """16 plain-[HRTF] sources, GAS_FLAG_PIPELINED_MIX: the sum of a callback waits for the next one (or the join)."""
    K = gas.capi
    both(lambda g, fail: block_leg(g, fail, 16, K.FLAG_PIPELINED_MIX, [(True, False, False)] * 4)[0], gas)


def test_process_block_batched_with_device_published_rows(gas):
    """GAS_FLAG_BATCHED_LAUNCH at depth 2 over 128 sources: gas_hrtf_uni_partials(128) = 16 workgroups of eight waves, so
    every wave has a source (128 >= 16 * 8) and every output column of a carried sum a job wave (16 * 4 >= 128 * 2 / 4) --
    the smallest list the batched launch takes at 128 frames.  Device-published rows in front of every second callback:
    callback 1 consumes them as block 1 of a k_hrtf_multi launch, callback 2 waits alone with its rows and is run by
    callback 3's new list (one k_hrtf_uni launch that reads the rows itself), callbacks 3 and 4 are a batch again."""
    K = gas.capi
    plan = [(True, False, False), (False, True, True), (False, True, False), (True, False, False), (False, True, True), (True, False, False)]
    kernels = {}

    def leg(g, fail):
        steps, kernels[fail] = block_leg(g, fail, 128, K.FLAG_PIPELINED_MIX | K.FLAG_BATCHED_LAUNCH, plan)
        return steps

    both(leg, gas)
    for fail in (False, True):  # the last timed launch behind callbacks 1 and 4 is the batch of two
        assert len(kernels[fail]) == 2 and all(k.startswith("k_hrtf_multi") for k in kernels[fail]), kernels[fail]


# ---- 3, 4: the stream entries ----


def stream_scene(ctx, K, rng, n_hrtf):
    """n_hrtf plain-[HRTF] playbacks, one [HIGHSHELF, HRTF] playback and one 3D-mix playback, each bound to an S16 stream
    of its own; playback 1 ends inside the third callback, the others outlast the test."""
    from godot_audio_spatializer_amd import synth

    hrtf = ctx.source_alloc_many(n_hrtf, K.KIND_EFFECT, (K.FX_HRTF,))
    shelf = ctx.source_alloc(K.KIND_EFFECT, (K.FX_HIGHSHELF, K.FX_HRTF))
    mix3d = ctx.source_alloc(K.KIND_3D_MIX, ())
    every = u32(list(hrtf) + [shelf, mix3d])
    params = synth.draw_params(rng, len(every), dirs=DIRS, frames=F)
    ctx.params_publish_batch(every, params)
    for i, s in enumerate(every):
        frames = 2 * F + 30 if i == 1 else 12 * F
        pcm = rng.integers(-20000, 20000, (frames, 2) if i % 2 else frames).astype(np.int16)
        ctx.source_bind_stream(int(s), ctx.stream_create(pcm), start_frame=i)
    return u32(hrtf), int(shelf), int(mix3d), params


def reject_pitch(ctx, K, slot, row, call):
    """A non-resampled playback published with pitch_scale 2 is refused; the parameter goes back before the valid call."""
    bad = row.copy()
    bad["pitch_scale"] = 2.0
    ctx.params_publish_batch(u32([slot]), bad)
    assert call() == UNSUPPORTED_CHAIN
    ctx.params_publish_batch(u32([slot]), row)


def streams_leg(gas, fail, mem):
    import torch

    K = gas.capi
    n = 16
    rng = np.random.default_rng(21)
    ctx = gas.SpatializerContext(max_sources=n + 4, frames=F)
    try:
        ctx.hrtf_load(hrir16())
        slots, shelf, mix3d, params = stream_scene(ctx, K, rng, n)
        free = unused_slot(n + 4, list(slots) + [shelf, mix3d])
        d_out = torch.full((1, F, 2), float("nan"), device="cuda")
        d_pk = torch.zeros(n, 2, device="cuda")
        torch.cuda.synchronize()

        def call(s, frames=F):
            """-> (status, mix, peaks, has_frames), through host or device memory"""
            s = u32(s)
            hf = np.full(len(s), 7, np.uint8)
            if mem == K.MEM_HOST:
                out, pk = np.full((1, F, 2), np.nan, np.float32), np.zeros((len(s), 2), np.float32)
                rc = ctx.lib.gas_process_block_streams(ctx.h, vp(s), len(s), frames, vp(out), vp(pk), vp(hf), mem)
                return rc, out, pk, hf
            rc = ctx.lib.gas_process_block_streams(ctx.h, vp(s), len(s), frames, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_pk.data_ptr()), vp(hf), mem)
            ctx.synchronize()
            return rc, d_out.cpu().numpy(), d_pk.cpu().numpy(), hf

        steps = []
        for t in range(5):
            if fail:
                assert call(slots, F // 2)[0] == FRAME_COUNT
                assert call(list(slots[:-1]) + [free])[0] == BAD_SLOT
                assert call(list(slots[:-1]) + [slots[0]])[0] == INVALID_ARGUMENT
                reject_pitch(ctx, K, slots[3], params[3:4], lambda: call(slots)[0])
            rc, mix, pk, hf = call(slots)
            assert rc == 0 and ctx.stream_last_fused() and mix.any() and not np.isnan(mix).any()
            steps.append({"mix": mix, "peaks": pk, "has_frames": hf, "positions": ctx.stream_positions(n)})
        assert steps[1]["has_frames"][1] == 1 and steps[2]["has_frames"][1] == 0  # playback 1 ended inside callback 2
        return steps
    finally:
        ctx.close()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_process_block_streams_fused(gas, mem):
    """16 bound S16 playbacks of plain [HRTF] chains: the HRTF launch samples the streams itself."""
    K = gas.capi
    both(lambda g, fail: streams_leg(g, fail, K.MEM_HOST if mem == "host" else K.MEM_DEVICE), gas)


def stream_buses_leg(gas, fail):
    K = gas.capi
    n, n_buses = 16, 2
    rng = np.random.default_rng(31)
    ctx = gas.SpatializerContext(max_sources=n + 4, frames=F)
    try:
        ctx.hrtf_load(hrir16())
        slots, shelf, mix3d, params = stream_scene(ctx, K, rng, n)
        every = u32(list(slots) + [shelf, mix3d])
        free = unused_slot(n + 4, every)
        routes = K.bus_routes(len(every))
        routes["dry_bus"] = rng.integers(0, n_buses, len(every))
        routes["send_bus"][::3] = 1
        routes["send"][::3, 0] = (0.5, 0.25)
        ctx.bus_routes_publish(every, routes)

        def status(s, frames=F):
            s = u32(s)
            out, pk, hf = np.full((n_buses, 1, F, 2), np.nan, np.float32), np.zeros((len(s), 2), np.float32), np.zeros(len(s), np.uint8)
            return ctx.lib.gas_process_block_streams_buses(ctx.h, vp(s), len(s), frames, vp(out), n_buses, vp(pk), vp(hf), K.MEM_HOST)

        steps = []
        staged_list = u32(list(slots[:-1]) + [shelf])  # one [HIGHSHELF, HRTF] source swapped in: the staged form, regrouped every call
        for t in range(6):
            lst = slots if t < 3 else staged_list
            if fail:
                assert status(lst, F // 2) == FRAME_COUNT
                assert status(list(lst[:-1]) + [free]) == BAD_SLOT
                assert status(list(lst[:-1]) + [lst[0]]) == INVALID_ARGUMENT
                assert status(list(lst[:-1]) + [mix3d]) == UNSUPPORTED_CHAIN
                reject_pitch(ctx, K, lst[3], params[3:4], lambda: status(lst))
            mix, pk, hf = ctx.process_block_streams_buses(lst, n_buses)
            assert ctx.stream_last_fused() == (t < 3) and mix[0].any() and mix[1].any() and not np.isnan(mix).any()
            steps.append({"mix": mix, "peaks": pk, "has_frames": hf, "positions": ctx.stream_positions(n)})
        return steps
    finally:
        ctx.close()


def test_process_block_streams_buses_fused_then_staged(gas):
    both(stream_buses_leg, gas)


# ---- 5: gas_process_block_buses, host memory ----


def buses_leg(gas, fail):
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, n_buses = 16, 3
    rng = np.random.default_rng(41)
    ctx = gas.SpatializerContext(max_sources=n + 4, frames=F)
    try:
        ctx.hrtf_load(hrir16())
        slots = u32(ctx.source_alloc_many(n, K.KIND_3D_MIX, ()))
        effect = ctx.source_alloc(K.KIND_EFFECT, (K.FX_HRTF,))
        every = u32(list(slots) + [effect])
        ctx.params_publish_batch(every, synth.draw_params(rng, n + 1, dirs=DIRS, frames=F))
        free = unused_slot(n + 4, every)
        routes = K.bus_routes(n + 1)
        routes["dry_bus"] = rng.integers(0, n_buses, n + 1)
        routes["send_bus"][::2] = 2
        routes["send"][::2, 0] = (0.7, 0.4)
        ctx.bus_routes_publish(every, routes)

        def status(src, s, frames=F):
            s = u32(s)
            out, pk = np.full((n_buses, 1, F, 2), np.nan, np.float32), np.zeros((len(s), 2), np.float32)
            return ctx.lib.gas_process_block_buses(ctx.h, vp(src), vp(s), len(s), frames, vp(out), n_buses, vp(pk), K.MEM_HOST)

        steps = []
        for t in range(4):
            src = synth.draw_sources(rng, n, F)
            if fail:
                assert status(src, slots, F // 2) == FRAME_COUNT
                assert status(src, list(slots[:-1]) + [free]) == BAD_SLOT
                assert status(src, list(slots[:-1]) + [slots[0]]) == INVALID_ARGUMENT
                assert status(src, list(slots[:-1]) + [effect]) == UNSUPPORTED_CHAIN
            mix, pk = ctx.process_block_buses(src, slots, n_buses)
            assert all(mix[b].any() for b in range(n_buses)) and not np.isnan(mix).any()
            steps.append({"mix": mix, "peaks": pk})
        return steps
    finally:
        ctx.close()


def test_process_block_buses_3d_mix(gas):
    both(buses_leg, gas)
