"""GAS_FX_DELAY / GAS_FX_REVERB on the GPU (k_fx_line.hip) against the numpy restatement tests/fx_line_ref.py,
composed with the oracle's existing kinds (oracle.binding.BatchOracle) and tests/fx_dyn_ref.py for mixed chains; and
the line pools' lifecycle (gas_ctx_reserve_fx_lines)."""
import numpy as np
import pytest

import fx_dyn_ref
import fx_line_ref as ref
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HS, ER, HRTF, LP, AMP = 1, 2, 3, 4, 9
DIST, COMP = 11, 12
DELAY, REVERB = 13, 14
LINE = (DELAY, REVERB)
BAD_ARG, OUT_OF_SLOTS, UNSUPPORTED = -1, -2, -6


def _hrir(dirs=32, seed=5):
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(seed), dirs=dirs)


class ChainRef:
    """A playback chain's reference: runs of the existing kinds through BatchOracle (one source per oracle where a new
    kind follows, for its rows; all sources in one oracle for a last run), the line kinds through fx_line_ref, the
    dynamics kinds through fx_dyn_ref (on their resource defaults)."""

    def __init__(self, ob, chain, n, frames, hrir=None, ring=0, max_ms=1500.0, echo_frames=None):
        self.stages = []
        segs = []
        for j, k in enumerate(chain):
            own = k in LINE or k in (DIST, COMP)
            if segs and not own and not segs[-1][0]:
                segs[-1][1].append(j)
            else:
                segs.append((own, [j]))
        for si, (own, pos) in enumerate(segs):
            k0 = chain[pos[0]]
            if k0 in LINE:
                self.stages.append(("line", ref.make_stage(k0, pos[0], n, max_ms=max_ms, echo_frames=echo_frames)))
                continue
            if own:
                self.stages.append(("dyn", fx_dyn_ref.DynStage(k0, pos[0], n)))
                continue
            sub = tuple(chain[j] for j in pos)
            mk = lambda m: ob.BatchOracle(ob.KIND_EFFECT, m, frames, chain=sub, hrir=hrir, er_ring_frames=max(ring, 1))  # noqa: E731
            if si == len(segs) - 1:
                self.stages.append(("last", mk(n)))
            else:
                self.stages.append(("rows", [mk(1) for _ in range(n)]))

    def reset(self, s):
        for kind, obj in self.stages:
            obj.reset(s)

    def block(self, params, src, settings, dyn=None):
        """-> (mix64 [F][2], peaks [n][2])."""
        import oracle.binding as ob

        p = params.astype(ob.PARAMS_DTYPE)
        x = np.asarray(src, np.float32)
        for kind, obj in self.stages:
            if kind == "line":
                x = obj.block(x, settings)
            elif kind == "dyn":
                x = obj.block(x, dyn if dyn is not None else _capi().fx_dyn_settings_defaults(len(x)))
            elif kind == "rows":
                x = np.stack([o.block(p[s : s + 1], x[s : s + 1])[0][0] for s, o in enumerate(obj)])
            else:
                _, peaks, r64 = obj.block(p, x, want64=True)
                return r64[0], peaks
        return x.astype(np.float64).sum(axis=0), np.abs(x).max(axis=1)


def _capi():
    from godot_audio_spatializer_amd import capi

    return capi


def _lines(chain, n):
    return n * sum(k == DELAY for k in chain), n * sum(k == REVERB for k in chain)


def run_chain(gas, ob, chain, n, frames, blocks=9, seed=0, max_ms=1500.0, max_pd=500.0, src_fn=None, hrir_dirs=32, edit=None, check=True, republish=True):
    """Random legal settings re-published at blocks 1, 4, 7 (all, then half the sources) unless `republish` is off;
    `edit(b, settings)` may change them before block b (published for every source).  Returns the last mix."""
    from godot_audio_spatializer_amd import synth

    rng = np.random.default_rng(seed)
    ring = 4096 if ER in chain else 0
    hrir = _hrir(hrir_dirs) if HRTF in chain else None
    echo = 2048 if max_pd <= 40.0 else None
    with gas.SpatializerContext(max_sources=n + 3, frames=frames, er_ring_frames=ring) as ctx:
        ctx.reserve_fx_lines(*_lines(chain, n))
        if hrir is not None:
            ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring, max_ms=max_ms, echo_frames=echo)
        settings = gas.capi.fx_line_settings_defaults(n)  # block 0 runs on the resource defaults
        if max_ms < 1500.0 or max_pd < 500.0:  # (the defaults' delays are longer than a small reference's buffers)
            settings = ref.draw_settings(rng, n, gas.capi, max_ms=max_ms, max_predelay_ms=max_pd)
            ctx.fx_line_settings_publish(slots, settings)
        for b in range(blocks):
            if b % 3 == 0:
                p = synth.draw_params(rng, n, dirs=hrir_dirs, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            if republish and b in (1, 4, 7):
                who = np.arange(n) if b == 1 else rng.choice(n, max(1, n // 2), replace=False)
                new = ref.draw_settings(rng, len(who), gas.capi, max_ms=max_ms, max_predelay_ms=max_pd)
                ctx.fx_line_settings_publish(slots[who], new)
                settings[who] = new
            if edit is not None and edit(b, settings):
                ctx.fx_line_settings_publish(slots, settings)
            src = synth.draw_sources(rng, n, frames) if src_fn is None else src_fn(rng, b, n, frames)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks = r.block(p, src, settings)
            if check:
                assert rel_rms(mix[0], want) <= TOL, f"{chain} n={n} F={frames} block {b}: {rel_rms(mix[0], want)}"
                np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=f"block {b}")
    return mix


NF = [(1, 128), (31, 256), (256, 512), (31, 128), (256, 256)]


@pytest.mark.parametrize("kind", LINE)
@pytest.mark.parametrize("n,frames", NF)
def test_alone(gas, ob, kind, n, frames):
    run_chain(gas, ob, (kind,), n, frames, seed=kind * 7 + n + frames)


@pytest.mark.parametrize("kind", LINE)
def test_alone_8192(gas, ob, kind):
    """8192 sources; delays and predelay up to 40 ms so that the reference's buffers fit in host memory."""
    run_chain(gas, ob, (kind,), 8192, 512, seed=kind, max_ms=40.0, max_pd=40.0)


def test_delay_long_run_wraps_ring_and_feedback(gas, ob):
    """300 blocks of 512: the 2^17-frame ring wraps (and the feedback buffer, many times); taps at 0, < F and 1500 ms."""
    def edit(b, s):
        if b == 0:
            s["delay_tap1_ms"][:, 0] = [0.0, 2.0, 700.0, 1500.0]
            s["delay_tap2_ms"][:, 0] = [1500.0, 1499.0, 0.5, 1000.0]
            s["delay_tap1_active"] = 1
            s["delay_tap2_active"] = 1
            s["delay_feedback_active"] = 1
            s["delay_feedback_ms"][:, 0] = [1500.0, 340.0, 1.0, 20.0]
            s["delay_feedback_level_db"] = -3.0
            return True
        return False

    def src_fn(rng, b, n, frames):  # bursts, so that the echoes show between them
        x = rng.uniform(-1, 1, (n, frames, 2)).astype(np.float32)
        return x if b % 50 < 2 else (x * np.float32(1e-3))

    run_chain(gas, ob, (DELAY,), 4, 512, blocks=300, seed=3, edit=edit, src_fn=src_fn, republish=False)


def test_reverb_long_run_wraps_the_echo_buffer(gas, ob):
    def edit(b, s):
        if b == 0:
            s["reverb_predelay_ms"][:, 0] = [20.0, 500.0, 150.0, 333.0]
            s["reverb_predelay_feedback"][:, 0] = [0.98, 0.5, 0.0, 0.9]
            s["reverb_room_size"][:, 0] = [1.0, 0.5, 0.0, 0.8]
            return True
        return False

    def src_fn(rng, b, n, frames):
        x = rng.uniform(-1, 1, (n, frames, 2)).astype(np.float32)
        return x if b % 20 < 3 else np.zeros_like(x)

    run_chain(gas, ob, (REVERB,), 4, 512, blocks=60, seed=4, edit=edit, src_fn=src_fn, republish=False)


def test_delay_edges(gas, ob):
    """Dfb at 0, below the 64-frame tile, below F and >= F; the feedback delay shortened mid-stream (q >= Dfb) and the
    feedback switched off mid-stream (the stored echo keeps playing one more cycle); tap 0 and taps below F."""
    fb_ms = np.array([0.0, 0.5, 1.0, 2.0, 8.0, 20.0, 340.0, 1500.0])

    def edit(b, s):
        if b == 0:
            s["delay_tap1_ms"][:, 0] = np.tile([0.0, 0.02, 1.0, 5.0], 2)
            s["delay_tap2_ms"][:, 0] = np.tile([10.0, 1.3, 0.0, 2.6], 2)
            s["delay_tap1_active"] = 1
            s["delay_tap2_active"] = 1
            s["delay_feedback_active"] = 1
            s["delay_feedback_ms"][:, 0] = fb_ms
            s["delay_feedback_level_db"] = -2.0
            s["delay_feedback_lowpass_hz"] = 12000.0
            return True
        if b == 4:
            s["delay_feedback_ms"][:, 0] = fb_ms / 3.0
            return True
        if b == 8:
            s["delay_feedback_active"] = 0
            return True
        return False

    def src_fn(rng, b, n, frames):
        x = rng.uniform(-1, 1, (n, frames, 2)).astype(np.float32)
        return x if b < 2 or b == 6 else x * np.float32(0.0)

    run_chain(gas, ob, (DELAY,), 8, 256, blocks=12, seed=5, edit=edit, src_fn=src_fn, republish=False)


def test_reverb_edges(gas, ob):
    """Spread changed mid-stream (limits move under the positions), hipass switched on and off, predelay at 20 and
    500 ms, predelay feedback 0.98 and room size 1."""
    def edit(b, s):
        if b == 0:
            s["reverb_predelay_ms"][:, 0] = [20.0, 500.0, 20.0, 500.0, 100.0, 250.0]
            s["reverb_predelay_feedback"][:, 0] = [0.98, 0.98, 0.0, 0.5, 0.98, 0.3]
            s["reverb_room_size"][:, 0] = [1.0, 1.0, 0.2, 1.0, 0.0, 0.7]
            s["reverb_spread"][:, 0] = [1.0, 0.0, 0.5, 1.0, 0.0, 0.25]
            s["reverb_hipass"][:, 0] = [0.0, 0.5, 0.0, 1.0, 0.2, 0.0]
            return True
        if b in (3, 5, 8):
            s["reverb_spread"][:, 0] = 1.0 - s["reverb_spread"][:, 0]
            s["reverb_hipass"][:, 0] = np.where(s["reverb_hipass"][:, 0] > 0, 0.0, 0.4)
            return True
        return False

    def src_fn(rng, b, n, frames):
        x = rng.uniform(-1, 1, (n, frames, 2)).astype(np.float32)
        return x if b % 4 == 0 else x * np.float32(0.01)

    run_chain(gas, ob, (REVERB,), 6, 512, blocks=12, seed=6, edit=edit, src_fn=src_fn, republish=False)


@pytest.mark.parametrize(
    "chain,frames",
    [
        ((REVERB, HRTF), 512),
        ((HS, DELAY, HRTF), 256),
        ((DELAY, REVERB), 512),
        ((COMP, DELAY, AMP), 128),
        ((DELAY, DELAY), 256),
        ((ER, REVERB), 256),
    ],
)
def test_mixed_chains_next_to_fused_chains(gas, ob, chain, frames):
    """The chain's playbacks share callbacks with fused [HRTF] and [HIGHSHELF] playbacks; mix and peaks of all."""
    from godot_audio_spatializer_amd import synth

    n, nf = 24, 10
    rng = np.random.default_rng(len(chain) * 13 + frames)
    ring = 4096 if ER in chain else 0
    hrir = _hrir()
    with gas.SpatializerContext(max_sources=n + 2 * nf, frames=frames, er_ring_frames=ring) as ctx:
        ctx.reserve_fx_lines(*_lines(chain, n))
        ctx.hrtf_load(hrir)
        a = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        h = ctx.source_alloc_many(nf, gas.capi.KIND_EFFECT, (HRTF,))
        s_ = ctx.source_alloc_many(nf, gas.capi.KIND_EFFECT, (HS,))
        slots = np.concatenate([a, h, s_])
        order = rng.permutation(len(slots))  # interleaved in the callback's list
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring)
        rh = ob.BatchOracle(ob.KIND_EFFECT, nf, frames, chain=(HRTF,), hrir=hrir, er_ring_frames=1)
        rs = ob.BatchOracle(ob.KIND_EFFECT, nf, frames, chain=(HS,), hrir=None, er_ring_frames=1)
        settings = gas.capi.fx_line_settings_defaults(n)
        for b in range(6):
            if b % 3 == 0:
                p = synth.draw_params(rng, len(slots), dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            if b in (1, 4):
                settings = ref.draw_settings(rng, n, gas.capi)
                ctx.fx_line_settings_publish(a, settings)
            src = synth.draw_sources(rng, len(slots), frames)
            mix, peaks = ctx.process_block(src[order], slots[order])
            w0, p0 = r.block(p[:n], src[:n], settings)
            _, p1, w1 = rh.block(p[n : n + nf].astype(ob.PARAMS_DTYPE), src[n : n + nf], want64=True)
            _, p2, w2 = rs.block(p[n + nf :].astype(ob.PARAMS_DTYPE), src[n + nf :], want64=True)
            want = w0 + w1[0] + w2[0]
            assert rel_rms(mix[0], want) <= TOL, f"{chain} block {b}: {rel_rms(mix[0], want)}"
            rpeaks = np.concatenate([p0, p1, p2])[order]
            np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=f"block {b}")


def test_reverb_hrtf_peaks_draining_only(gas, ob):
    """[REVERB, HRTF] under GAS_FLAG_PEAKS_DRAINING_ONLY: +inf for the playbacks that are not draining, the exact peak
    for the draining ones."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F = 40, 512
    rng = np.random.default_rng(21)
    hrir = _hrir()
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PEAKS_DRAINING_ONLY) as ctx:
        ctx.reserve_fx_lines(0, n)
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (REVERB, HRTF))
        draining = np.arange(n) % 5 == 2
        for s in slots[draining]:
            ctx.source_set_draining(int(s), True)
        r = ChainRef(ob, (REVERB, HRTF), n, F, hrir=hrir)
        settings = ref.draw_settings(rng, n, K)
        ctx.fx_line_settings_publish(slots, settings)
        p = synth.draw_params(rng, n, dirs=32, frames=F)
        ctx.params_publish_batch(slots, p)
        for b in range(4):
            src = synth.draw_sources(rng, n, F)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks = r.block(p, src, settings)
            assert rel_rms(mix[0], want) <= TOL
            assert np.isinf(peaks[~draining]).all() and (peaks[~draining] > 0).all()
            np.testing.assert_allclose(peaks[draining], rpeaks[draining], rtol=2e-5, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------- pools
def _status(gas, fn, *a):
    try:
        fn(*a)
    except gas.GasError as e:
        return e.status
    return 0


def _free_slots(gas, ctx):
    got = []
    while True:
        try:
            got.append(ctx.source_alloc(gas.capi.KIND_EFFECT, ()))
        except gas.GasError as e:
            assert e.status == OUT_OF_SLOTS
            break
    for s in got:
        ctx.source_free(s)
    ctx.process_block(np.zeros((0, ctx.frames, 2), np.float32), np.zeros(0, np.uint32))
    return len(got)


def test_pool_errors_and_lifecycle(gas):
    K = gas.capi
    F = 128
    with gas.SpatializerContext(max_sources=8, frames=F) as ctx:
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY,)) == UNSUPPORTED  # no pool reserved
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (HS, REVERB)) == UNSUPPORTED
        ctx.reserve_fx_lines(2, 1)
        a = ctx.source_alloc(K.KIND_EFFECT, (DELAY,))
        b = ctx.source_alloc(K.KIND_EFFECT, (DELAY, REVERB))
        from godot_audio_spatializer_amd import synth

        ctx.params_publish(b, synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F)[0])
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY,)) == OUT_OF_SLOTS  # delay pool exhausted
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (REVERB,)) == OUT_OF_SLOTS
        assert _free_slots(gas, ctx) == 6  # nothing was taken by the refused calls
        assert _status(gas, ctx.reserve_fx_lines, 4, 4) == BAD_ARG  # lines are held
        ctx.source_free(a)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY,)) == OUT_OF_SLOTS  # back at the next block only
        assert _status(gas, ctx.reserve_fx_lines, 4, 4) == BAD_ARG
        ctx.process_block(np.zeros((1, F, 2), np.float32), np.array([b], np.uint32))
        c = ctx.source_alloc(K.KIND_EFFECT, (DELAY,))
        ctx.source_free(b)
        ctx.source_free(c)
        ctx.process_block(np.zeros((0, F, 2), np.float32), np.zeros(0, np.uint32))
        ctx.reserve_fx_lines(1, 2)  # nothing held: re-sized
        ctx.source_alloc(K.KIND_EFFECT, (REVERB, REVERB))
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY, DELAY)) == OUT_OF_SLOTS
    with gas.SpatializerContext(max_sources=4, frames=512, mix_rate=22050.0) as ctx:  # 20 ms < 512 frames
        assert _status(gas, ctx.reserve_fx_lines, 0, 1) == BAD_ARG
        ctx.reserve_fx_lines(1, 0)
        ctx.reserve_fx_lines(0, 0)
    with gas.SpatializerContext(max_sources=4, frames=256, mix_rate=22050.0) as ctx:
        ctx.reserve_fx_lines(1, 1)


def _render(gas, chain, srcs, settings, slot_prep=None):
    """A fresh context's output for one playback of `chain` over srcs; slot_prep(ctx) may run a different history first."""
    from godot_audio_spatializer_amd import synth

    F = srcs[0].shape[1]
    with gas.SpatializerContext(max_sources=2, frames=F) as ctx:
        ctx.reserve_fx_lines(*_lines(chain, 1))
        p = synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F)
        slot = ctx.source_alloc(gas.capi.KIND_EFFECT, chain) if slot_prep is None else slot_prep(ctx, p)
        ctx.params_publish(slot, p[0])
        ctx.fx_line_settings_publish(np.array([slot], np.uint32), settings)
        return np.stack([ctx.process_block(x, np.array([slot], np.uint32))[0] for x in srcs])


@pytest.mark.parametrize("how", ["recycled", "reset"])
def test_recycled_or_reset_line_is_bitwise_fresh(gas, how):
    """A loud history with long feedback / a full reverb, then the slot and its lines recycled (free, block, alloc) or
    gas_source_reset: the next playback equals a fresh context's bit for bit (no echo left over)."""
    K = gas.capi
    F = 256
    chain = (DELAY, REVERB)
    rng = np.random.default_rng(31)
    s = K.fx_line_settings_defaults(1)
    s["delay_feedback_active"] = 1
    s["delay_feedback_level_db"] = -1.0
    s["reverb_room_size"] = 1.0
    s["reverb_predelay_feedback"] = 0.98
    srcs = [rng.uniform(-1, 1, (1, F, 2)).astype(np.float32) for _ in range(6)]

    def prep(ctx, p):
        slot = ctx.source_alloc(K.KIND_EFFECT, chain)
        ctx.params_publish(slot, p[0])
        ctx.fx_line_settings_publish(np.array([slot], np.uint32), s)
        for _ in range(8):
            ctx.process_block(rng.uniform(-1, 1, (1, F, 2)).astype(np.float32), np.array([slot], np.uint32))
        if how == "reset":
            ctx.source_reset(slot)
            return slot
        ctx.source_free(slot)
        ctx.process_block(np.zeros((0, F, 2), np.float32), np.zeros(0, np.uint32))
        slot2 = ctx.source_alloc(K.KIND_EFFECT, chain)
        assert slot2 == slot
        return slot2

    fresh = _render(gas, chain, srcs, s)
    again = _render(gas, chain, srcs, s, slot_prep=prep)
    np.testing.assert_array_equal(again, fresh)


def test_buses_with_line_kinds(gas, ob):
    from godot_audio_spatializer_amd import synth

    F, n = 256, 30
    rng = np.random.default_rng(10)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_lines(n, 0)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (DELAY,))
        p = synth.draw_params(rng, n, dirs=8, frames=F)
        ctx.params_publish_batch(slots, p)
        s = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_line_settings_publish(slots, s)
        routes = gas.capi.bus_routes(n)
        routes["dry_bus"] = np.where(np.arange(n) % 3 == 0, 1, 0)
        routes["send_bus"] = np.where(np.arange(n) % 3 == 0, 0, 1)
        routes["send"] = rng.uniform(0, 1, (n, 1, 1)).astype(np.float32) * np.ones((4, 2), np.float32)
        ctx.bus_routes_publish(slots, routes)
        st = ref.DelayStage(0, n)
        for b in range(4):
            src = synth.draw_sources(rng, n, F)
            out, peaks = ctx.process_block_buses(src, slots, 2)
            y = st.block(src, s).astype(np.float64)
            for bus in range(2):
                w = (routes["dry_bus"] == bus).astype(np.float64) + (routes["send_bus"] == bus) * routes["send"][:, 0, 0].astype(np.float64)
                want = (y * w[:, None, None]).sum(axis=0)
                assert rel_rms(out[bus, 0], want) <= TOL, f"block {b} bus {bus}"
            np.testing.assert_allclose(peaks, np.abs(y).max(axis=1), rtol=2e-5, atol=1e-7)


def test_process_frames_1_matches_the_batched_row_bitwise(gas):
    from godot_audio_spatializer_amd import synth

    F = 256
    rng = np.random.default_rng(11)
    chain = (REVERB, DELAY)
    s = ref.draw_settings(rng, 1, gas.capi)
    srcs = [synth.draw_sources(rng, 1, F) for _ in range(4)]
    outs = []
    for single in (False, True):
        with gas.SpatializerContext(max_sources=2, frames=F) as ctx:
            ctx.reserve_fx_lines(1, 1)
            slots = ctx.source_alloc_many(1, gas.capi.KIND_EFFECT, chain)
            ctx.params_publish_batch(slots, synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F))
            ctx.fx_line_settings_publish(slots, s)
            got = [ctx.process_frames_1(int(slots[0]), x[0]) if single else ctx.process_block(x, slots)[0][0] for x in srcs]
            outs.append(np.stack(got))
    np.testing.assert_array_equal(outs[0], outs[1])


def test_host_layer_queues_line_settings(gas):
    """BatchedSpatializerHost + gas_host_set_effect_settings_line: one playback through [DELAY, REVERB] equals the
    reference applied to what the same host delivers for an empty chain."""
    K = gas.capi
    F = 256
    rng = np.random.default_rng(12)
    stream = rng.uniform(-0.8, 0.8, (F * 20, 2)).astype(np.float32)
    from godot_audio_spatializer_amd import synth

    params = synth.draw_params(rng, 1, dirs=8, frames=F)
    new = ref.draw_settings(rng, 1, K)
    got = {}
    for chain in ((DELAY, REVERB), ()):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_fx_lines(2, 2)
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, chain)
            pid = host.start_playback_array(stream)
            host.set_spatializer_parameters(pid, params[0])
            outs = []
            for cb in range(8):
                if cb == 3 and chain:
                    assert host.set_effect_line_settings(pid, new) == 0
                    bad = new.copy()
                    bad["reverb_predelay_ms"][0, 2] = 10.0
                    assert host.set_effect_line_settings(pid, bad) == BAD_ARG  # refused when queued
                rc, out = host.get_mixed_frames(0, F)
                assert rc == 0
                outs.append(out.copy())
            host.close()
        got[chain] = np.stack(outs)
    window = got[()]
    dl, rv = ref.DelayStage(0, 1), ref.ReverbStage(1, 1)
    d = K.fx_line_settings_defaults(1)
    for cb in range(8):
        st = new if cb >= 3 else d
        y = rv.block(dl.block(window[cb][None], st), st)[0]
        assert rel_rms(got[(DELAY, REVERB)][cb], y) <= TOL, f"callback {cb}"


def test_two_runs_are_bitwise_equal(gas, ob):
    a = run_chain(gas, ob, (DELAY, REVERB), 70, 256, blocks=4, seed=5, check=False)
    b = run_chain(gas, ob, (DELAY, REVERB), 70, 256, blocks=4, seed=5, check=False)
    np.testing.assert_array_equal(a, b)


def test_invalid_settings_are_refused_with_nothing_taken(gas, ob):
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F = 128
    with gas.SpatializerContext(max_sources=3, frames=F) as ctx:
        ctx.reserve_fx_lines(2, 0)
        slots = ctx.source_alloc_many(2, K.KIND_EFFECT, (DELAY,))
        bad_values = [
            ("delay_tap1_ms", 1500.5), ("delay_tap2_ms", -1.0), ("delay_feedback_ms", 2000.0), ("delay_tap1_pan", 1.5),
            ("delay_tap2_pan", -1.01), ("delay_feedback_lowpass_hz", 0.5), ("delay_feedback_lowpass_hz", 16001.0),
            ("reverb_predelay_ms", 19.0), ("reverb_predelay_ms", 501.0), ("reverb_predelay_feedback", 0.99),
            ("reverb_room_size", 1.1), ("reverb_damping", -0.1), ("reverb_spread", 2.0), ("reverb_hipass", 1.5),
            ("reverb_dry", np.nan), ("reverb_wet", -0.5), ("delay_dry", 1.2), ("delay_tap1_level_db", np.inf),
            ("delay_feedback_level_db", np.nan),
        ]
        for field, value in bad_values:
            s = K.fx_line_settings_defaults(2)
            s["delay_tap1_ms"][0] = 3.0  # a valid change on the first row: must not be taken either
            s[field][1, 3] = value
            with pytest.raises(gas.GasError) as ei:
                ctx.fx_line_settings_publish(slots, s)
            assert ei.value.status == BAD_ARG, (field, value)
        p = synth.draw_params(np.random.default_rng(0), 2, dirs=8, frames=F)
        ctx.params_publish_batch(slots, p)
        st = ref.DelayStage(0, 2)
        d = K.fx_line_settings_defaults(2)
        rng = np.random.default_rng(1)
        for _ in range(3):
            src = rng.uniform(-1, 1, (2, F, 2)).astype(np.float32)
            mix, _ = ctx.process_block(src, slots)
            assert rel_rms(mix[0], st.block(src, d).astype(np.float64).sum(axis=0)) <= TOL
        with pytest.raises(gas.GasError):
            ctx.source_alloc(K.KIND_EFFECT, (DELAY, 15))  # 15 is no effect kind
