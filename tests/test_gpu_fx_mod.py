"""GAS_FX_CHORUS / GAS_FX_PHASER on the GPU (k_fx_mod.hip) against the numpy restatement tests/fx_mod_ref.py, composed
with the oracle's existing kinds (oracle.binding.BatchOracle) and tests/fx_{dyn,line,eq}_ref.py for mixed chains; and
the pools' lifecycle (gas_ctx_reserve_fx_mod).

The kernels run every recurrence in the engine's order with separate f32 operations, as the restatement does, and
evaluate every sine in f64.  The device's f64 sine and exp may differ from the host's in the last f64 bit, which moves
an f32 result only where it rounds on a tie, so a source's peak is compared within 1e-6 of the restatement's and the
number of bitwise-equal peaks is reported (all of them are expected to be).  The mix is compared within TOL because
the library sums the sources in f32 in its own order and the reference in f64."""
import numpy as np
import pytest

import fx_dyn_ref
import fx_eq_ref
import fx_line_ref
import fx_mod_ref as ref
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HS, ER, HRTF, LP, AMP = 1, 2, 3, 4, 9
DIST, COMP = 11, 12
DELAY, REVERB = 13, 14
EQ6, EQ10, EQ21 = 16, 17, 18
CHORUS, PHASER = 19, 20
MODS = (CHORUS, PHASER)
BAD_ARG, OUT_OF_SLOTS, UNSUPPORTED = -1, -2, -6


def _hrir(dirs=32, seed=5):
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(seed), dirs=dirs)


def _capi():
    from godot_audio_spatializer_amd import capi

    return capi


def _close_peaks(peaks, rpeaks, what):
    """Within 1e-6 of the restatement's peak per source and ear; returns how many are bitwise equal."""
    np.testing.assert_allclose(peaks, rpeaks, rtol=1e-6, atol=1e-9, err_msg=what)
    return int((peaks == rpeaks).all(axis=-1).sum())


class ChainRef:
    """A playback chain's reference: runs of the existing kinds through BatchOracle (one source per oracle where a new
    kind follows, for its rows; all sources in one oracle for a last run), the chorus and phaser through fx_mod_ref,
    the other library kinds through fx_dyn_ref / fx_line_ref / fx_eq_ref on their resource defaults."""

    def __init__(self, ob, chain, n, frames, hrir=None, ring=0, mix_rate=48000.0):
        self.stages = []
        segs = []
        own_kinds = MODS + (DIST, COMP, DELAY, REVERB, EQ6, EQ10, EQ21)
        for j, k in enumerate(chain):
            own = k in own_kinds
            if segs and not own and not segs[-1][0]:
                segs[-1][1].append(j)
            else:
                segs.append((own, [j]))
        for si, (own, pos) in enumerate(segs):
            k0 = chain[pos[0]]
            if k0 in MODS:
                self.stages.append(("mod", ref.make_stage(k0, pos[0], n, mix_rate)))
            elif k0 in (EQ6, EQ10, EQ21):
                self.stages.append(("eq", fx_eq_ref.EqStage(k0, pos[0], n, mix_rate)))
            elif k0 in (DELAY, REVERB):
                self.stages.append(("line", fx_line_ref.make_stage(k0, pos[0], n)))
            elif own:
                self.stages.append(("dyn", fx_dyn_ref.DynStage(k0, pos[0], n)))
            else:
                sub = tuple(chain[j] for j in pos)
                mk = lambda m: ob.BatchOracle(ob.KIND_EFFECT, m, frames, chain=sub, hrir=hrir, er_ring_frames=max(ring, 1))  # noqa: E731
                self.stages.append(("last", mk(n)) if si == len(segs) - 1 else ("rows", [mk(1) for _ in range(n)]))

    def reset(self, s):
        for _, obj in self.stages:
            obj.reset(s)

    def block(self, params, src, settings):
        """-> (mix64 [F][2], peaks [n][2], rows [n][F][2] f32 or None when the last stage is the oracle's)."""
        import oracle.binding as ob

        p = params.astype(ob.PARAMS_DTYPE)
        x = np.asarray(src, np.float32)
        for kind, obj in self.stages:
            if kind == "mod":
                x = obj.block(x, settings)
            elif kind == "eq":
                x = obj.block(x, _capi().fx_eq_settings_defaults(len(x)))
            elif kind == "line":
                x = obj.block(x, _capi().fx_line_settings_defaults(len(x)))
            elif kind == "dyn":
                x = obj.block(x, _capi().fx_dyn_settings_defaults(len(x)))
            elif kind == "rows":
                x = np.stack([o.block(p[s : s + 1], x[s : s + 1])[0][0] for s, o in enumerate(obj)])
            else:
                _, peaks, r64 = obj.block(p, x, want64=True)
                return r64[0], peaks, None
        return x.astype(np.float64).sum(axis=0), np.abs(x).max(axis=1), x


def _params(n, frames):
    """Spatializer parameters for playbacks whose chain does not read them (every source needs some published)."""
    from godot_audio_spatializer_amd import synth

    return synth.draw_params(np.random.default_rng(0), n, dirs=8, frames=frames)


def _mods(chain, n):
    return n * sum(k == CHORUS for k in chain), n * sum(k == PHASER for k in chain)


def _reserve(ctx, chain, n):
    ctx.reserve_fx_mod(*_mods(chain, n))
    if DELAY in chain or REVERB in chain:
        ctx.reserve_fx_lines(n * sum(k == DELAY for k in chain), n * sum(k == REVERB for k in chain))
    if any(k in (EQ6, EQ10, EQ21) for k in chain):
        ctx.reserve_fx_eq(n * sum(k in (EQ6, EQ10, EQ21) for k in chain))


def run_chain(gas, ob, chain, n, frames, blocks=4, seed=0, mix_rate=48000.0, check=True):
    """Random settings over the whole range (voice counts 1 .. 4), re-published at every block from the second on (all,
    then half the sources, alternately).  Returns the last mix and the number of bitwise-equal peaks."""
    from godot_audio_spatializer_amd import synth

    rng = np.random.default_rng(seed)
    ring = 4096 if ER in chain else 0
    hrir = _hrir() if HRTF in chain else None
    equal = 0
    with gas.SpatializerContext(max_sources=n + 3, frames=frames, er_ring_frames=ring, mix_rate=mix_rate) as ctx:
        _reserve(ctx, chain, n)
        if hrir is not None:
            ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring, mix_rate=mix_rate)
        settings = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_mod_settings_publish(slots, settings)
        for b in range(blocks):
            if b % 3 == 0:
                p = synth.draw_params(rng, n, dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            if b >= 1:
                who = np.arange(n) if b % 2 else rng.choice(n, max(1, n // 2), replace=False)
                new = ref.draw_settings(rng, len(who), gas.capi)
                ctx.fx_mod_settings_publish(slots[who], new)
                settings[who] = new
            src = synth.draw_sources(rng, n, frames)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks, rows = r.block(p, src, settings)
            if check:
                assert rel_rms(mix[0], want) <= TOL, f"{chain} n={n} F={frames} block {b}: {rel_rms(mix[0], want)}"
                if rows is not None:
                    equal += _close_peaks(peaks, rpeaks, f"{chain} block {b}")
                else:
                    np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=f"block {b}")
    if check and equal:
        print(f"{chain} n={n} F={frames}: {equal} of {n * blocks} source peaks bitwise equal")
    return mix, equal


NF = [(1, 128), (31, 256), (256, 512), (64, 384), (256, 128), (1, 512)]


@pytest.mark.parametrize("kind", MODS)
@pytest.mark.parametrize("n,frames", NF)
def test_alone(gas, ob, kind, n, frames):
    _, equal = run_chain(gas, ob, (kind,), n, frames, seed=kind * 7 + n + frames)
    assert equal == 4 * n


@pytest.mark.parametrize("kind", MODS)
def test_alone_8192(gas, ob, kind):
    _, equal = run_chain(gas, ob, (kind,), 8192, 512, blocks=3, seed=kind)
    assert equal >= 3 * 8192 - 8  # (a device f64 sine one bit off on an f32 tie; none expected)


@pytest.mark.parametrize("kind", MODS)
def test_alone_at_other_rates(gas, ob, kind):
    for sr, F in ((44100.0, 256), (96000.0, 512)):
        run_chain(gas, ob, (kind,), 20, F, blocks=3, mix_rate=sr, seed=kind + int(sr))


@pytest.mark.parametrize("kind", MODS)
def test_one_512_block_equals_two_256_blocks(gas, kind):
    """GPU only: the chorus's 256-frame chunks (and the phaser's frame-by-frame LFO) make one F = 512 callback equal two
    F = 256 callbacks bit for bit -- one source's output, and the peaks of many."""
    rng = np.random.default_rng(40 + kind)
    K = gas.capi
    for n in (1, 37):
        s = ref.draw_settings(rng, n, K)
        x = rng.uniform(-1, 1, (6, n, 512, 2)).astype(np.float32)
        got = {}
        for F in (512, 256):
            with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
                _reserve(ctx, (kind,), n)
                slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (kind,))
                ctx.params_publish_batch(slots, _params(n, F))
                ctx.fx_mod_settings_publish(slots, s)
                mixes, peaks = [], []
                for b in range(6):
                    for h in range(512 // F):
                        m, p = ctx.process_block(x[b][:, h * F : (h + 1) * F], slots)
                        mixes.append(m[0])
                        peaks.append(p)
                got[F] = (np.concatenate(mixes), np.stack(peaks))
        p256 = got[256][1].reshape(6, 2, n, 2).max(axis=1)
        np.testing.assert_array_equal(got[512][1], p256)
        if n == 1:
            np.testing.assert_array_equal(got[512][0], got[256][0])


@pytest.mark.parametrize(
    "chain,frames",
    [
        ((CHORUS, HRTF), 512),
        ((PHASER, EQ10), 256),
        ((DELAY, CHORUS, REVERB), 256),
        ((CHORUS, CHORUS), 512),
        ((COMP, PHASER, AMP), 128),
        ((PHASER, ER, HRTF), 256),
    ],
)
def test_mixed_chains_next_to_fused_chains(gas, ob, chain, frames):
    """The chain's playbacks share callbacks with fused [HRTF] and [HIGHSHELF] playbacks; mix and peaks of all."""
    from godot_audio_spatializer_amd import synth

    n, nf = 24, 10
    rng = np.random.default_rng(len(chain) * 13 + frames + chain[0])
    ring = 4096 if ER in chain else 0
    hrir = _hrir()
    with gas.SpatializerContext(max_sources=n + 2 * nf, frames=frames, er_ring_frames=ring) as ctx:
        _reserve(ctx, chain, n)
        ctx.hrtf_load(hrir)
        a = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        h = ctx.source_alloc_many(nf, gas.capi.KIND_EFFECT, (HRTF,))
        s_ = ctx.source_alloc_many(nf, gas.capi.KIND_EFFECT, (HS,))
        slots = np.concatenate([a, h, s_])
        order = rng.permutation(len(slots))
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring)
        rh = ob.BatchOracle(ob.KIND_EFFECT, nf, frames, chain=(HRTF,), hrir=hrir, er_ring_frames=1)
        rs = ob.BatchOracle(ob.KIND_EFFECT, nf, frames, chain=(HS,), hrir=None, er_ring_frames=1)
        settings = gas.capi.fx_mod_settings_defaults(n)
        for b in range(5):
            if b % 3 == 0:
                p = synth.draw_params(rng, len(slots), dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            if b in (1, 3):
                settings = ref.draw_settings(rng, n, gas.capi)
                ctx.fx_mod_settings_publish(a, settings)
            src = synth.draw_sources(rng, len(slots), frames)
            mix, peaks = ctx.process_block(src[order], slots[order])
            w0, p0, _ = r.block(p[:n], src[:n], settings)
            _, p1, w1 = rh.block(p[n : n + nf].astype(ob.PARAMS_DTYPE), src[n : n + nf], want64=True)
            _, p2, w2 = rs.block(p[n + nf :].astype(ob.PARAMS_DTYPE), src[n + nf :], want64=True)
            want = w0 + w1[0] + w2[0]
            assert rel_rms(mix[0], want) <= TOL, f"{chain} block {b}: {rel_rms(mix[0], want)}"
            rpeaks = np.concatenate([p0, p1, p2])[order]
            np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=f"block {b}")


def test_chorus_two_instances_hold_independent_lines(gas, ob):
    """[CHORUS, CHORUS]: each position reads its own settings and its own line (rows bitwise those of the restatement)."""
    run_chain(gas, ob, (CHORUS, CHORUS), 12, 256, blocks=5, seed=77)


def test_chorus_hrtf_peaks_draining_only(gas, ob):
    """[CHORUS, HRTF] under GAS_FLAG_PEAKS_DRAINING_ONLY: +inf for the playbacks that are not draining, the exact peak
    for the draining ones."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F = 40, 512
    rng = np.random.default_rng(21)
    hrir = _hrir()
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PEAKS_DRAINING_ONLY) as ctx:
        ctx.reserve_fx_mod(n, 0)
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (CHORUS, HRTF))
        draining = np.arange(n) % 5 == 2
        for s in slots[draining]:
            ctx.source_set_draining(int(s), True)
        r = ChainRef(ob, (CHORUS, HRTF), n, F, hrir=hrir)
        settings = ref.draw_settings(rng, n, K)
        ctx.fx_mod_settings_publish(slots, settings)
        p = synth.draw_params(rng, n, dirs=32, frames=F)
        ctx.params_publish_batch(slots, p)
        for b in range(3):
            src = synth.draw_sources(rng, n, F)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks, _ = r.block(p, src, settings)
            assert rel_rms(mix[0], want) <= TOL
            assert np.isinf(peaks[~draining]).all() and (peaks[~draining] > 0).all()
            np.testing.assert_allclose(peaks[draining], rpeaks[draining], rtol=2e-5, atol=1e-7)


def test_invalid_settings_are_refused_with_nothing_taken(gas):
    K = gas.capi
    F = 128
    with gas.SpatializerContext(max_sources=3, frames=F) as ctx:
        ctx.reserve_fx_mod(1, 1)
        slots = np.array([ctx.source_alloc(K.KIND_EFFECT, (CHORUS,)), ctx.source_alloc(K.KIND_EFFECT, (PHASER,))], np.uint32)
        ctx.params_publish_batch(slots, _params(2, F))
        bad = [
            ("chorus_voice_count", (0,), 0),
            ("chorus_voice_count", (3,), 5),
            ("chorus_dry", (1,), 1.5),
            ("chorus_wet", (2,), -0.1),
            ("chorus_delay_ms", (0, 3), 50.5),
            ("chorus_rate_hz", (3, 2), 0.05),
            ("chorus_depth_ms", (1, 1), 21.0),
            ("chorus_level_db", (0, 0), np.nan),
            ("chorus_cutoff_hz", (2, 3), 0.5),
            ("chorus_pan", (3, 3), np.inf),
            ("phaser_range_min_hz", (0,), 9.0),
            ("phaser_range_max_hz", (3,), 10001.0),
            ("phaser_rate_hz", (1,), 21.0),
            ("phaser_feedback", (2,), 0.95),
            ("phaser_depth", (0,), -np.inf),
        ]
        for field, idx, value in bad:
            s = K.fx_mod_settings_defaults(2)
            s["chorus_wet"][0, 0] = 0.25  # a valid change on the first row: must not be taken either
            s[field][(1,) + idx] = value
            with pytest.raises(gas.GasError) as ei:
                ctx.fx_mod_settings_publish(slots, s)
            assert ei.value.status == BAD_ARG, (field, idx, value)
        edge = K.fx_mod_settings_defaults(2)
        edge["chorus_voice_count"][:] = (1, 4, 1, 4)
        edge["chorus_delay_ms"][:, :, 0] = 0.0
        edge["chorus_delay_ms"][:, :, 1] = 50.0
        edge["chorus_cutoff_hz"][:, :, 2] = 20500.0
        edge["phaser_range_min_hz"] = 10000.0  # min > max is legal
        edge["phaser_range_max_hz"] = 10.0
        ctx.fx_mod_settings_publish(slots, edge)
        d = K.fx_mod_settings_defaults(2)
        ctx.fx_mod_settings_publish(slots, d)
        st = [ref.ChorusStage(0, 1), ref.PhaserStage(0, 1)]
        rng = np.random.default_rng(1)
        for _ in range(3):
            src = rng.uniform(-1, 1, (2, F, 2)).astype(np.float32)
            _, peaks = ctx.process_block(src, slots)
            want = np.concatenate([np.abs(t.block(src[k : k + 1], d[k : k + 1])).max(axis=1) for k, t in enumerate(st)])
            _close_peaks(peaks, want, "defaults")
        for chain in ((CHORUS, 15), (DELAY, 15), (PHASER, 10)):
            with pytest.raises(gas.GasError):
                ctx.source_alloc(K.KIND_EFFECT, chain)  # 10 and 15 are no effect kinds


# ---------------------------------------------------------------------------------------------------------------- pool
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
    z = lambda: ctx.process_block(np.zeros((0, F, 2), np.float32), np.zeros(0, np.uint32))  # noqa: E731
    with gas.SpatializerContext(max_sources=10, frames=F) as ctx:
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS,)) == UNSUPPORTED  # no pool reserved
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (HS, PHASER)) == UNSUPPORTED
        ctx.reserve_fx_lines(1, 0)  # the other pools are not these
        ctx.reserve_fx_eq(1)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY, CHORUS)) == UNSUPPORTED
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ6, PHASER)) == UNSUPPORTED
        ctx.reserve_fx_mod(2, 1)
        a = ctx.source_alloc(K.KIND_EFFECT, (CHORUS,))
        b = ctx.source_alloc(K.KIND_EFFECT, (CHORUS, PHASER))
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS,)) == OUT_OF_SLOTS  # lines exhausted
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (PHASER,)) == OUT_OF_SLOTS  # banks exhausted
        assert _free_slots(gas, ctx) == 8  # nothing was taken by the refused calls
        assert _status(gas, ctx.reserve_fx_mod, 4, 4) == BAD_ARG  # lines and banks are held
        ctx.reserve_fx_lines(0, 0)  # ... which does not stop the other pools from being released
        ctx.reserve_fx_eq(0)
        ctx.reserve_fx_lines(1, 0)
        ctx.reserve_fx_eq(1)
        ctx.source_free(a)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS,)) == OUT_OF_SLOTS  # back at the next block only
        assert _status(gas, ctx.reserve_fx_mod, 4, 4) == BAD_ARG
        z()
        d = ctx.source_alloc(K.KIND_EFFECT, (DELAY,))  # the only delay line
        e = ctx.source_alloc(K.KIND_EFFECT, (EQ6,))  # the only EQ bank
        # short in exactly one of the four pools: nothing taken in the others
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS, DELAY)) == OUT_OF_SLOTS
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS, EQ10)) == OUT_OF_SLOTS
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS, CHORUS)) == OUT_OF_SLOTS
        ctx.source_free(b)
        z()
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS, PHASER, PHASER)) == OUT_OF_SLOTS  # one bank only
        c = ctx.source_alloc(K.KIND_EFFECT, (CHORUS, CHORUS))  # so both lines are still free
        f = ctx.source_alloc(K.KIND_EFFECT, (PHASER,))  # and the bank
        for s in (c, d, e, f):
            ctx.source_free(s)
        z()
        assert _status(gas, ctx.reserve_fx_lines, 2, 0) == 0  # all free: each re-sized independently
        ctx.reserve_fx_mod(0, 3)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS,)) == OUT_OF_SLOTS  # a pool of 0 lines
        ctx.source_alloc(K.KIND_EFFECT, (PHASER, PHASER, PHASER))
        held = ctx.source_alloc(K.KIND_EFFECT, (DELAY,))
        assert _status(gas, ctx.reserve_fx_lines, 0, 0) == BAD_ARG  # a line is held, whatever the banks do
        ctx.source_free(held)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_fx_mod(4, 4)
        ctx.reserve_fx_mod(0, 0)  # released
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (PHASER,)) == UNSUPPORTED


def test_reserve_refused_at_a_mix_rate_too_low(gas):
    """R = 512 at 2 kHz: below lrint(0.05 sr) + 2 (int)(0.02 sr) + 12 + 512, but enough for 128 frames; phaser banks
    need no ring."""
    with gas.SpatializerContext(max_sources=2, frames=512, mix_rate=2000.0) as ctx:
        assert _status(gas, ctx.reserve_fx_mod, 1, 0) == BAD_ARG
        assert _status(gas, ctx.reserve_fx_mod, 0, 1) == 0
    with gas.SpatializerContext(max_sources=2, frames=128, mix_rate=2000.0) as ctx:
        assert _status(gas, ctx.reserve_fx_mod, 1, 1) == 0


def _render(gas, chain, srcs, settings, slot_prep=None):
    """A fresh context's output for one playback of `chain` over srcs; slot_prep(ctx, p) may run a different history."""
    from godot_audio_spatializer_amd import synth

    F = srcs[0].shape[1]
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_fx_mod(*_mods(chain, 4))
        p = synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F)
        slot = ctx.source_alloc(gas.capi.KIND_EFFECT, chain) if slot_prep is None else slot_prep(ctx, p)
        ctx.params_publish(slot, p[0])
        ctx.fx_mod_settings_publish(np.array([slot], np.uint32), settings)
        return np.stack([ctx.process_block(x, np.array([slot], np.uint32))[0] for x in srcs])


@pytest.mark.parametrize("how", ["recycled", "reset", "reset_many"])
def test_recycled_or_reset_state_is_bitwise_fresh(gas, how):
    """A loud history, then the slot and its line and bank recycled (free, block, alloc) or gas_source_reset (once, or
    many times before the next block): the next playback equals a fresh context's bit for bit."""
    K = gas.capi
    F = 256
    chain = (PHASER, CHORUS)
    rng = np.random.default_rng(31)
    s = ref.draw_settings(rng, 1, K)
    srcs = [rng.uniform(-1, 1, (1, F, 2)).astype(np.float32) for _ in range(4)]

    def prep(ctx, p):
        slot = ctx.source_alloc(K.KIND_EFFECT, chain)
        ctx.params_publish(slot, p[0])
        ctx.fx_mod_settings_publish(np.array([slot], np.uint32), s)
        for _ in range(6):
            ctx.process_block(rng.uniform(-1, 1, (1, F, 2)).astype(np.float32), np.array([slot], np.uint32))
        if how.startswith("reset"):
            for _ in range(1 if how == "reset" else 5):
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


def test_buses_with_mod_kinds(gas):
    from godot_audio_spatializer_amd import synth

    F, n = 256, 30
    rng = np.random.default_rng(10)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_mod(n, n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (PHASER, CHORUS))
        p = synth.draw_params(rng, n, dirs=8, frames=F)
        ctx.params_publish_batch(slots, p)
        s = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_mod_settings_publish(slots, s)
        routes = gas.capi.bus_routes(n)
        routes["dry_bus"] = np.where(np.arange(n) % 3 == 0, 1, 0)
        routes["send_bus"] = np.where(np.arange(n) % 3 == 0, 0, 1)
        routes["send"] = rng.uniform(0, 1, (n, 1, 1)).astype(np.float32) * np.ones((4, 2), np.float32)
        ctx.bus_routes_publish(slots, routes)
        ph, ch = ref.PhaserStage(0, n), ref.ChorusStage(1, n)
        for b in range(4):
            src = synth.draw_sources(rng, n, F)
            out, peaks = ctx.process_block_buses(src, slots, 2)
            y = ch.block(ph.block(src, s), s).astype(np.float64)
            for bus in range(2):
                w = (routes["dry_bus"] == bus).astype(np.float64) + (routes["send_bus"] == bus) * routes["send"][:, 0, 0].astype(np.float64)
                want = (y * w[:, None, None]).sum(axis=0)
                assert rel_rms(out[bus, 0], want) <= TOL, f"block {b} bus {bus}"
            np.testing.assert_allclose(peaks, np.abs(y).max(axis=1), rtol=2e-5, atol=1e-7)


def test_process_frames_1_matches_the_batched_row_bitwise(gas):
    from godot_audio_spatializer_amd import synth

    F = 256
    rng = np.random.default_rng(11)
    chain = (CHORUS, PHASER)
    s = ref.draw_settings(rng, 1, gas.capi)
    srcs = [synth.draw_sources(rng, 1, F) for _ in range(4)]
    outs = []
    for single in (False, True):
        with gas.SpatializerContext(max_sources=2, frames=F) as ctx:
            ctx.reserve_fx_mod(2, 2)
            slots = ctx.source_alloc_many(1, gas.capi.KIND_EFFECT, chain)
            ctx.params_publish_batch(slots, synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F))
            ctx.fx_mod_settings_publish(slots, s)
            got = [ctx.process_frames_1(int(slots[0]), x[0]) if single else ctx.process_block(x, slots)[0][0] for x in srcs]
            outs.append(np.stack(got))
    np.testing.assert_array_equal(outs[0], outs[1])


def test_host_layer_queues_mod_settings(gas):
    """BatchedSpatializerHost + gas_host_set_effect_settings_mod: one playback through [CHORUS, PHASER] equals the
    reference applied to what the same host delivers for an empty chain."""
    K = gas.capi
    F = 256
    rng = np.random.default_rng(12)
    stream = rng.uniform(-0.8, 0.8, (F * 20, 2)).astype(np.float32)
    from godot_audio_spatializer_amd import synth

    params = synth.draw_params(rng, 1, dirs=8, frames=F)
    new = ref.draw_settings(rng, 1, K)
    got = {}
    for chain in ((CHORUS, PHASER), ()):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_fx_mod(2, 2)
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, chain)
            pid = host.start_playback_array(stream)
            host.set_spatializer_parameters(pid, params[0])
            outs = []
            for cb in range(8):
                if cb == 3 and chain:
                    assert host.set_effect_settings_mod(pid, new) == 0
                    bad = new.copy()
                    bad["chorus_voice_count"][0, 3] = 7
                    assert host.set_effect_settings_mod(pid, bad) == BAD_ARG  # refused when queued
                rc, out = host.get_mixed_frames(0, F)
                assert rc == 0
                outs.append(out.copy())
            host.close()
        got[chain] = np.stack(outs)
    window = got[()]
    ch, ph = ref.ChorusStage(0, 1), ref.PhaserStage(1, 1)
    d = K.fx_mod_settings_defaults(1)
    for cb in range(8):
        s = new if cb >= 3 else d
        y = ph.block(ch.block(window[cb][None], s), s)[0]
        assert rel_rms(got[(CHORUS, PHASER)][cb], y) <= TOL, f"callback {cb}"


def test_two_runs_are_bitwise_equal(gas, ob):
    a, _ = run_chain(gas, ob, (CHORUS, PHASER), 70, 512, blocks=3, seed=5, check=False)
    b, _ = run_chain(gas, ob, (CHORUS, PHASER), 70, 512, blocks=3, seed=5, check=False)
    np.testing.assert_array_equal(a, b)
