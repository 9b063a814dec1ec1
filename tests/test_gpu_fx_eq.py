"""GAS_FX_EQ6 / _EQ10 / _EQ21 on the GPU (k_fx_eq.hip) against the numpy restatement tests/fx_eq_ref.py, composed with
the oracle's existing kinds (oracle.binding.BatchOracle), tests/fx_dyn_ref.py and tests/fx_line_ref.py for mixed chains;
and the bank pool's lifecycle (gas_ctx_reserve_fx_eq).

The kernel runs every band in the engine's order with separate f32 operations, as the restatement does, so a source's
rows -- and with them its peak -- are bitwise the restatement's; the mix is compared within TOL because the library
sums the sources in f32 in its own order and the reference in f64."""
import numpy as np
import pytest

import fx_dyn_ref
import fx_eq_ref as ref
import fx_line_ref
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HS, ER, HRTF, LP, AMP = 1, 2, 3, 4, 9
DIST, COMP = 11, 12
DELAY, REVERB = 13, 14
EQ6, EQ10, EQ21 = 16, 17, 18
EQS = (EQ6, EQ10, EQ21)
BAD_ARG, OUT_OF_SLOTS, UNSUPPORTED = -1, -2, -6


def _hrir(dirs=32, seed=5):
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(seed), dirs=dirs)


def _capi():
    from godot_audio_spatializer_amd import capi

    return capi


class ChainRef:
    """A playback chain's reference: runs of the existing kinds through BatchOracle (one source per oracle where a new
    kind follows, for its rows; all sources in one oracle for a last run), the equalisers through fx_eq_ref, the
    dynamics and line kinds through fx_dyn_ref / fx_line_ref on their resource defaults."""

    def __init__(self, ob, chain, n, frames, hrir=None, ring=0, mix_rate=48000.0):
        self.stages = []
        segs = []
        own_kinds = EQS + (DIST, COMP, DELAY, REVERB)
        for j, k in enumerate(chain):
            own = k in own_kinds
            if segs and not own and not segs[-1][0]:
                segs[-1][1].append(j)
            else:
                segs.append((own, [j]))
        for si, (own, pos) in enumerate(segs):
            k0 = chain[pos[0]]
            if k0 in EQS:
                self.stages.append(("eq", ref.EqStage(k0, pos[0], n, mix_rate)))
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
            if kind == "eq":
                x = obj.block(x, settings)
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


def _eqs(chain, n):
    return n * sum(k in EQS for k in chain)


def _lines(chain, n):
    return n * sum(k == DELAY for k in chain), n * sum(k == REVERB for k in chain)


def run_chain(gas, ob, chain, n, frames, blocks=4, seed=0, mix_rate=48000.0, check=True, bitwise=True):
    """Random gains over the whole range, re-published at blocks 1 and 3 (all, then half the sources).  Returns the
    last mix."""
    from godot_audio_spatializer_amd import synth

    rng = np.random.default_rng(seed)
    ring = 4096 if ER in chain else 0
    hrir = _hrir() if HRTF in chain else None
    with gas.SpatializerContext(max_sources=n + 3, frames=frames, er_ring_frames=ring, mix_rate=mix_rate) as ctx:
        ctx.reserve_fx_eq(_eqs(chain, n))
        if DELAY in chain or REVERB in chain:
            ctx.reserve_fx_lines(*_lines(chain, n))
        if hrir is not None:
            ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring, mix_rate=mix_rate)
        settings = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_eq_settings_publish(slots, settings)
        for b in range(blocks):
            if b % 3 == 0:
                p = synth.draw_params(rng, n, dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            if b in (1, 3):
                who = np.arange(n) if b == 1 else rng.choice(n, max(1, n // 2), replace=False)
                new = ref.draw_settings(rng, len(who), gas.capi)
                ctx.fx_eq_settings_publish(slots[who], new)
                settings[who] = new
            src = synth.draw_sources(rng, n, frames)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks, rows = r.block(p, src, settings)
            if check:
                assert rel_rms(mix[0], want) <= TOL, f"{chain} n={n} F={frames} block {b}: {rel_rms(mix[0], want)}"
                np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=f"block {b}")
                if bitwise and rows is not None:
                    np.testing.assert_array_equal(peaks, rpeaks, err_msg=f"block {b}: rows are not the restatement's bits")
    return mix


NF = [(1, 128), (31, 256), (256, 512), (31, 128), (256, 256), (1, 512)]


@pytest.mark.parametrize("kind", EQS)
@pytest.mark.parametrize("n,frames", NF)
def test_alone(gas, ob, kind, n, frames):
    run_chain(gas, ob, (kind,), n, frames, seed=kind * 7 + n + frames)


@pytest.mark.parametrize("kind", EQS)
def test_alone_8192(gas, ob, kind):
    run_chain(gas, ob, (kind,), 8192, 512, blocks=3, seed=kind)


@pytest.mark.parametrize("kind", EQS)
def test_alone_at_44100(gas, ob, kind):
    """EQ21's 22 kHz band at 44.1 kHz has the longest recurrence (pole radius 0.99989)."""
    run_chain(gas, ob, (kind,), 40, 256, mix_rate=44100.0, seed=kind + 1)


def test_mixed_ranges_in_one_callback(gas, ob):
    """EQ6, EQ10 and EQ21 playbacks interleaved in one callback's list: each its own run of the staged chain."""
    from godot_audio_spatializer_amd import synth

    F, per = 256, 20
    rng = np.random.default_rng(4)
    with gas.SpatializerContext(max_sources=3 * per, frames=F) as ctx:
        ctx.reserve_fx_eq(3 * per)
        groups = [ctx.source_alloc_many(per, gas.capi.KIND_EFFECT, (k,)) for k in EQS]
        slots = np.concatenate(groups)
        order = rng.permutation(len(slots))
        stages = [ref.EqStage(k, 0, per) for k in EQS]
        sets = [ref.draw_settings(rng, per, gas.capi) for _ in EQS]
        for g, s in zip(groups, sets):
            ctx.fx_eq_settings_publish(g, s)
        ctx.params_publish_batch(slots, synth.draw_params(rng, len(slots), dirs=8, frames=F))
        for b in range(4):
            src = synth.draw_sources(rng, len(slots), F)
            mix, peaks = ctx.process_block(src[order], slots[order])
            ys = [st.block(src[i * per : (i + 1) * per], s) for i, (st, s) in enumerate(zip(stages, sets))]
            y = np.concatenate(ys)
            assert rel_rms(mix[0], y.astype(np.float64).sum(axis=0)) <= TOL, f"block {b}"
            np.testing.assert_array_equal(peaks, np.abs(y).max(axis=1)[order])


@pytest.mark.parametrize(
    "chain,frames",
    [
        ((EQ10, HRTF), 512),
        ((LP, EQ21), 256),
        ((HS, EQ6, AMP), 128),
        ((ER, EQ10, HRTF), 256),
        ((EQ6, EQ21), 512),
        ((EQ6, DIST, REVERB), 256),
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
        ctx.reserve_fx_eq(_eqs(chain, n))
        if REVERB in chain:
            ctx.reserve_fx_lines(*_lines(chain, n))
        ctx.hrtf_load(hrir)
        a = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        h = ctx.source_alloc_many(nf, gas.capi.KIND_EFFECT, (HRTF,))
        s_ = ctx.source_alloc_many(nf, gas.capi.KIND_EFFECT, (HS,))
        slots = np.concatenate([a, h, s_])
        order = rng.permutation(len(slots))
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring)
        rh = ob.BatchOracle(ob.KIND_EFFECT, nf, frames, chain=(HRTF,), hrir=hrir, er_ring_frames=1)
        rs = ob.BatchOracle(ob.KIND_EFFECT, nf, frames, chain=(HS,), hrir=None, er_ring_frames=1)
        settings = gas.capi.fx_eq_settings_defaults(n)
        for b in range(5):
            if b % 3 == 0:
                p = synth.draw_params(rng, len(slots), dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            if b in (1, 3):
                # Behind the early reflections the gains stay within -6 .. 6 dB.  The oracle's ER rows differ from the
                # kernel's in the last bit, and an EQ scales that relative difference by up to its gain spread between
                # bands: with the full range it reached 1.5e-5 of the mix, with -30 .. 12 dB 5e-5 of one peak
                # (measured).  Every other chain takes the full range.
                settings = ref.draw_settings(rng, n, gas.capi, *((-6.0, 6.0) if ER in chain else ()))
                ctx.fx_eq_settings_publish(a, settings)
            src = synth.draw_sources(rng, len(slots), frames)
            mix, peaks = ctx.process_block(src[order], slots[order])
            w0, p0, _ = r.block(p[:n], src[:n], settings)
            _, p1, w1 = rh.block(p[n : n + nf].astype(ob.PARAMS_DTYPE), src[n : n + nf], want64=True)
            _, p2, w2 = rs.block(p[n + nf :].astype(ob.PARAMS_DTYPE), src[n + nf :], want64=True)
            want = w0 + w1[0] + w2[0]
            assert rel_rms(mix[0], want) <= TOL, f"{chain} block {b}: {rel_rms(mix[0], want)}"
            rpeaks = np.concatenate([p0, p1, p2])[order]
            np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=f"block {b}")


def test_long_run_sine_at_the_22hz_band(gas):
    """A sine at EQ21's 22 Hz band, 48 kHz, 200 blocks of 512, gains at 0 dB: every block within TOL of the restatement
    (in fact its bits), the steady state equals sum_k H_k(e^{jw}) within 5e-4, and its amplitude does not drift.

    The bound is the f32 recurrence's own: with poles at radius 0.9994 its rounding bias moves the fitted amplitude of a
    20-block window by about +-1.2e-4 around a point 2e-4 off the exact response (the restatement does the same,
    tests/test_fx_eq_reference.py), so drift is judged on the mean over windows early and late in the run."""
    F, blocks, sr = 512, 200, 48000.0
    w = 2.0 * np.pi * 22.0 / np.float64(np.float32(sr))
    t = np.arange(F * blocks)
    x = np.sin(w * t).astype(np.float32)
    x = np.stack([x, -0.5 * x], axis=1)
    st = ref.EqStage(EQ21, 0, 1, sr)
    s = _capi().fx_eq_settings_defaults(1)
    with gas.SpatializerContext(max_sources=1, frames=F, mix_rate=sr) as ctx:
        ctx.reserve_fx_eq(1)
        slot = ctx.source_alloc(gas.capi.KIND_EFFECT, (EQ21,))
        ctx.params_publish(slot, _params(1, F)[0])
        got = []
        for b in range(blocks):
            blk = x[b * F : (b + 1) * F][None]
            mix, _ = ctx.process_block(blk, np.array([slot], np.uint32))
            y = st.block(blk, s)[0]
            assert rel_rms(mix[0], y.astype(np.float64)) <= TOL, f"block {b}"
            got.append(mix[0])
    y = np.concatenate(got)
    c1, c2, c3, _ = ref.coefficients(EQ21, sr)
    H = ref.response(c1, c2, c3, w).sum()
    for ear, scale in ((0, 1.0), (1, -0.5)):
        amps = []
        for lo in range(40, 200, 20):
            tail = np.arange(lo * F, (lo + 20) * F)
            basis = np.stack([np.sin(w * tail), np.cos(w * tail)], axis=1)
            (a, b), *_ = np.linalg.lstsq(basis, y[tail, ear].astype(np.float64) / scale, rcond=None)
            assert abs((a + 1j * b) - H) <= 5e-4, (lo, ear, a + 1j * b, H)
            amps.append(abs(a + 1j * b))
        assert abs(np.mean(amps[-3:]) - np.mean(amps[:3])) <= 1e-4, amps  # no drift


def test_latest_settings_win_without_a_ramp(gas):
    """Two publications before a block: the later one is what the block uses, in full from its first frame."""
    F, n = 256, 8
    rng = np.random.default_rng(8)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_eq(n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (EQ10,))
        ctx.params_publish_batch(slots, _params(n, F))
        st = ref.EqStage(EQ10, 0, n)
        s = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_eq_settings_publish(slots, s)
        for b in range(4):
            if b == 2:
                ctx.fx_eq_settings_publish(slots, ref.draw_settings(rng, n, gas.capi))
                s = ref.draw_settings(rng, n, gas.capi, lo=-6.0, hi=24.0)
                ctx.fx_eq_settings_publish(slots, s)
            src = rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)
            _, peaks = ctx.process_block(src, slots)
            np.testing.assert_array_equal(peaks, np.abs(st.block(src, s)).max(axis=1), err_msg=f"block {b}")


def test_invalid_settings_are_refused_with_nothing_taken(gas):
    K = gas.capi
    F = 128
    with gas.SpatializerContext(max_sources=3, frames=F) as ctx:
        ctx.reserve_fx_eq(2)
        slots = ctx.source_alloc_many(2, K.KIND_EFFECT, (EQ6,))
        ctx.params_publish_batch(slots, _params(2, F))
        for value in (np.nan, np.inf, -np.inf, -60.5, 24.5):
            for j, k in ((0, 2), (0, 15), (3, 20)):  # a used band, an unused band, an unused position
                s = K.fx_eq_settings_defaults(2)
                s["band_gain_db"][0, 0, 1] = -20.0  # a valid change on the first row: must not be taken either
                s["band_gain_db"][1, j, k] = value
                with pytest.raises(gas.GasError) as ei:
                    ctx.fx_eq_settings_publish(slots, s)
                assert ei.value.status == BAD_ARG, (value, j, k)
        edge = K.fx_eq_settings_defaults(2)
        edge["band_gain_db"][:, :, 0] = -60.0
        edge["band_gain_db"][:, :, 1] = 24.0
        ctx.fx_eq_settings_publish(slots, edge)  # the range's ends are legal
        ctx.fx_eq_settings_publish(slots, K.fx_eq_settings_defaults(2))
        st = ref.EqStage(EQ6, 0, 2)
        d = K.fx_eq_settings_defaults(2)
        rng = np.random.default_rng(1)
        for _ in range(3):
            src = rng.uniform(-1, 1, (2, F, 2)).astype(np.float32)
            _, peaks = ctx.process_block(src, slots)
            np.testing.assert_array_equal(peaks, np.abs(st.block(src, d)).max(axis=1))
        with pytest.raises(gas.GasError):
            ctx.source_alloc(K.KIND_EFFECT, (EQ6, 15))  # 15 is no effect kind


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
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F = 128
    with gas.SpatializerContext(max_sources=8, frames=F) as ctx:
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ6,)) == UNSUPPORTED  # no pool reserved
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (HS, EQ21)) == UNSUPPORTED
        ctx.reserve_fx_lines(1, 0)  # the line pools are not the bank pool
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY, EQ10)) == UNSUPPORTED
        ctx.reserve_fx_eq(3)
        a = ctx.source_alloc(K.KIND_EFFECT, (EQ6,))
        b = ctx.source_alloc(K.KIND_EFFECT, (EQ10, EQ21))
        ctx.params_publish(b, synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F)[0])
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ6,)) == OUT_OF_SLOTS  # banks exhausted
        assert _free_slots(gas, ctx) == 6  # nothing was taken by the refused call
        assert _status(gas, ctx.reserve_fx_eq, 8) == BAD_ARG  # banks are held
        ctx.reserve_fx_lines(0, 0)  # ... which does not stop the line pools from being released
        ctx.reserve_fx_lines(1, 0)
        ctx.source_free(a)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ6,)) == OUT_OF_SLOTS  # back at the next block only
        assert _status(gas, ctx.reserve_fx_eq, 8) == BAD_ARG
        ctx.process_block(np.zeros((1, F, 2), np.float32), np.array([b], np.uint32))
        d = ctx.source_alloc(K.KIND_EFFECT, (DELAY,))  # the only line
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ6, DELAY)) == OUT_OF_SLOTS  # a bank, but no line: all or nothing
        c = ctx.source_alloc(K.KIND_EFFECT, (EQ6,))  # so the bank is still free
        for s in (b, c, d):
            ctx.source_free(s)
        ctx.process_block(np.zeros((0, F, 2), np.float32), np.zeros(0, np.uint32))
        assert _status(gas, ctx.reserve_fx_lines, 2, 0) == 0  # lines free, banks free: both re-sized independently
        ctx.reserve_fx_eq(2)
        ctx.source_alloc(K.KIND_EFFECT, (EQ6, EQ6))
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ6,)) == OUT_OF_SLOTS
        held = ctx.source_alloc(K.KIND_EFFECT, (DELAY,))
        assert _status(gas, ctx.reserve_fx_lines, 0, 0) == BAD_ARG  # a line is held, whatever the banks do
        ctx.source_free(held)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_fx_eq(4)
        ctx.reserve_fx_eq(0)  # released
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ21,)) == UNSUPPORTED


def _render(gas, chain, srcs, settings, slot_prep=None):
    """A fresh context's output for one playback of `chain` over srcs; slot_prep(ctx, p) may run a different history."""
    from godot_audio_spatializer_amd import synth

    F = srcs[0].shape[1]
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_fx_eq(4 * _eqs(chain, 1))
        p = synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F)
        slot = ctx.source_alloc(gas.capi.KIND_EFFECT, chain) if slot_prep is None else slot_prep(ctx, p)
        ctx.params_publish(slot, p[0])
        ctx.fx_eq_settings_publish(np.array([slot], np.uint32), settings)
        return np.stack([ctx.process_block(x, np.array([slot], np.uint32))[0] for x in srcs])


@pytest.mark.parametrize("how", ["recycled", "reset", "reset_many"])
def test_recycled_or_reset_bank_is_bitwise_fresh(gas, how):
    """A loud history, then the slot and its banks recycled (free, block, alloc) or gas_source_reset (once, or many
    times before the next block): the next playback equals a fresh context's bit for bit."""
    K = gas.capi
    F = 256
    chain = (EQ21, EQ6)
    rng = np.random.default_rng(31)
    s = ref.draw_settings(rng, 1, K, lo=0.0, hi=24.0)
    srcs = [rng.uniform(-1, 1, (1, F, 2)).astype(np.float32) for _ in range(4)]

    def prep(ctx, p):
        slot = ctx.source_alloc(K.KIND_EFFECT, chain)
        ctx.params_publish(slot, p[0])
        ctx.fx_eq_settings_publish(np.array([slot], np.uint32), s)
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


def test_reset_of_every_slot_of_a_full_pool(gas):
    """Every bank of a full pool in use, a loud history, then every slot reset: the next blocks equal a fresh pool's."""
    K = gas.capi
    F, n = 128, 12
    rng = np.random.default_rng(32)
    s = ref.draw_settings(rng, n, K)
    srcs = [rng.uniform(-1, 1, (n, F, 2)).astype(np.float32) for _ in range(3)]
    outs = []
    for history in (False, True):
        with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
            ctx.reserve_fx_eq(2 * n)
            slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (EQ10, EQ21))
            ctx.params_publish_batch(slots, _params(n, F))
            ctx.fx_eq_settings_publish(slots, s)
            if history:
                for _ in range(4):
                    ctx.process_block(rng.uniform(-1, 1, (n, F, 2)).astype(np.float32), slots)
                for sl in slots:
                    ctx.source_reset(int(sl))
            outs.append(np.stack([ctx.process_block(x, slots)[1] for x in srcs]))
    np.testing.assert_array_equal(outs[1], outs[0])


def test_buses_with_eq_kinds(gas):
    from godot_audio_spatializer_amd import synth

    F, n = 256, 30
    rng = np.random.default_rng(10)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_eq(n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (EQ21,))
        p = synth.draw_params(rng, n, dirs=8, frames=F)
        ctx.params_publish_batch(slots, p)
        s = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_eq_settings_publish(slots, s)
        routes = gas.capi.bus_routes(n)
        routes["dry_bus"] = np.where(np.arange(n) % 3 == 0, 1, 0)
        routes["send_bus"] = np.where(np.arange(n) % 3 == 0, 0, 1)
        routes["send"] = rng.uniform(0, 1, (n, 1, 1)).astype(np.float32) * np.ones((4, 2), np.float32)
        ctx.bus_routes_publish(slots, routes)
        st = ref.EqStage(EQ21, 0, n)
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
    chain = (EQ10, EQ6)
    s = ref.draw_settings(rng, 1, gas.capi)
    srcs = [synth.draw_sources(rng, 1, F) for _ in range(4)]
    outs = []
    for single in (False, True):
        with gas.SpatializerContext(max_sources=2, frames=F) as ctx:
            ctx.reserve_fx_eq(2)
            slots = ctx.source_alloc_many(1, gas.capi.KIND_EFFECT, chain)
            ctx.params_publish_batch(slots, synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F))
            ctx.fx_eq_settings_publish(slots, s)
            got = [ctx.process_frames_1(int(slots[0]), x[0]) if single else ctx.process_block(x, slots)[0][0] for x in srcs]
            outs.append(np.stack(got))
    np.testing.assert_array_equal(outs[0], outs[1])


def test_host_layer_queues_eq_settings(gas):
    """BatchedSpatializerHost + gas_host_set_effect_settings_eq: one playback through [EQ21] equals the reference
    applied to what the same host delivers for an empty chain."""
    K = gas.capi
    F = 256
    rng = np.random.default_rng(12)
    stream = rng.uniform(-0.8, 0.8, (F * 20, 2)).astype(np.float32)
    from godot_audio_spatializer_amd import synth

    params = synth.draw_params(rng, 1, dirs=8, frames=F)
    new = ref.draw_settings(rng, 1, K)
    got = {}
    for chain in ((EQ21,), ()):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_fx_eq(2)
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, chain)
            pid = host.start_playback_array(stream)
            host.set_spatializer_parameters(pid, params[0])
            outs = []
            for cb in range(8):
                if cb == 3 and chain:
                    assert host.set_effect_settings_eq(pid, new) == 0
                    bad = new.copy()
                    bad["band_gain_db"][0, 3, 20] = np.nan
                    assert host.set_effect_settings_eq(pid, bad) == BAD_ARG  # refused when queued
                rc, out = host.get_mixed_frames(0, F)
                assert rc == 0
                outs.append(out.copy())
            host.close()
        got[chain] = np.stack(outs)
    window = got[()]
    st = ref.EqStage(EQ21, 0, 1)
    d = K.fx_eq_settings_defaults(1)
    for cb in range(8):
        y = st.block(window[cb][None], new if cb >= 3 else d)[0]
        assert rel_rms(got[(EQ21,)][cb], y) <= TOL, f"callback {cb}"


def test_two_runs_are_bitwise_equal(gas, ob):
    a = run_chain(gas, ob, (EQ6, EQ21), 70, 256, blocks=3, seed=5, check=False)
    b = run_chain(gas, ob, (EQ6, EQ21), 70, 256, blocks=3, seed=5, check=False)
    np.testing.assert_array_equal(a, b)


def test_eq21_hrtf_peaks_draining_only(gas, ob):
    """[EQ21, HRTF] under GAS_FLAG_PEAKS_DRAINING_ONLY: +inf for the playbacks that are not draining, the exact peak
    for the draining ones."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F = 40, 512
    rng = np.random.default_rng(21)
    hrir = _hrir()
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PEAKS_DRAINING_ONLY) as ctx:
        ctx.reserve_fx_eq(n)
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (EQ21, HRTF))
        draining = np.arange(n) % 5 == 2
        for s in slots[draining]:
            ctx.source_set_draining(int(s), True)
        r = ChainRef(ob, (EQ21, HRTF), n, F, hrir=hrir)
        settings = ref.draw_settings(rng, n, K)
        ctx.fx_eq_settings_publish(slots, settings)
        p = synth.draw_params(rng, n, dirs=32, frames=F)
        ctx.params_publish_batch(slots, p)
        for b in range(3):
            src = synth.draw_sources(rng, n, F)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks, _ = r.block(p, src, settings)
            assert rel_rms(mix[0], want) <= TOL
            assert np.isinf(peaks[~draining]).all() and (peaks[~draining] > 0).all()
            np.testing.assert_allclose(peaks[draining], rpeaks[draining], rtol=2e-5, atol=1e-7)
