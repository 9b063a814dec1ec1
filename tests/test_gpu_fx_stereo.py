"""GAS_FX_PANNER / GAS_FX_STEREO_ENHANCE / GAS_FX_LIMITER on the GPU (k_fx_stereo.hip) against the numpy restatement
tests/fx_stereo_ref.py, composed with the oracle's existing kinds (oracle.binding.BatchOracle) and
tests/fx_{dyn,mod}_ref.py for mixed chains; and the ring pool's lifecycle (gas_ctx_reserve_fx_stereo).

The kernel runs every product and sum as a separate f32 operation in the restatement's order.  Panner and stereo
enhance have no transcendental per sample and their block constants are plain IEEE f64 arithmetic, so their rows are
expected to equal the restatement's bit for bit; the limiter's per-sample log and exp are evaluated in f64 on the device,
which may differ from the host's in the last f64 bit and move an f32 result where it rounds on a tie.  The mix is
compared within TOL (relative RMS) because the library sums the sources in f32 in its own order and the reference in
f64, peaks within rtol 2e-5 / atol 1e-7 like the other effect tests; the number of bitwise-equal rows is reported."""
import numpy as np
import pytest

import fx_dyn_ref
import fx_mod_ref
import fx_stereo_ref as ref
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HS, ER, HRTF, LP, AMP = 1, 2, 3, 4, 9
DIST, COMP = 11, 12
DELAY, REVERB = 13, 14
EQ6, EQ10, EQ21 = 16, 17, 18
CHORUS, PHASER = 19, 20
PANNER, ENHANCE, LIMITER = 21, 22, 23
STEREO = (PANNER, ENHANCE, LIMITER)
BAD_ARG, OUT_OF_SLOTS, UNSUPPORTED = -1, -2, -6
PEAK_TOL = dict(rtol=2e-5, atol=1e-7)


def _hrir(dirs=32, seed=5):
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(seed), dirs=dirs)


def _capi():
    from godot_audio_spatializer_amd import capi

    return capi


class ChainRef:
    """A playback chain's reference: runs of the existing kinds through BatchOracle (one source per oracle where a new
    kind follows, for its rows; all sources in one oracle for a last run), panner / stereo enhance / limiter through
    fx_stereo_ref, chorus / phaser and distortion / compressor through their restatements on the resource defaults."""

    def __init__(self, ob, chain, n, frames, hrir=None, ring=0, mix_rate=48000.0):
        self.stages = []
        segs = []
        own_kinds = STEREO + (DIST, COMP, CHORUS, PHASER)
        for j, k in enumerate(chain):
            own = k in own_kinds
            if segs and not own and not segs[-1][0]:
                segs[-1][1].append(j)
            else:
                segs.append((own, [j]))
        for si, (own, pos) in enumerate(segs):
            k0 = chain[pos[0]]
            if k0 in STEREO:
                self.stages.append(("stereo", ref.make_stage(k0, pos[0], n, mix_rate)))
            elif k0 in (CHORUS, PHASER):
                self.stages.append(("mod", fx_mod_ref.make_stage(k0, pos[0], n, mix_rate)))
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
            if kind == "stereo":
                x = obj.block(x, settings)
            elif kind == "mod":
                x = obj.block(x, _capi().fx_mod_settings_defaults(len(x)))
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


def _reserve(ctx, chain, n):
    if ENHANCE in chain:
        ctx.reserve_fx_stereo(n * sum(k == ENHANCE for k in chain))
    if CHORUS in chain or PHASER in chain:
        ctx.reserve_fx_mod(n * sum(k == CHORUS for k in chain), n * sum(k == PHASER for k in chain))


def _blocks_to_wrap(chain, frames, mix_rate=48000.0):
    """Enough blocks for a stereo enhance's ring to wrap at least once; 4 for the stateless kinds."""
    return ref.ring_frames(mix_rate) // frames + 2 if ENHANCE in chain else 4


def run_chain(gas, ob, chain, n, frames, blocks=None, seed=0, mix_rate=48000.0, check=True, scale=1.0):
    """Random settings over the whole ranges with the edges on some sources, re-published at every block from the second
    on (all, then half the sources, alternately).  Returns the last mix and the number of sources whose peaks were
    bitwise equal, summed over the blocks."""
    from godot_audio_spatializer_amd import synth

    rng = np.random.default_rng(seed)
    ring = 4096 if ER in chain else 0
    hrir = _hrir() if HRTF in chain else None
    blocks = blocks or _blocks_to_wrap(chain, frames, mix_rate)
    equal = 0
    with gas.SpatializerContext(max_sources=n + 3, frames=frames, er_ring_frames=ring, mix_rate=mix_rate) as ctx:
        _reserve(ctx, chain, n)
        if hrir is not None:
            ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring, mix_rate=mix_rate)
        settings = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_stereo_settings_publish(slots, settings)
        for b in range(blocks):
            if b % 3 == 0:
                p = synth.draw_params(rng, n, dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            if b >= 1:
                who = np.arange(n) if b % 2 else rng.choice(n, max(1, n // 2), replace=False)
                new = ref.draw_settings(rng, len(who), gas.capi)
                ctx.fx_stereo_settings_publish(slots[who], new)
                settings[who] = new
            src = synth.draw_sources(rng, n, frames) * np.float32(scale)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks, rows = r.block(p, src, settings)
            if check:
                err = rel_rms(mix[0], want)
                assert err <= TOL, f"{chain} n={n} F={frames} block {b}: {err}"
                np.testing.assert_allclose(peaks, rpeaks, err_msg=f"{chain} block {b}", **PEAK_TOL)
                if rows is not None:
                    equal += int((peaks == rpeaks).all(axis=-1).sum())
    if check:
        print(f"{chain} n={n} F={frames}: {equal} of {n * blocks} source peaks bitwise equal over {blocks} blocks")
    return mix, equal, n * blocks


NF = [(1, 128), (31, 256), (256, 512), (64, 384), (256, 128), (1, 512)]


@pytest.mark.parametrize("kind", STEREO)
@pytest.mark.parametrize("n,frames", NF)
def test_alone(gas, ob, kind, n, frames):
    # the limiter is driven 4x louder, so that a good share of the samples takes its soft-clip branch
    _, equal, total = run_chain(gas, ob, (kind,), n, frames, seed=kind * 7 + n + frames, scale=4.0 if kind == LIMITER else 1.0)
    if kind != LIMITER:
        assert equal == total


@pytest.mark.parametrize("kind", STEREO)
def test_alone_8192(gas, ob, kind):
    _, equal, total = run_chain(gas, ob, (kind,), 8192, 512, seed=kind, scale=4.0 if kind == LIMITER else 1.0)
    if kind != LIMITER:
        assert equal == total


@pytest.mark.parametrize("kind", STEREO)
def test_alone_at_other_rates(gas, ob, kind):
    for sr, F in ((44100.0, 256), (96000.0, 512)):
        _, equal, total = run_chain(gas, ob, (kind,), 20, F, mix_rate=sr, seed=kind + int(sr))
        if kind != LIMITER:
            assert equal == total


@pytest.mark.parametrize("kind", STEREO)
@pytest.mark.parametrize("F,sr", [(512, 48000.0), (128, 48000.0), (384, 44100.0), (256, 96000.0)])
def test_rows_against_the_restatement_bitwise(gas, kind, F, sr):
    """Every source in a callback of its own, so the mix is that source's row: compared with the restatement's row
    sample by sample (24 sources, enough blocks for the ring to wrap, every block size and three rates).  All rows are
    expected bitwise equal for panner and stereo enhance (asserted); for the limiter the count is reported and the
    rows are held to TOL.  The tests at more sources see rows only through their peaks and the mix."""
    K = gas.capi
    n = 24
    rng = np.random.default_rng(60 + kind + F)
    blocks = _blocks_to_wrap((kind,), F, sr)
    with gas.SpatializerContext(max_sources=n, frames=F, mix_rate=sr) as ctx:
        _reserve(ctx, (kind,), n)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (kind,))
        ctx.params_publish_batch(slots, _params(n, F))
        st = ref.make_stage(kind, 0, n, sr)
        equal = 0
        for b in range(blocks):
            s = ref.draw_settings(rng, n, K)
            ctx.fx_stereo_settings_publish(slots, s)
            x = (rng.standard_normal((n, F, 2)) * (2.0 if kind == LIMITER else 0.5)).astype(np.float32)
            want = st.block(x, s)
            for k in range(n):
                mix, _ = ctx.process_block(x[k : k + 1], slots[k : k + 1])
                same = bool((mix[0] == want[k]).all())
                equal += same
                if kind != LIMITER:
                    assert same, f"kind {kind} block {b} source {k}: {np.argwhere(mix[0] != want[k])[:4]}"
                else:
                    assert rel_rms(mix[0], want[k]) <= TOL
        print(f"kind {kind} F={F} sr={sr}: {equal} of {n * blocks} rows bitwise equal")


@pytest.mark.parametrize("kind", STEREO)
def test_one_512_block_equals_two_256_blocks(gas, kind):
    """GPU only: no chunking anywhere, so one F = 512 callback equals two F = 256 callbacks bit for bit -- one source's
    output, and the peaks of many; 10 x 512 frames, so the stereo enhance's ring wraps."""
    rng = np.random.default_rng(40 + kind)
    K = gas.capi
    B = 10
    for n in (1, 37):
        s = ref.draw_settings(rng, n, K)
        x = rng.uniform(-1, 1, (B, n, 512, 2)).astype(np.float32)
        got = {}
        for F in (512, 256):
            with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
                _reserve(ctx, (kind,), n)
                slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (kind,))
                ctx.params_publish_batch(slots, _params(n, F))
                ctx.fx_stereo_settings_publish(slots, s)
                mixes, peaks = [], []
                for b in range(B):
                    for h in range(512 // F):
                        m, p = ctx.process_block(x[b][:, h * F : (h + 1) * F], slots)
                        mixes.append(m[0])
                        peaks.append(p)
                got[F] = (np.concatenate(mixes), np.stack(peaks))
        p256 = got[256][1].reshape(B, 2, n, 2).max(axis=1)
        np.testing.assert_array_equal(got[512][1], p256)
        if n == 1:
            np.testing.assert_array_equal(got[512][0], got[256][0])


@pytest.mark.parametrize(
    "chain,frames",
    [
        ((PANNER, HRTF), 512),
        ((ENHANCE, LIMITER), 256),
        ((CHORUS, ENHANCE), 256),
        ((COMP, LIMITER), 128),
        ((PANNER, ER, HRTF), 256),
        ((ENHANCE, ENHANCE), 512),
        ((LIMITER, PANNER, ENHANCE, AMP), 384),
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
        settings = gas.capi.fx_stereo_settings_defaults(n)
        for b in range(_blocks_to_wrap(chain, frames) + 1):
            if b % 3 == 0:
                p = synth.draw_params(rng, len(slots), dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            if b in (1, 3):
                settings = ref.draw_settings(rng, n, gas.capi)
                ctx.fx_stereo_settings_publish(a, settings)
            src = synth.draw_sources(rng, len(slots), frames)
            mix, peaks = ctx.process_block(src[order], slots[order])
            w0, p0, _ = r.block(p[:n], src[:n], settings)
            _, p1, w1 = rh.block(p[n : n + nf].astype(ob.PARAMS_DTYPE), src[n : n + nf], want64=True)
            _, p2, w2 = rs.block(p[n + nf :].astype(ob.PARAMS_DTYPE), src[n + nf :], want64=True)
            want = w0 + w1[0] + w2[0]
            assert rel_rms(mix[0], want) <= TOL, f"{chain} block {b}: {rel_rms(mix[0], want)}"
            rpeaks = np.concatenate([p0, p1, p2])[order]
            np.testing.assert_allclose(peaks, rpeaks, err_msg=f"block {b}", **PEAK_TOL)


def test_two_enhances_hold_independent_rings_and_delays(gas, ob):
    """[ENHANCE, ENHANCE] with different delays and modes at the two positions: each reads its own settings and ring."""
    K = gas.capi
    n, F = 12, 256
    rng = np.random.default_rng(77)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_stereo(2 * n)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (ENHANCE, ENHANCE))
        ctx.params_publish_batch(slots, _params(n, F))
        s = ref.draw_settings(rng, n, K)
        s["enhance_time_pullout_ms"][:, 0] = rng.uniform(0, 5, n)
        s["enhance_time_pullout_ms"][:, 1] = rng.uniform(20, 50, n)
        s["enhance_surround"][:, 0] = 0.0
        s["enhance_surround"][:, 1] = rng.uniform(0.1, 1, n)
        ctx.fx_stereo_settings_publish(slots, s)
        a, b = ref.EnhanceStage(0, n), ref.EnhanceStage(1, n)
        for blk in range(20):
            x = rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)
            _, peaks = ctx.process_block(x, slots)
            want = b.block(a.block(x, s), s)
            np.testing.assert_array_equal(peaks, np.abs(want).max(axis=1), err_msg=f"block {blk}")


def test_hrtf_peaks_draining_only(gas, ob):
    """[ENHANCE, HRTF] under GAS_FLAG_PEAKS_DRAINING_ONLY: +inf for the playbacks that are not draining, the exact peak
    for the draining ones."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F = 40, 512
    rng = np.random.default_rng(21)
    hrir = _hrir()
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PEAKS_DRAINING_ONLY) as ctx:
        ctx.reserve_fx_stereo(n)
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (ENHANCE, HRTF))
        draining = np.arange(n) % 5 == 2
        for s in slots[draining]:
            ctx.source_set_draining(int(s), True)
        r = ChainRef(ob, (ENHANCE, HRTF), n, F, hrir=hrir)
        settings = ref.draw_settings(rng, n, K)
        ctx.fx_stereo_settings_publish(slots, settings)
        p = synth.draw_params(rng, n, dirs=32, frames=F)
        ctx.params_publish_batch(slots, p)
        for b in range(3):
            src = synth.draw_sources(rng, n, F)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks, _ = r.block(p, src, settings)
            assert rel_rms(mix[0], want) <= TOL
            assert np.isinf(peaks[~draining]).all() and (peaks[~draining] > 0).all()
            np.testing.assert_allclose(peaks[draining], rpeaks[draining], **PEAK_TOL)


def test_invalid_settings_are_refused_with_nothing_taken(gas):
    """Every refused call also carries a valid change (pan 0.75 on the first row, a [PANNER] playback whose mix at
    pan 0 is its input bit for bit, and a valid pullout on the refused row): the blocks that follow the refused calls
    directly, with no publish in between, show that none of it was taken -- first against the defaults a slot starts
    with, then against settings published before a second round of refused calls."""
    K = gas.capi
    F = 128
    chain = (PANNER, ENHANCE, LIMITER)  # position 3 is unused
    rng = np.random.default_rng(1)
    with gas.SpatializerContext(max_sources=3, frames=F) as ctx:
        ctx.reserve_fx_stereo(1)
        slots = np.array([ctx.source_alloc(K.KIND_EFFECT, (PANNER,)), ctx.source_alloc(K.KIND_EFFECT, chain)], np.uint32)
        ctx.params_publish_batch(slots, _params(2, F))
        up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))  # noqa: E731
        down = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))  # noqa: E731
        bad = []
        for field, (lo, hi) in {name: e[:2] for name, e in ref._EDGES.items()}.items():
            bad += [(field, 0, down(lo)), (field, 1, up(hi)), (field, 2, np.nan), (field, 3, np.inf), (field, 3, -np.inf), (field, 3, up(hi))]
        st = [ref.make_stage(k, j, 1) for j, k in enumerate(chain)]

        def refuse_all(start):
            for field, j, value in bad:
                s = start.copy()
                s["panner_pan"][0, 0] = 0.75  # a valid change on the first row: must not be taken either
                s["enhance_pan_pullout"][1, 1] = 3.0  # nor a valid one on the refused row
                s[field][1, j] = value
                with pytest.raises(gas.GasError) as ei:
                    ctx.fx_stereo_settings_publish(slots, s)
                assert ei.value.status == BAD_ARG, (field, j, value)

        def blocks_match(current, what):
            """Three blocks right away: the [PANNER] playback's mix bitwise, the other playback's peaks."""
            for _ in range(3):
                src = rng.uniform(-1, 1, (2, F, 2)).astype(np.float32)
                mix, _ = ctx.process_block(src[:1], slots[:1])
                want = ref.PannerStage(0, 1).block(src[:1], current[:1])
                assert (mix[0] == want[0]).all(), what
                _, peaks = ctx.process_block(src, slots)
                y = src[1:]
                for t in st:
                    y = t.block(y, current[1:])
                np.testing.assert_allclose(peaks[1:], np.abs(y).max(axis=1), err_msg=what, **PEAK_TOL)
                np.testing.assert_array_equal(peaks[:1], np.abs(want).max(axis=1), err_msg=what)

        d = K.fx_stereo_settings_defaults(2)
        refuse_all(d)
        src = rng.uniform(-1, 1, (1, F, 2)).astype(np.float32)
        mix, _ = ctx.process_block(src, slots[:1])
        assert (mix[0] == src[0]).all()  # pan 0, the default, is the identity: the refused calls' 0.75 is not there
        blocks_match(d, "the defaults after refused calls")
        base = ref.draw_settings(rng, 2, K, edges=False)
        base["panner_pan"][0, 0] = -0.5
        ctx.fx_stereo_settings_publish(slots, base)
        blocks_match(base, "published settings")
        refuse_all(base)
        blocks_match(base, "published settings after refused calls")
        edge = K.fx_stereo_settings_defaults(2)
        for field, e in ref._EDGES.items():
            edge[field][0], edge[field][1] = e[0], e[1]
        ctx.fx_stereo_settings_publish(slots, edge)  # both ends of every range pass
        blocks_match(edge, "both ends of every range")
        for bad_chain in ((PANNER, 15), (LIMITER, 10), (ENHANCE, 24)):
            with pytest.raises(gas.GasError):
                ctx.source_alloc(K.KIND_EFFECT, bad_chain)  # 10, 15 and 24 are no effect kinds


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
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (ENHANCE,)) == UNSUPPORTED  # no pool reserved
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (PANNER, ENHANCE)) == UNSUPPORTED
        pl = ctx.source_alloc(K.KIND_EFFECT, (PANNER, LIMITER))  # stateless kinds need no reservation
        pl2 = ctx.source_alloc(K.KIND_EFFECT, (LIMITER, AMP, PANNER, HS))
        ctx.reserve_fx_lines(1, 0)  # the other pools are not this one
        ctx.reserve_fx_eq(1)
        ctx.reserve_fx_mod(1, 0)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY, ENHANCE)) == UNSUPPORTED
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ6, ENHANCE)) == UNSUPPORTED
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS, ENHANCE)) == UNSUPPORTED
        ctx.reserve_fx_stereo(2)  # (reserving does not disturb the stateless playbacks already there)
        a = ctx.source_alloc(K.KIND_EFFECT, (ENHANCE,))
        b = ctx.source_alloc(K.KIND_EFFECT, (PANNER, ENHANCE, LIMITER))
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (ENHANCE,)) == OUT_OF_SLOTS  # rings exhausted
        assert _free_slots(gas, ctx) == 6  # nothing was taken by the refused calls
        assert _status(gas, ctx.reserve_fx_stereo, 4) == BAD_ARG  # rings are held
        assert _status(gas, ctx.reserve_fx_stereo, 0) == BAD_ARG
        ctx.reserve_fx_lines(0, 0)  # ... which does not stop the other pools from being released
        ctx.reserve_fx_eq(0)
        ctx.reserve_fx_mod(0, 0)
        ctx.reserve_fx_lines(1, 0)
        ctx.reserve_fx_eq(1)
        ctx.reserve_fx_mod(1, 0)
        ctx.source_free(a)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (ENHANCE,)) == OUT_OF_SLOTS  # back at the next block only
        assert _status(gas, ctx.reserve_fx_stereo, 4) == BAD_ARG
        z()
        # one ring free; short in exactly one of the other pools, or in the rings: nothing taken anywhere
        d = ctx.source_alloc(K.KIND_EFFECT, (DELAY,))  # the only delay line
        e = ctx.source_alloc(K.KIND_EFFECT, (EQ6,))  # the only EQ bank
        c = ctx.source_alloc(K.KIND_EFFECT, (CHORUS,))  # the only chorus line
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (ENHANCE, DELAY)) == OUT_OF_SLOTS
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (ENHANCE, EQ10)) == OUT_OF_SLOTS
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (CHORUS, ENHANCE)) == OUT_OF_SLOTS
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (ENHANCE, ENHANCE)) == OUT_OF_SLOTS
        for s in (d, e, c):
            ctx.source_free(s)
        z()
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY, ENHANCE, ENHANCE)) == OUT_OF_SLOTS  # one ring only: the line is not taken
        g = ctx.source_alloc(K.KIND_EFFECT, (DELAY, EQ6, CHORUS, ENHANCE))  # so the line, the bank, the chorus line and the ring are still free
        for s in (b, g, pl, pl2):
            ctx.source_free(s)
        z()
        ctx.reserve_fx_stereo(3)  # all free: re-sized
        h3 = ctx.source_alloc(K.KIND_EFFECT, (ENHANCE, ENHANCE, ENHANCE))
        held = ctx.source_alloc(K.KIND_EFFECT, (DELAY,))
        assert _status(gas, ctx.reserve_fx_lines, 0, 0) == BAD_ARG  # a line is held, whatever the rings do
        ctx.source_free(held)
        ctx.source_free(h3)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_fx_stereo(4)
        ctx.reserve_fx_stereo(0)  # released
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (ENHANCE,)) == UNSUPPORTED
        s = ctx.source_alloc(K.KIND_EFFECT, (PANNER, LIMITER))  # the settings table does not go with the pool
        slots = np.array([s], np.uint32)
        ctx.params_publish_batch(slots, _params(1, F))
        st = K.fx_stereo_settings_defaults(1)
        st["panner_pan"][0, 0] = 1.0
        ctx.fx_stereo_settings_publish(slots, st)
        x = np.random.default_rng(3).uniform(-0.2, 0.2, (1, F, 2)).astype(np.float32)
        mix, _ = ctx.process_block(x, slots)
        want = ref.LimiterStage(1, 1).block(ref.PannerStage(0, 1).block(x, st), st)
        assert (mix[0, :, 0] == 0).all() and rel_rms(mix[0], want[0]) <= TOL


def test_reserve_refused_where_the_ring_is_shorter_than_a_block(gas, ob):
    """R = 256 at 4 kHz: below 512 frames (two frames of a block on one ring entry), enough for 256 and 128."""
    assert ref.ring_frames(4000.0) == 256
    with gas.SpatializerContext(max_sources=2, frames=512, mix_rate=4000.0) as ctx:
        assert _status(gas, ctx.reserve_fx_stereo, 1) == BAD_ARG
        assert _status(gas, ctx.reserve_fx_stereo, 0) == 0
        ctx.source_alloc(gas.capi.KIND_EFFECT, (PANNER, LIMITER))
    run_chain(gas, ob, (ENHANCE,), 5, 256, mix_rate=4000.0, seed=9)  # R = frames: every entry rewritten each block


@pytest.mark.parametrize("frames,below,at", [(512, 4920.0, 4930.0), (256, 2450.0, 2470.0), (128, 1220.0, 1240.0)])
def test_the_librarys_ring_size_is_the_restatements(gas, frames, below, at):
    """The reservation is refused exactly where R < frames, so the two mix rates on either side of
    (int)(0.052 sr) = frames / 2 pin the library's ring size (the 0.052 and the bit length) to ref.ring_frames."""
    assert ref.ring_frames(below) == frames // 2 and ref.ring_frames(at) == frames
    with gas.SpatializerContext(max_sources=1, frames=frames, mix_rate=below) as ctx:
        assert _status(gas, ctx.reserve_fx_stereo, 1) == BAD_ARG
    with gas.SpatializerContext(max_sources=1, frames=frames, mix_rate=at) as ctx:
        assert _status(gas, ctx.reserve_fx_stereo, 1) == 0


def _render(gas, chain, srcs, settings, slot_prep=None):
    """A fresh context's output for one playback of `chain` over srcs; slot_prep(ctx, p) may run a different history."""
    from godot_audio_spatializer_amd import synth

    F = srcs[0].shape[1]
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_fx_stereo(4 * sum(k == ENHANCE for k in chain))
        p = synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F)
        slot = ctx.source_alloc(gas.capi.KIND_EFFECT, chain) if slot_prep is None else slot_prep(ctx, p)
        ctx.params_publish(slot, p[0])
        ctx.fx_stereo_settings_publish(np.array([slot], np.uint32), settings)
        return np.stack([ctx.process_block(x, np.array([slot], np.uint32))[0] for x in srcs])


@pytest.mark.parametrize("how", ["recycled", "reset", "reset_many"])
def test_recycled_or_reset_state_is_bitwise_fresh(gas, how):
    """A loud history, then the slot and its rings recycled (free, block, alloc) or gas_source_reset (once, or many
    times before the next block): the next playback equals a fresh context's bit for bit."""
    K = gas.capi
    F = 256
    chain = (ENHANCE, LIMITER, ENHANCE)
    rng = np.random.default_rng(31)
    s = ref.draw_settings(rng, 1, K)
    s["enhance_time_pullout_ms"][:, 0] = 35.0  # the history is read for 6 blocks
    s["enhance_time_pullout_ms"][:, 2] = 50.0
    s["enhance_surround"][:, 2] = 0.8
    srcs = [rng.uniform(-1, 1, (1, F, 2)).astype(np.float32) for _ in range(12)]

    def prep(ctx, p):
        slot = ctx.source_alloc(K.KIND_EFFECT, chain)
        ctx.params_publish(slot, p[0])
        ctx.fx_stereo_settings_publish(np.array([slot], np.uint32), s)
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
    st = [ref.make_stage(k, j, 1) for j, k in enumerate(chain)]
    for b, x in enumerate(srcs):  # and the fresh context is the restatement from rest
        y = x
        for t in st:
            y = t.block(y, s)
        assert rel_rms(fresh[b, 0], y[0]) <= TOL, b


def test_a_recycled_slot_starts_from_the_default_settings(gas):
    K = gas.capi
    F = 128
    with gas.SpatializerContext(max_sources=1, frames=F) as ctx:
        x = np.random.default_rng(8).uniform(-1, 1, (1, F, 2)).astype(np.float32)
        s = K.fx_stereo_settings_defaults(1)
        s["panner_pan"][0, 0] = -1.0
        slot = ctx.source_alloc(K.KIND_EFFECT, (PANNER,))
        slots = np.array([slot], np.uint32)
        ctx.params_publish_batch(slots, _params(1, F))
        ctx.fx_stereo_settings_publish(slots, s)
        mix, _ = ctx.process_block(x, slots)
        assert (mix[0, :, 1] == 0).all()
        ctx.source_free(slot)
        ctx.process_block(np.zeros((0, F, 2), np.float32), np.zeros(0, np.uint32))
        assert ctx.source_alloc(K.KIND_EFFECT, (PANNER,)) == slot
        ctx.params_publish_batch(slots, _params(1, F))
        mix, _ = ctx.process_block(x, slots)
        assert (mix[0] == x[0]).all()


def test_buses_with_stereo_kinds(gas):
    from godot_audio_spatializer_amd import synth

    F, n = 256, 30
    rng = np.random.default_rng(10)
    chain = (ENHANCE, PANNER, LIMITER)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_stereo(n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        p = synth.draw_params(rng, n, dirs=8, frames=F)
        ctx.params_publish_batch(slots, p)
        s = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_stereo_settings_publish(slots, s)
        routes = gas.capi.bus_routes(n)
        routes["dry_bus"] = np.where(np.arange(n) % 3 == 0, 1, 0)
        routes["send_bus"] = np.where(np.arange(n) % 3 == 0, 0, 1)
        routes["send"] = rng.uniform(0, 1, (n, 1, 1)).astype(np.float32) * np.ones((4, 2), np.float32)
        ctx.bus_routes_publish(slots, routes)
        st = [ref.make_stage(k, j, n) for j, k in enumerate(chain)]
        for b in range(4):
            src = synth.draw_sources(rng, n, F)
            out, peaks = ctx.process_block_buses(src, slots, 2)
            y = src
            for t in st:
                y = t.block(y, s)
            y = y.astype(np.float64)
            for bus in range(2):
                w = (routes["dry_bus"] == bus).astype(np.float64) + (routes["send_bus"] == bus) * routes["send"][:, 0, 0].astype(np.float64)
                want = (y * w[:, None, None]).sum(axis=0)
                assert rel_rms(out[bus, 0], want) <= TOL, f"block {b} bus {bus}"
            np.testing.assert_allclose(peaks, np.abs(y).max(axis=1), **PEAK_TOL)


def test_process_frames_1_matches_the_batched_row_bitwise(gas):
    from godot_audio_spatializer_amd import synth

    F = 256
    rng = np.random.default_rng(11)
    chain = (PANNER, ENHANCE, LIMITER)
    s = ref.draw_settings(rng, 1, gas.capi)
    s["enhance_time_pullout_ms"][:, 1] = 12.0
    srcs = [synth.draw_sources(rng, 1, F) * np.float32(3.0) for _ in range(6)]
    outs = []
    for single in (False, True):
        with gas.SpatializerContext(max_sources=2, frames=F) as ctx:
            ctx.reserve_fx_stereo(2)
            slots = ctx.source_alloc_many(1, gas.capi.KIND_EFFECT, chain)
            ctx.params_publish_batch(slots, synth.draw_params(np.random.default_rng(0), 1, dirs=8, frames=F))
            ctx.fx_stereo_settings_publish(slots, s)
            got = [ctx.process_frames_1(int(slots[0]), x[0]) if single else ctx.process_block(x, slots)[0][0] for x in srcs]
            outs.append(np.stack(got))
    np.testing.assert_array_equal(outs[0], outs[1])


def test_host_layer_queues_stereo_settings(gas):
    """BatchedSpatializerHost + gas_host_set_effect_settings_stereo: one playback through [ENHANCE, PANNER, LIMITER]
    equals the reference applied to what the same host delivers for an empty chain."""
    K = gas.capi
    F = 256
    rng = np.random.default_rng(12)
    stream = rng.uniform(-0.8, 0.8, (F * 20, 2)).astype(np.float32)
    from godot_audio_spatializer_amd import synth

    chain = (ENHANCE, PANNER, LIMITER)
    params = synth.draw_params(rng, 1, dirs=8, frames=F)
    new = ref.draw_settings(rng, 1, K)
    new["enhance_time_pullout_ms"][:, 0] = 9.0
    new["panner_pan"][:, 1] = 0.4
    got = {}
    for ch in (chain, ()):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_fx_stereo(2)
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, ch)
            pid = host.start_playback_array(stream)
            host.set_spatializer_parameters(pid, params[0])
            outs = []
            for cb in range(8):
                if cb == 3 and ch:
                    assert host.set_effect_settings_stereo(pid, new) == 0
                    bad = new.copy()
                    bad["limiter_ceiling_db"][0, 3] = 0.0
                    assert host.set_effect_settings_stereo(pid, bad) == BAD_ARG  # refused when queued
                rc, out = host.get_mixed_frames(0, F)
                assert rc == 0
                outs.append(out.copy())
            host.close()
        got[ch] = np.stack(outs)
    window = got[()]
    st = [ref.make_stage(k, j, 1) for j, k in enumerate(chain)]
    d = K.fx_stereo_settings_defaults(1)
    for cb in range(8):
        s = new if cb >= 3 else d
        y = window[cb][None]
        for t in st:
            y = t.block(y, s)
        assert rel_rms(got[chain][cb], y[0]) <= TOL, f"callback {cb}"


def test_two_runs_are_bitwise_equal(gas, ob):
    a, _, _ = run_chain(gas, ob, (PANNER, ENHANCE, LIMITER), 70, 512, blocks=10, seed=5, check=False, scale=3.0)
    b, _, _ = run_chain(gas, ob, (PANNER, ENHANCE, LIMITER), 70, 512, blocks=10, seed=5, check=False, scale=3.0)
    np.testing.assert_array_equal(a, b)
