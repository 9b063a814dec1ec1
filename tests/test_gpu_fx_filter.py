"""GAS_FX_FILTER on the GPU (k_fx_filter.hip) against the numpy restatement tests/fx_filter_ref.py, against the existing
one-stage kinds 1 and 4 .. 8 (which are in turn checked against the oracle), composed with the oracle's kinds
(oracle.binding.BatchOracle) and tests/fx_eq_ref.py for mixed chains; and the bank pool's lifecycle
(gas_ctx_reserve_fx_filter).

The kernel runs every stage in the engine's order with separate f32 operations, as the restatement does, so a source's
rows -- and with them its peak -- are the restatement's bits; the mix is compared within TOL because the library sums
the sources in f32 in its own order and the reference in f64."""
import numpy as np
import pytest

import fx_eq_ref
import fx_filter_ref as ref
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HS, ER, HRTF, LP, HP, BP, NOTCH, LS, AMP = 1, 2, 3, 4, 5, 6, 7, 8, 9
DELAY, EQ6, CHORUS, ENHANCE = 13, 16, 19, 22
FILTER = 24
BAD_ARG, OUT_OF_SLOTS, UNSUPPORTED = -1, -2, -6
# which one-stage kind is which type of the new kind
KIND_OF_TYPE = {ref.LOWPASS: LP, ref.HIGHPASS: HP, ref.BANDPASS: BP, ref.NOTCH: NOTCH, ref.LOWSHELF: LS, ref.HIGHSHELF: HS}


def _hrir(dirs=32, seed=5):
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(seed), dirs=dirs)


def _capi():
    from godot_audio_spatializer_amd import capi

    return capi


def _params(n, frames):
    from godot_audio_spatializer_amd import synth

    return synth.draw_params(np.random.default_rng(0), n, dirs=8, frames=frames)


def _one(n, ftype, db, cutoff=2000.0, resonance=0.5, gain=1.0, pos=0):
    s = _capi().fx_filter_settings_defaults(n)
    s["type"][:, pos], s["db"][:, pos], s["cutoff_hz"][:, pos], s["resonance"][:, pos], s["gain"][:, pos] = ftype, db, cutoff, resonance, gain
    return s


class ChainRef:
    """A playback chain's reference: runs of the oracle's kinds through BatchOracle (one source per oracle where a new
    kind follows, for its rows; all sources in one oracle for a last run), GAS_FX_FILTER through fx_filter_ref, EQ6
    through fx_eq_ref at 0 dB."""

    def __init__(self, ob, chain, n, frames, hrir=None, ring=0, mix_rate=48000.0):
        self.stages = []
        segs = []
        for j, k in enumerate(chain):
            own = k in (FILTER, EQ6)
            if segs and not own and not segs[-1][0]:
                segs[-1][1].append(j)
            else:
                segs.append((own, [j]))
        for si, (own, pos) in enumerate(segs):
            k0 = chain[pos[0]]
            if k0 == FILTER:
                self.stages.append(("flt", ref.FilterStage(pos[0], n, mix_rate)))
            elif k0 == EQ6:
                self.stages.append(("eq", fx_eq_ref.EqStage(k0, pos[0], n, mix_rate)))
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
            if kind == "flt":
                x = obj.block(x, settings)
            elif kind == "eq":
                x = obj.block(x, _capi().fx_eq_settings_defaults(len(x)))
            elif kind == "rows":
                x = np.stack([o.block(p[s : s + 1], x[s : s + 1])[0][0] for s, o in enumerate(obj)])
            else:
                _, peaks, r64 = obj.block(p, x, want64=True)
                return r64[0], peaks, None
        return x.astype(np.float64).sum(axis=0), np.abs(x).max(axis=1), x


def _banks(chain, n):
    return n * sum(k == FILTER for k in chain)


def _ctx(gas, chain, n, frames, mix_rate=48000.0, extra=0, flags=0):
    ring = 4096 if ER in chain else 0
    ctx = gas.SpatializerContext(max_sources=n + extra, frames=frames, er_ring_frames=ring, mix_rate=mix_rate, flags=flags)
    ctx.reserve_fx_filter(max(1, _banks(chain, n)))
    if EQ6 in chain:
        ctx.reserve_fx_eq(n)
    return ctx, ring


def run_chain(gas, ob, chain, n, frames, blocks=4, seed=0, mix_rate=48000.0, check=True, draw=None):
    """Settings drawn over the whole range and re-published every block.  Returns the last mix."""
    from godot_audio_spatializer_amd import synth

    rng = np.random.default_rng(seed)
    draw = draw or (lambda m: ref.draw_settings(rng, m, gas.capi))
    hrir = _hrir() if HRTF in chain else None
    ctx, ring = _ctx(gas, chain, n, frames, mix_rate)
    with ctx:
        if hrir is not None:
            ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring, mix_rate=mix_rate)
        for b in range(blocks):
            if b % 3 == 0:
                p = synth.draw_params(rng, n, dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            settings = draw(n)
            ctx.fx_filter_settings_publish(slots, settings)
            src = synth.draw_sources(rng, n, frames)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks, rows = r.block(p, src, settings)
            if check:
                print(f"{chain} n={n} F={frames} block {b}: mix {rel_rms(mix[0], want):.3e}")
                assert rel_rms(mix[0], want) <= TOL, f"{chain} n={n} F={frames} block {b}: {rel_rms(mix[0], want)}"
                np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=f"block {b}")
                if rows is not None:
                    np.testing.assert_array_equal(peaks, rpeaks, err_msg=f"block {b}: rows are not the restatement's bits")
    return mix


# ------------------------------------------------------------------------------------------ rows against the restatement
@pytest.mark.parametrize("frames,mix_rate", [(128, 44100.0), (256, 48000.0), (384, 96000.0), (512, 48000.0), (512, 44100.0), (128, 96000.0)])
@pytest.mark.parametrize("ftype", ref.TYPES)
def test_rows_are_the_restatements_bits(gas, ftype, frames, mix_rate):
    """24 sources of one type, six of them at each slope, random cutoff / resonance / gain, re-published every block.
    Even blocks run batched (peaks bitwise, mix within TOL); odd blocks run one source per call, whose mix is that
    source's row: compared sample by sample."""
    n = 24
    rng = np.random.default_rng(ftype * 100 + frames)
    with gas.SpatializerContext(max_sources=n, frames=frames, mix_rate=mix_rate) as ctx:
        ctx.reserve_fx_filter(n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (FILTER,))
        ctx.params_publish_batch(slots, _params(n, frames))
        st = ref.FilterStage(0, n, mix_rate)
        for b in range(4):
            s = ref.draw_settings(rng, n, gas.capi, types=(ftype,))
            s["db"][:, 0] = np.arange(n) % 4
            ctx.fx_filter_settings_publish(slots, s)
            src = rng.uniform(-1, 1, (n, frames, 2)).astype(np.float32)
            y = st.block(src, s)
            if b % 2 == 0:
                mix, peaks = ctx.process_block(src, slots)
                np.testing.assert_array_equal(peaks, np.abs(y).max(axis=1), err_msg=f"block {b}")
                assert rel_rms(mix[0], y.astype(np.float64).sum(axis=0)) <= TOL, f"block {b}"
            else:
                for i in range(n):
                    row = ctx.process_block(src[i : i + 1], slots[i : i + 1])[0][0]
                    np.testing.assert_array_equal(row, y[i], err_msg=f"block {b} source {i} db {i % 4}")


# ------------------------------------------------------------------------------------------- pinned to the existing kinds
def _peaks_and_rows(gas, chain, n, frames, srcs, publish):
    """Peaks of every block and the rows of the last one (one source per call) for n playbacks of `chain`."""
    with gas.SpatializerContext(max_sources=n, frames=frames) as ctx:
        ctx.reserve_fx_filter(n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        publish(ctx, slots)
        peaks = [ctx.process_block(x, slots)[1] for x in srcs[:-1]]
        rows = np.stack([ctx.process_block(srcs[-1][i : i + 1], slots[i : i + 1])[0][0] for i in range(n)])
    return np.stack(peaks), rows


def test_24db_lowpass_equals_four_lowpass_stages_bitwise(gas, monkeypatch):
    """[FILTER(LOWPASS, 24 dB, resonance <= 1)] against [LP, LP, LP, LP] of the same cutoff and resonance, both in
    engine order (GAS_SHELF_SCAN=0): rows and peaks bit for bit."""
    monkeypatch.setenv("GAS_SHELF_SCAN", "0")
    n, F = 24, 256
    rng = np.random.default_rng(41)
    cutoff = np.exp(rng.uniform(np.log(20.0), np.log(20000.0), n)).astype(np.float32)
    res = rng.uniform(0.0, 1.0, n).astype(np.float32)
    srcs = [rng.uniform(-1, 1, (n, F, 2)).astype(np.float32) for _ in range(4)]

    def new(ctx, slots):
        ctx.params_publish_batch(slots, _params(n, F))
        ctx.fx_filter_settings_publish(slots, _one(n, ref.LOWPASS, 3, cutoff, res))

    def old(ctx, slots):
        ctx.params_publish_batch(slots, _params(n, F))
        s = ctx.fx_settings_defaults(n)
        s["filter_cutoff_hz"][:] = cutoff[:, None]
        s["filter_resonance"][:] = res[:, None]
        ctx.fx_settings_publish(slots, s)

    p_new, r_new = _peaks_and_rows(gas, (FILTER,), n, F, srcs, new)
    p_old, r_old = _peaks_and_rows(gas, (LP, LP, LP, LP), n, F, srcs, old)
    np.testing.assert_array_equal(p_new, p_old)
    np.testing.assert_array_equal(r_new, r_old)


@pytest.mark.parametrize("ftype", sorted(KIND_OF_TYPE))
def test_6db_equals_the_one_stage_kind_bitwise(gas, monkeypatch, ftype):
    """[FILTER(type, 6 dB)] against [kind] for kinds 1 and 4 .. 8 (engine order): rows and peaks bit for bit.  Kind 1
    takes cutoff and gain from gas_params and runs at resonance 1."""
    monkeypatch.setenv("GAS_SHELF_SCAN", "0")
    n, F = 24, 256
    kind = KIND_OF_TYPE[ftype]
    rng = np.random.default_rng(50 + ftype)
    cutoff = np.exp(rng.uniform(np.log(20.0), np.log(20000.0), n)).astype(np.float32)
    res = np.ones(n, np.float32) if kind == HS else rng.uniform(0.0, 1.0, n).astype(np.float32)
    gain = rng.uniform(0.0, 4.0, n).astype(np.float32)
    srcs = [rng.uniform(-1, 1, (n, F, 2)).astype(np.float32) for _ in range(4)]
    p = _params(n, F)
    p["fx_shelf_cutoff_hz"] = cutoff
    p["fx_shelf_gain"] = gain

    def new(ctx, slots):
        ctx.params_publish_batch(slots, p)
        ctx.fx_filter_settings_publish(slots, _one(n, ftype, 0, cutoff, res, gain))

    def old(ctx, slots):
        ctx.params_publish_batch(slots, p)
        s = ctx.fx_settings_defaults(n)
        s["filter_cutoff_hz"][:] = cutoff[:, None]
        s["filter_resonance"][:] = res[:, None]
        s["filter_gain"][:] = gain[:, None]
        ctx.fx_settings_publish(slots, s)

    p_new, r_new = _peaks_and_rows(gas, (FILTER,), n, F, srcs, new)
    p_old, r_old = _peaks_and_rows(gas, (kind,), n, F, srcs, old)
    np.testing.assert_array_equal(p_new, p_old)
    np.testing.assert_array_equal(r_new, r_old)


# ----------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n,frames", [(1, 128), (31, 256), (33, 384), (256, 512), (1, 512), (1000, 256)])
def test_alone(gas, ob, n, frames):
    run_chain(gas, ob, (FILTER,), n, frames, seed=n + frames)


def test_alone_8192(gas, ob):
    run_chain(gas, ob, (FILTER,), 8192, 512, blocks=3, seed=8)


def test_db_and_type_change_between_blocks(gas):
    """24 dB -> 6 dB -> 24 dB and a type change per block: stages that sit out keep their history (the restatement's
    rows, bitwise, only if the bank's upper stages were left alone)."""
    n, F = 16, 256
    rng = np.random.default_rng(61)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_filter(n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (FILTER,))
        ctx.params_publish_batch(slots, _params(n, F))
        st = ref.FilterStage(0, n)
        for b, (db, ftype) in enumerate([(3, ref.HIGHPASS), (0, ref.HIGHPASS), (3, ref.HIGHPASS), (1, ref.LOWSHELF), (2, ref.BANDLIMIT), (3, ref.NOTCH)]):
            s = ref.draw_settings(rng, n, gas.capi, types=(ftype,), dbs=(db,))
            ctx.fx_filter_settings_publish(slots, s)
            src = rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)
            _, peaks = ctx.process_block(src, slots)
            np.testing.assert_array_equal(peaks, np.abs(st.block(src, s)).max(axis=1), err_msg=f"block {b}")


def test_two_instances_in_one_chain_with_different_slopes(gas, ob):
    rng = np.random.default_rng(62)

    def draw(m):
        s = ref.draw_settings(rng, m, _capi())
        s["db"][:, 0], s["db"][:, 1] = 3, 1
        return s

    run_chain(gas, ob, (FILTER, FILTER), 40, 256, seed=62, draw=draw)
    run_chain(gas, ob, (FILTER, FILTER, FILTER, FILTER), 9, 128, seed=63)  # GAS_MAX_EFFECTS of them


def test_512_frames_equal_two_contexts_of_256(gas):
    n = 20
    rng = np.random.default_rng(64)
    s = ref.draw_settings(rng, n, gas.capi)
    srcs = [rng.uniform(-1, 1, (n, 512, 2)).astype(np.float32) for _ in range(3)]
    outs = []
    for F in (512, 256):
        with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
            ctx.reserve_fx_filter(n)
            slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (FILTER,))
            ctx.params_publish_batch(slots, _params(n, F))
            ctx.fx_filter_settings_publish(slots, s)
            got = []
            for x in srcs:
                got.append(np.concatenate([ctx.process_block(x[:, k : k + F], slots)[0][0] for k in range(0, 512, F)]))
            outs.append(np.stack(got))
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize(
    "chain,frames",
    [
        ((FILTER, HRTF), 512),
        ((FILTER, ER, HRTF), 256),
        ((EQ6, FILTER), 256),
        ((LP, FILTER, AMP), 128),
        ((HS, FILTER), 512),
    ],
)
def test_mixed_chains_next_to_fused_chains(gas, ob, chain, frames):
    """The chain's playbacks share callbacks with fused [HRTF] and [HIGHSHELF] playbacks; mix and peaks of all."""
    from godot_audio_spatializer_amd import synth

    n, nf = 24, 10
    rng = np.random.default_rng(len(chain) * 17 + frames)
    hrir = _hrir()
    ctx, ring = _ctx(gas, chain, n, frames, extra=2 * nf)
    with ctx:
        ctx.hrtf_load(hrir)
        a = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        h = ctx.source_alloc_many(nf, gas.capi.KIND_EFFECT, (HRTF,))
        s_ = ctx.source_alloc_many(nf, gas.capi.KIND_EFFECT, (HS,))
        slots = np.concatenate([a, h, s_])
        order = rng.permutation(len(slots))
        r = ChainRef(ob, chain, n, frames, hrir=hrir, ring=ring)
        rh = ob.BatchOracle(ob.KIND_EFFECT, nf, frames, chain=(HRTF,), hrir=hrir, er_ring_frames=1)
        rs = ob.BatchOracle(ob.KIND_EFFECT, nf, frames, chain=(HS,), hrir=None, er_ring_frames=1)
        for b in range(5):
            if b % 3 == 0:
                p = synth.draw_params(rng, len(slots), dirs=32, ring_frames=max(ring, 2 * frames), frames=frames)
                ctx.params_publish_batch(slots, p)
            # behind another stage whose rows differ from the oracle's in the last bit the filters stay moderate: a
            # resonant or high-gain cascade scales that difference (fx_eq's test does the same behind the reflections)
            settings = ref.draw_settings(rng, n, gas.capi, lo_hz=200.0, hi_hz=8000.0)
            settings["resonance"] = np.maximum(settings["resonance"], 0.3)
            settings["gain"] = np.clip(settings["gain"], 0.5, 2.0)
            ctx.fx_filter_settings_publish(a, settings)
            src = synth.draw_sources(rng, len(slots), frames)
            mix, peaks = ctx.process_block(src[order], slots[order])
            w0, p0, _ = r.block(p[:n], src[:n], settings)
            _, p1, w1 = rh.block(p[n : n + nf].astype(ob.PARAMS_DTYPE), src[n : n + nf], want64=True)
            _, p2, w2 = rs.block(p[n + nf :].astype(ob.PARAMS_DTYPE), src[n + nf :], want64=True)
            want = w0 + w1[0] + w2[0]
            print(f"{chain} block {b}: mix {rel_rms(mix[0], want):.3e}")
            assert rel_rms(mix[0], want) <= TOL, f"{chain} block {b}: {rel_rms(mix[0], want)}"
            rpeaks = np.concatenate([p0, p1, p2])[order]
            np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=f"block {b}")


def test_filter_hrtf_peaks_draining_only(gas, ob):
    """[FILTER, HRTF] under GAS_FLAG_PEAKS_DRAINING_ONLY: +inf for the playbacks that are not draining, the exact peak
    for the draining ones."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F = 40, 512
    rng = np.random.default_rng(65)
    hrir = _hrir()
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PEAKS_DRAINING_ONLY) as ctx:
        ctx.reserve_fx_filter(n)
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (FILTER, HRTF))
        draining = np.arange(n) % 5 == 2
        for s in slots[draining]:
            ctx.source_set_draining(int(s), True)
        r = ChainRef(ob, (FILTER, HRTF), n, F, hrir=hrir)
        settings = _one(n, ref.LOWPASS, 3, 1200.0, 0.7)
        ctx.fx_filter_settings_publish(slots, settings)
        p = synth.draw_params(rng, n, dirs=32, frames=F)
        ctx.params_publish_batch(slots, p)
        for b in range(3):
            src = synth.draw_sources(rng, n, F)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks, _ = r.block(p, src, settings)
            assert rel_rms(mix[0], want) <= TOL
            assert np.isinf(peaks[~draining]).all() and (peaks[~draining] > 0).all()
            np.testing.assert_allclose(peaks[draining], rpeaks[draining], rtol=2e-5, atol=1e-7)


# -------------------------------------------------------------------------------------------------------------- settings
def test_invalid_settings_are_refused_with_nothing_taken(gas):
    K = gas.capi
    F = 128
    with gas.SpatializerContext(max_sources=3, frames=F) as ctx:
        ctx.reserve_fx_filter(2)
        slots = ctx.source_alloc_many(2, K.KIND_EFFECT, (FILTER,))
        ctx.params_publish_batch(slots, _params(2, F))
        bad = [("type", -1), ("type", 7), ("db", -1), ("db", 4), ("cutoff_hz", 0.5), ("cutoff_hz", 20501.0), ("cutoff_hz", np.nan), ("resonance", -0.1), ("resonance", 1.1), ("resonance", np.inf), ("gain", -0.1), ("gain", 4.1), ("gain", np.nan)]
        for field, value in bad:
            for j in (0, 3):  # a used and an unused position
                s = K.fx_filter_settings_defaults(2)
                s["cutoff_hz"][0, 0] = 300.0  # a valid change on the first row: must not be taken either
                s[field][1, j] = value
                with pytest.raises(gas.GasError) as ei:
                    ctx.fx_filter_settings_publish(slots, s)
                assert ei.value.status == BAD_ARG, (field, value, j)
        for res in (0.0, -0.0):  # the band limit at resonance <= 0: refused (the engine's coefficients are NaN there)
            s = _one(2, ref.BANDLIMIT, 0, 2000.0, res, pos=2)
            with pytest.raises(gas.GasError) as ei:
                ctx.fx_filter_settings_publish(slots, s)
            assert ei.value.status == BAD_ARG
        ctx.fx_filter_settings_publish(slots, _one(2, ref.BANDLIMIT, 3, 20500.0, 1.0, 4.0))  # the ranges' ends are legal
        ctx.fx_filter_settings_publish(slots, _one(2, ref.LOWPASS, 0, 1.0, 0.0, 0.0))
        ctx.fx_filter_settings_publish(slots, K.fx_filter_settings_defaults(2))
        st = ref.FilterStage(0, 2)
        d = K.fx_filter_settings_defaults(2)
        rng = np.random.default_rng(1)
        for _ in range(3):
            src = rng.uniform(-1, 1, (2, F, 2)).astype(np.float32)
            _, peaks = ctx.process_block(src, slots)
            np.testing.assert_array_equal(peaks, np.abs(st.block(src, d)).max(axis=1))
        with pytest.raises(gas.GasError):
            ctx.source_alloc(K.KIND_EFFECT, (FILTER, 25))  # 25 is no effect kind
        for k in (10, 15):
            with pytest.raises(gas.GasError):
                ctx.source_alloc(K.KIND_EFFECT, (k,))  # still unassigned


def test_a_new_slot_starts_at_the_resource_defaults(gas):
    F, n = 128, 5
    rng = np.random.default_rng(66)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_filter(n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (FILTER,))
        ctx.params_publish_batch(slots, _params(n, F))
        st = ref.FilterStage(0, n)
        src = rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)
        _, peaks = ctx.process_block(src, slots)
        np.testing.assert_array_equal(peaks, np.abs(st.block(src, gas.capi.fx_filter_settings_defaults(n))).max(axis=1))


# ------------------------------------------------------------------------------------------------------------------ pool
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


def test_pool_errors_and_lifecycle_with_every_other_pool(gas):
    K = gas.capi
    F = 128
    with gas.SpatializerContext(max_sources=8, frames=F) as ctx:
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (FILTER,)) == UNSUPPORTED  # no pool reserved
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (HS, FILTER)) == UNSUPPORTED
        ctx.reserve_fx_lines(1, 0)  # the other pools are not this pool
        ctx.reserve_fx_eq(1)
        ctx.reserve_fx_mod(1, 0)
        ctx.reserve_fx_stereo(1)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (DELAY, FILTER)) == UNSUPPORTED
        ctx.reserve_fx_filter(3)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (FILTER, EQ6, EQ6)) == OUT_OF_SLOTS  # one EQ bank only
        a = ctx.source_alloc(K.KIND_EFFECT, (FILTER,))
        b = ctx.source_alloc(K.KIND_EFFECT, (FILTER, FILTER))
        ctx.params_publish(b, _params(1, F)[0])
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (FILTER,)) == OUT_OF_SLOTS  # banks exhausted
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (EQ6, FILTER)) == OUT_OF_SLOTS  # an EQ bank, but no filter bank
        assert _free_slots(gas, ctx) == 6  # nothing was taken by the refused calls
        e = ctx.source_alloc(K.KIND_EFFECT, (EQ6,))  # so the EQ bank is still free
        assert _status(gas, ctx.reserve_fx_filter, 8) == BAD_ARG  # banks are held
        assert _status(gas, ctx.reserve_fx_filter, 0) == BAD_ARG
        ctx.reserve_fx_lines(0, 0)  # ... which does not stop another pool from being released
        ctx.reserve_fx_lines(1, 0)
        ctx.source_free(a)
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (FILTER,)) == OUT_OF_SLOTS  # back at the next block only
        assert _status(gas, ctx.reserve_fx_filter, 8) == BAD_ARG
        ctx.process_block(np.zeros((1, F, 2), np.float32), np.array([b], np.uint32))
        for chain in ((FILTER, DELAY, DELAY), (FILTER, CHORUS, CHORUS), (FILTER, ENHANCE, ENHANCE)):
            assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, chain) == OUT_OF_SLOTS  # a bank, but one line / ring only
        c = ctx.source_alloc(K.KIND_EFFECT, (FILTER, DELAY, CHORUS, ENHANCE))  # so the bank is still free; one of each pool
        for s in (b, c, e):
            ctx.source_free(s)
        ctx.process_block(np.zeros((0, F, 2), np.float32), np.zeros(0, np.uint32))
        ctx.reserve_fx_filter(2)  # all free: re-sized
        ctx.source_alloc(K.KIND_EFFECT, (FILTER, FILTER))
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (FILTER,)) == OUT_OF_SLOTS
        ctx.reserve_fx_eq(0)  # a held filter bank does not hold the other pools
        ctx.reserve_fx_mod(0, 0)
        ctx.reserve_fx_stereo(0)
        ctx.reserve_fx_lines(0, 0)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_fx_filter(4)
        ctx.reserve_fx_filter(0)  # released
        assert _status(gas, ctx.source_alloc, K.KIND_EFFECT, (FILTER,)) == UNSUPPORTED
        ctx.fx_filter_settings_publish(np.zeros(0, np.uint32), K.fx_filter_settings_defaults(0))  # nothing to reach: fine


def _render(gas, chain, srcs, settings, slot_prep=None):
    """A fresh context's output for one playback of `chain` over srcs; slot_prep(ctx, p) may run a different history."""
    F = srcs[0].shape[1]
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_fx_filter(4 * _banks(chain, 1))
        p = _params(1, F)
        slot = ctx.source_alloc(gas.capi.KIND_EFFECT, chain) if slot_prep is None else slot_prep(ctx, p)
        ctx.params_publish(slot, p[0])
        ctx.fx_filter_settings_publish(np.array([slot], np.uint32), settings)
        return np.stack([ctx.process_block(x, np.array([slot], np.uint32))[0] for x in srcs])


@pytest.mark.parametrize("how", ["recycled", "reset", "reset_many"])
def test_recycled_or_reset_bank_is_bitwise_fresh(gas, how):
    """A loud history, then the slot and its banks recycled (free, block, alloc) or gas_source_reset (once, or many
    times before the next block): the next playback equals a fresh context's bit for bit."""
    K = gas.capi
    F = 256
    chain = (FILTER, FILTER)
    rng = np.random.default_rng(71)
    s = _one(1, ref.LOWPASS, 3, 300.0, 1.0)
    s["type"][:, 1], s["db"][:, 1], s["cutoff_hz"][:, 1], s["gain"][:, 1] = ref.LOWSHELF, 2, 500.0, 3.0
    srcs = [rng.uniform(-1, 1, (1, F, 2)).astype(np.float32) for _ in range(4)]

    def prep(ctx, p):
        slot = ctx.source_alloc(K.KIND_EFFECT, chain)
        ctx.params_publish(slot, p[0])
        ctx.fx_filter_settings_publish(np.array([slot], np.uint32), s)
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
    rng = np.random.default_rng(72)
    s = ref.draw_settings(rng, n, K)
    srcs = [rng.uniform(-1, 1, (n, F, 2)).astype(np.float32) for _ in range(3)]
    outs = []
    for history in (False, True):
        with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
            ctx.reserve_fx_filter(2 * n)
            slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (FILTER, FILTER))
            ctx.params_publish_batch(slots, _params(n, F))
            ctx.fx_filter_settings_publish(slots, s)
            if history:
                for _ in range(4):
                    ctx.process_block(rng.uniform(-1, 1, (n, F, 2)).astype(np.float32), slots)
                for sl in slots:
                    ctx.source_reset(int(sl))
            outs.append(np.stack([ctx.process_block(x, slots)[1] for x in srcs]))
    np.testing.assert_array_equal(outs[1], outs[0])


# ------------------------------------------------------------------------------------------------- the other entry points
def test_buses_with_the_filter_kind(gas):
    from godot_audio_spatializer_amd import synth

    F, n = 256, 30
    rng = np.random.default_rng(73)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_filter(n)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (FILTER,))
        ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=8, frames=F))
        s = ref.draw_settings(rng, n, gas.capi)
        ctx.fx_filter_settings_publish(slots, s)
        routes = gas.capi.bus_routes(n)
        routes["dry_bus"] = np.where(np.arange(n) % 3 == 0, 1, 0)
        routes["send_bus"] = np.where(np.arange(n) % 3 == 0, 0, 1)
        routes["send"] = rng.uniform(0, 1, (n, 1, 1)).astype(np.float32) * np.ones((4, 2), np.float32)
        ctx.bus_routes_publish(slots, routes)
        st = ref.FilterStage(0, n)
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
    rng = np.random.default_rng(74)
    chain = (FILTER, FILTER)
    s = ref.draw_settings(rng, 1, gas.capi)
    srcs = [synth.draw_sources(rng, 1, F) for _ in range(4)]
    outs = []
    for single in (False, True):
        with gas.SpatializerContext(max_sources=2, frames=F) as ctx:
            ctx.reserve_fx_filter(2)
            slots = ctx.source_alloc_many(1, gas.capi.KIND_EFFECT, chain)
            ctx.params_publish_batch(slots, _params(1, F))
            ctx.fx_filter_settings_publish(slots, s)
            got = [ctx.process_frames_1(int(slots[0]), x[0]) if single else ctx.process_block(x, slots)[0][0] for x in srcs]
            outs.append(np.stack(got))
    np.testing.assert_array_equal(outs[0], outs[1])


def test_host_layer_queues_filter_settings(gas):
    """BatchedSpatializerHost + gas_host_set_effect_settings_filter: one playback through [FILTER] equals the reference
    applied to what the same host delivers for an empty chain."""
    K = gas.capi
    F = 256
    rng = np.random.default_rng(75)
    stream = rng.uniform(-0.8, 0.8, (F * 20, 2)).astype(np.float32)
    params = _params(1, F)
    new = _one(1, ref.LOWPASS, 3, 900.0, 0.8)
    got = {}
    for chain in ((FILTER,), ()):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_fx_filter(2)
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, chain)
            pid = host.start_playback_array(stream)
            host.set_spatializer_parameters(pid, params[0])
            outs = []
            for cb in range(8):
                if cb == 3 and chain:
                    assert host.set_effect_settings_filter(pid, new) == 0
                    bad = new.copy()
                    bad["db"][0, 3] = 4
                    assert host.set_effect_settings_filter(pid, bad) == BAD_ARG  # refused when queued
                    bad = _one(1, ref.BANDLIMIT, 0, 2000.0, 0.0)
                    assert host.set_effect_settings_filter(pid, bad) == BAD_ARG
                rc, out = host.get_mixed_frames(0, F)
                assert rc == 0
                outs.append(out.copy())
            host.close()
        got[chain] = np.stack(outs)
    window = got[()]
    st = ref.FilterStage(0, 1)
    d = K.fx_filter_settings_defaults(1)
    for cb in range(8):
        y = st.block(window[cb][None], new if cb >= 3 else d)[0]
        assert rel_rms(got[(FILTER,)][cb], y) <= TOL, f"callback {cb}"


def test_two_runs_are_bitwise_equal(gas, ob):
    a = run_chain(gas, ob, (FILTER, FILTER), 70, 256, blocks=3, seed=5, check=False)
    b = run_chain(gas, ob, (FILTER, FILTER), 70, 256, blocks=3, seed=5, check=False)
    np.testing.assert_array_equal(a, b)
