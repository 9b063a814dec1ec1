"""GAS_FLAG_ER_TAP_FADE on the GPU: k_er_only<FADE> in every place an early-reflection stage runs on a flagged context,
against tests/er_fade_ref.py (two er_ref closed forms in lockstep, lerped in float64).

Inputs, tap tables, the render loop and the comparison are test_gpu_er_edges.py's: taps from er_ref.TapDrawer's edge
table, redrawn every third callback -- so changed and unchanged blocks alternate -- over er_ref.callbacks(F, R) callbacks;
the mix at rel_rms <= TOL against float64 and the peaks at rtol 2e-5, atol 1e-7.  Every case asserts that the reference
both faded and passed through, so neither road goes unseen."""
import numpy as np
import pytest

import er_fade_ref
import er_ref
import er_rooms_ref
import hrtf_blend_fade_ref
import test_gpu_er_edges as E
import test_gpu_er_rooms as RM
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HS, ER, HRTF, AMPLIFY = E.HS, E.ER, E.HRTF, E.AMPLIFY
SHAPES = [(128, 256), (512, 1024)]
_ids = E._ids


def fade_blocks(F, R, params, srcs, through_hrtf=False, active_of=None, amplify=False):
    """[(mix64, peaks)] from er_fade_ref alone, and the bank (for its fade counts).  through_hrtf: as
    test_gpu_er_edges.closed_form_blocks -- a unit-impulse HRIR and hrtf_gain = 1, both ears (yl + yr) / 2 times the HRTF
    stage's gain ramp over the first callback.  amplify: the rows times AMP_DB behind the stage."""
    n = len(params[0])
    bank = er_fade_ref.ErFadeBank(n, F, R)
    out = []
    for b, (p, x) in enumerate(zip(params, srcs)):
        act = np.arange(n) if active_of is None else np.asarray(active_of(b))
        rows = bank.block(p[act], x[act], active=act)
        if through_hrtf:
            mono = rows.mean(axis=2)
            if b == 0:
                mono = mono * (np.arange(F, dtype=np.float64) / F)[None, :]
            rows = np.stack([mono, mono], axis=2)
        if amplify:
            rows = rows * float(np.float32(10.0 ** (E.AMP_DB / 20.0)))
        out.append((rows.sum(axis=0), np.abs(rows).max(axis=1)))
    return out, bank


def both_roads(bank, blocks, sources=None):
    """Every (listed) source faded in some callbacks and passed through in others."""
    for s, k in enumerate(bank.faded()):
        if sources is None or s in sources:
            assert 0 < k < blocks - 1, f"source {s} faded in {k} of {blocks} callbacks"


def odd_only(params):
    """The case with the even sources' taps held at the first draw: on a wave that owns several sources, changed and
    unchanged ones alternate."""
    out, first = [], params[0]
    cache = {}
    for p in params:
        if id(p) not in cache:
            q = p.copy()
            q["er_gain"][::2], q["er_delay"][::2] = first["er_gain"][::2], first["er_delay"][::2]
            cache[id(p)] = q
        out.append(cache[id(p)])
    return out


def assert_covered(params, F, R, sources):
    """er_ref's whole table lay on taps with a non-zero gain of the given sources, over the case."""
    inside, outside = er_ref.edge_delays(F, R)
    seen = {int(d) for p in params for s in sources for d, g in zip(p["er_delay"][s], p["er_gain"][s]) if g != 0.0}
    assert set(inside + outside) <= seen, f"the case misses {sorted(set(inside + outside) - seen)}"


# ---- 1. [ER], one source: frame for frame ------------------------------------------------------------------------------


@pytest.mark.parametrize("FR", SHAPES + [(256, 8192)], ids=_ids)
def test_one_source_is_the_composed_reference(gas, FR):
    F, R = FR
    params, srcs = E.inputs(F, R, 1, seed=R - F)
    want, bank = fade_blocks(F, R, params, srcs)
    both_roads(bank, len(params))
    E.check(E.render(gas, (ER,), F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE), want, what=f"fade n 1 F {F} R {R}")


# ---- 2. [ER] summed, several sources per workgroup, odd sources republished ----------------------------------------------


@pytest.mark.parametrize("n", [9, 24])
@pytest.mark.parametrize("FR", SHAPES, ids=_ids)
def test_summed_with_changed_and_unchanged_sources_side_by_side(gas, FR, n):
    F, R = FR
    params, srcs = E.inputs(F, R, n, seed=R + F)
    params = odd_only(params)
    want, bank = fade_blocks(F, R, params, srcs)
    both_roads(bank, len(params), sources=range(1, n, 2))
    assert all(k == 0 for k in bank.faded()[::2])
    assert_covered(params, F, R, range(1, n, 2) if n == 24 else range(n))  # the fading sources alone hold the table at n = 24
    E.check(E.render(gas, (ER,), F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE), want, what=f"fade odd sources n {n} F {F} R {R}")


def test_two_sources_on_one_wave(gas):
    """n = 2049 (test_gpu_er_edges: the smallest n at which a wave owns two sources), 5 callbacks, odd sources republished:
    the wave's first source fades or not, its second the other way round, each with ITS slot's old row."""
    F, R, n = 128, 256, 2049
    params, srcs = E.inputs(F, R, n, seed=2049, blocks=5)
    params = odd_only(params)
    want, bank = fade_blocks(F, R, params, srcs)
    assert bank.faded()[0] == 0 and bank.faded()[1] == 1
    E.check(E.render(gas, (ER,), F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE), want, what="fade 2049")


# ---- 3. staged chains: rows_out as first and as later stage -------------------------------------------------------------


@pytest.mark.parametrize("chain_name", ["er_amplify", "highshelf_er"])
@pytest.mark.parametrize("FR", SHAPES, ids=_ids)
def test_staged_chains(gas, ob, FR, chain_name):
    """[ER, AMPLIFY]: k_er_only<FADE> writing rows_out as the first stage; the reference's rows times the amplifier's gain.
    [HIGHSHELF, ER]: as the second stage, over a ping-pong buffer's rows; the reference fed the oracle's [HIGHSHELF] rows
    (float64), the shelf being untouched by the flag."""
    F, R = FR
    n = 24
    params, srcs = E.inputs(F, R, n, seed=R + F)
    if chain_name == "er_amplify":
        chain = (ER, AMPLIFY)
        want, bank = fade_blocks(F, R, params, srcs, amplify=True)
    else:
        chain = (HS, ER)
        shelves = [ob.BatchOracle(ob.KIND_EFFECT, 1, F, chain=[HS], er_ring_frames=R) for _ in range(n)]  # one per source: its mix is the row
        shelved = []
        for p, x in zip(params, srcs):
            po = E.clamped(p, F, R).astype(ob.PARAMS_DTYPE)
            shelved.append(np.stack([shelves[s].block(po[s : s + 1], x[s : s + 1], want64=True)[2][0] for s in range(n)]))
        want, bank = fade_blocks(F, R, params, shelved)
    both_roads(bank, len(params))
    E.check(E.render(gas, chain, F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE), want, what=f"fade {chain_name} F {F} R {R}")


# ---- 4. [ER, HRTF] on a flagged context: a staged chain -----------------------------------------------------------------


@pytest.mark.parametrize("FR", SHAPES, ids=_ids)
def test_er_hrtf_unit_impulse_is_the_closed_form(gas, FR):
    K = gas.capi
    F, R = FR
    n = 24
    params, srcs = E.inputs(F, R, n, seed=5, gain_one=True)
    exact = E.third(n)
    want, bank = fade_blocks(F, R, params, srcs, through_hrtf=True)
    both_roads(bank, len(params))
    got = E.render(gas, (ER, HRTF), F, R, params, srcs, flags=K.FLAG_ER_TAP_FADE | K.FLAG_PEAKS_DRAINING_ONLY, draining=np.flatnonzero(exact), hrir=E._hrir("impulse"))
    E.check(got, want, exact, what=f"fade [ER, HRTF] impulse F {F} R {R}")


def test_gas_uni_er_does_not_fuse_a_flagged_tail(gas, monkeypatch):
    """[AMPLIFY, ER, HRTF] with GAS_UNI_ER=2 ("always k_hrtf_uni<ER>"): on a flagged context the tail stays two launches, so
    the early-reflection stage fades.  Everything is linear: the closed form of [ER, HRTF] times the amplifier's gain."""
    K = gas.capi
    F, R, n = 128, 256, 24
    monkeypatch.setenv("GAS_UNI_ER", "2")
    params, srcs = E.inputs(F, R, n, seed=5, gain_one=True)
    want, bank = fade_blocks(F, R, params, srcs, through_hrtf=True, amplify=True)
    both_roads(bank, len(params))
    got = E.render(gas, (AMPLIFY, ER, HRTF), F, R, params, srcs, flags=K.FLAG_ER_TAP_FADE, hrir=E._hrir("impulse"))
    E.check(got, want, what="fade [AMPLIFY, ER, HRTF] under GAS_UNI_ER=2")


@pytest.mark.parametrize("blend", [False, True], ids=["alone", "interpolate_blend_fade"])
@pytest.mark.parametrize("FR", SHAPES, ids=_ids)
def test_er_hrtf_against_the_oracles_hrtf_fed_the_reference_rows(gas, ob, FR, blend):
    """The HRTF stage is not touched by the flag: the oracle's [HRTF] (hrtf_blend_fade_ref's composition of it under
    FLAG_HRTF_INTERPOLATE | FLAG_HRTF_BLEND_FADE) fed the composed reference's early-reflection rows, cast to f32 as the
    device's rows are.  Alone, the last stage is k_hrtf_uni: exact peaks for the draining third, +inf for the rest; under
    the HRTF flags it is k_hrtf_rows_blend_fade plus k_rows_accumulate, whose peaks are exact for every source."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, R = FR
    n = 9
    params, srcs = E.inputs(F, R, n, seed=R + F)
    exact = E.third(n)
    bank = er_fade_ref.ErFadeBank(n, F, R)
    hrir = E._hrir()
    rng = np.random.default_rng(F)
    blends = [synth.draw_blends(rng, n, E.DIRS) for _ in params] if blend else None
    if blend:
        ref = hrtf_blend_fade_ref.BlendFadeReference(ob, n, F, (HRTF,), hrir, er_ring_frames=R)
    else:
        ora = ob.BatchOracle(ob.KIND_EFFECT, n, F, chain=[HRTF], hrir=hrir, er_ring_frames=R)
    want = []
    for b, (p, x) in enumerate(zip(params, srcs)):
        rows32 = bank.block(p, x).astype(np.float32)
        if blend:
            _, rpk, m64 = ref.block(E.clamped(p, F, R), blends[b], rows32)
        else:
            _, rpk, m64 = ora.block(E.clamped(p, F, R).astype(ob.PARAMS_DTYPE), rows32, want64=True)
            m64 = m64[0]
        want.append((m64, rpk))
    both_roads(bank, len(params))
    flags = K.FLAG_ER_TAP_FADE | K.FLAG_PEAKS_DRAINING_ONLY | ((K.FLAG_HRTF_INTERPOLATE | K.FLAG_HRTF_BLEND_FADE) if blend else 0)
    got = E.render(gas, (ER, HRTF), F, R, params, srcs, flags=flags, draining=np.flatnonzero(exact), hrir=hrir, blends=blends)
    E.check(got, want, None if blend else exact, what=f"fade [ER, HRTF] {'blend fade' if blend else 'alone'} F {F} R {R}")


# ---- 5. bitwise: nothing to fade, and the clamp ------------------------------------------------------------------------


@pytest.mark.parametrize("chain", [(ER,), (ER, AMPLIFY)], ids=["er", "er_amplify"])
def test_unchanged_taps_are_an_unflagged_context_bitwise(gas, chain):
    """The same row republished every third callback: the flagged context compares, finds nothing and takes the unflagged
    loop -- mix and peaks array_equal with a context that was never told about the flag."""
    F, R, n = 128, 256, 24
    params, srcs = E.inputs(F, R, n, seed=R + F)
    params = [params[0]] * len(params)
    plain = E.render(gas, chain, F, R, params, srcs)
    flagged = E.render(gas, chain, F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE)
    for (ma, pa), (mb, pb) in zip(plain, flagged):
        assert np.isfinite(ma).all() and np.abs(ma).max() > 0
        np.testing.assert_array_equal(ma, mb)
        np.testing.assert_array_equal(pa, pb)


@pytest.mark.parametrize("FR", SHAPES, ids=_ids)
def test_out_of_range_delays_are_the_clamped_ones_bitwise(gas, FR):
    F, R = FR
    params, srcs = E.inputs(F, R, 24, seed=R + F)
    assert any((p["er_delay"] > R - F).any() for p in params)
    raw = E.render(gas, (ER,), F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE)
    twin = E.render(gas, (ER,), F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE, clamp=True)
    for (ma, pa), (mb, pb) in zip(raw, twin):
        assert np.isfinite(ma).all() and np.abs(ma).max() > 0
        np.testing.assert_array_equal(ma, mb)
        np.testing.assert_array_equal(pa, pb)


# ---- 6. changes of one kind ---------------------------------------------------------------------------------------------


def test_single_kind_changes(gas):
    """Two sources, F = 128, R = 256, a new row at callbacks 3, 6, 9, 12: gains only; delays only; the delay of the
    zero-gain tap only (a changed word, two equal renders); that tap's gain 0.0 -> -0.0 (likewise).  The reference counts
    four fades per source."""
    from godot_audio_spatializer_amd import synth

    F, R, n, T = 128, 256, 2, 15
    rng = np.random.default_rng(6)
    p = synth.draw_params(rng, n, dirs=E.DIRS, ring_frames=R, frames=F)
    p["er_gain"] = (0.7 ** np.arange(1, 9)) * np.array([1, -1, 1, 1, -1, 1, -1, 1])
    p["er_gain"][:, 3] = 0.0
    p["er_delay"] = [[1, 63, 64, 5, 65, 127, 128, 2], [128, 2, 127, 9, 1, 64, 63, 65]]
    steps = [p]
    q = p.copy()
    q["er_gain"][:, [0, 5]] *= -0.5
    steps.append(q)
    q = q.copy()
    q["er_delay"][:, [1, 6]] = [[128, 1], [64, 126]]
    steps.append(q)
    q = q.copy()
    q["er_delay"][:, 3] = 77
    steps.append(q)
    q = q.copy()
    q["er_gain"][:, 3] = -0.0
    steps.append(q)
    assert np.signbit(q["er_gain"][:, 3]).all()
    params = [steps[b // 3] for b in range(T)]
    srcs = [synth.draw_sources(rng, n, F) for _ in range(T)]
    want, bank = fade_blocks(F, R, params, srcs)
    assert bank.faded() == [4, 4]
    E.check(E.render(gas, (ER,), F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE), want, what="fade single-kind changes")


# ---- 7. left out, reset, free and re-alloc ------------------------------------------------------------------------------


def test_a_playback_left_out_fades_from_the_taps_it_last_rendered_with(gas):
    """Three sources, nine callbacks, rows republished to all of them at callbacks 3 and 6.  Source 1 is off the list from
    callback 2 to 7: at 8 it fades from the first draw (rendered at callback 1) to the third, over its own history."""
    F, R, n, T = 128, 256, 3, 9
    params, srcs = E.inputs(F, R, n, seed=71, blocks=T)
    active_of = lambda b: [0, 2] if 2 <= b <= 7 else [0, 1, 2]  # noqa: E731
    want, bank = fade_blocks(F, R, params, srcs, active_of=active_of)
    assert bank.faded() == [2, 1, 2]
    E.check(E.render(gas, (ER,), F, R, params, srcs, flags=gas.capi.FLAG_ER_TAP_FADE, active_of=active_of), want, what="fade left out")


@pytest.mark.parametrize("how", ["reset", "free_realloc"])
def test_reset_and_reused_slots_do_not_fade(gas, how):
    """A playback renders three callbacks with one row; then a new row is published and the slot is reset (or freed and,
    a callback later, handed out again): its next block is bitwise the first block of a fresh flagged context given the
    same row and input.  A second, silent playback rides along in both contexts so that the lists match."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, R = 128, 256
    rng = np.random.default_rng(8)
    drawer = er_ref.TapDrawer(rng, F, R)
    rows = []
    for _ in range(2):
        p = synth.draw_params(rng, 2, dirs=E.DIRS, ring_frames=R, frames=F)
        p["er_delay"], p["er_gain"] = drawer.draw(2)
        rows.append(p)
    rows[1][1] = rows[0][1]  # the silent playback keeps its row
    xs = synth.draw_sources(rng, 5, F)
    silent = np.zeros((F, 2), np.float32)

    def fresh_first_block():
        with gas.SpatializerContext(max_sources=2, frames=F, er_ring_frames=R, flags=K.FLAG_ER_TAP_FADE) as c:
            s = c.source_alloc_many(2, K.KIND_EFFECT, (ER,))
            c.params_publish_batch(s, rows[1])
            return c.process_block(np.stack([xs[4], silent]), s)

    with gas.SpatializerContext(max_sources=2, frames=F, er_ring_frames=R, flags=K.FLAG_ER_TAP_FADE) as c:
        s = c.source_alloc_many(2, K.KIND_EFFECT, (ER,))
        c.params_publish_batch(s, rows[0])
        for t in range(3):
            c.process_block(np.stack([xs[t], silent]), s)
        if how == "reset":
            c.params_publish_batch(s, rows[1])
            c.source_reset(int(s[0]))
        else:
            c.source_free(int(s[0]))  # takes effect at the next callback
            c.process_block(silent[None], s[1:])
            again = c.source_alloc(K.KIND_EFFECT, (ER,))
            assert again == s[0]
            c.params_publish_batch(s, rows[1])
        mix, pk = c.process_block(np.stack([xs[4], silent]), s)
        nofade = np.stack([xs[3], silent])  # and the block after it, the same row: the unflagged loop
        c.process_block(nofade, s)
    want_mix, want_pk = fresh_first_block()
    assert np.abs(mix).max() > 0
    np.testing.assert_array_equal(mix, want_mix)
    np.testing.assert_array_equal(pk, want_pk)


# ---- 8. continuity ------------------------------------------------------------------------------------------------------


def test_dc_is_continuous_on_the_device(gas):
    """x = 1, delays 1 .. 8, all gains 0.1 -> 0.5 between callbacks 1 and 2.  Flagged: the mix steps by at most sum|dg| / F
    (+ 1e-6 for f32) into and out of the fade block.  Unflagged: by more than 3 into callback 2."""
    K = gas.capi
    F, R = 128, 256
    p = np.zeros(1, K.PARAMS_DTYPE)
    p["er_delay"] = np.arange(1, 9)
    x = np.ones((1, F, 2), np.float32)
    plan = [0.1, 0.1, 0.5, 0.5]
    total = float(np.abs(np.full(8, 0.5, np.float32).astype(np.float64) - np.full(8, 0.1, np.float32).astype(np.float64)).sum())
    jumps = {}
    for name, flags in (("flagged", K.FLAG_ER_TAP_FADE), ("unflagged", 0)):
        with gas.SpatializerContext(max_sources=1, frames=F, er_ring_frames=R, flags=flags) as c:
            s = c.source_alloc_many(1, K.KIND_EFFECT, (ER,))
            y = []
            for g in plan:
                p["er_gain"] = g
                c.params_publish_batch(s, p)
                y.append(c.process_block(x, s)[0][0].astype(np.float64))
        jumps[name] = [float(np.abs(y[b + 1][0] - y[b][-1]).max()) for b in (1, 2)]
        inner = float(np.abs(np.diff(y[2], axis=0)).max())
        print(f"{name}: jump into the changed block {jumps[name][0]:.6f}, out of it {jumps[name][1]:.6f}, largest step inside {inner:.6f}")
        if name == "flagged":
            assert inner <= total / F + 1e-6
    assert max(jumps["flagged"]) <= total / F + 1e-6
    assert jumps["unflagged"][0] > 3


# ---- 9. with the tap generator -----------------------------------------------------------------------------------------


def test_generated_taps_fade_end_to_end(gas):
    """One source walks across a box room; gas_calc_early_reflections writes its taps on the device (device poses, the
    slot's row) every second callback.  The output is the composed reference's fed the taps the slot-less mode hands back
    for the same poses."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    f, ring, T = 256, 1024, 8
    rng = np.random.default_rng(9)
    room = er_rooms_ref.unit_room(half_extent=(2.0, 1.5, 1.8))
    lis = [0.4, -0.3, 0.2]
    start, step = np.array([[-1.7, 1.0, -1.2]]), np.array([[0.9, -0.45, 0.6]])
    with gas.SpatializerContext(max_sources=1, frames=f, er_ring_frames=ring, flags=K.FLAG_ER_TAP_FADE) as c:
        slots = c.source_alloc_many(1, K.KIND_EFFECT, (ER,))
        c.params_publish_batch(slots, synth.draw_params(rng, 1, dirs=16, ring_frames=ring, frames=f))
        bank = er_fade_ref.ErFadeBank(1, f, ring)
        q = np.zeros(1, K.PARAMS_DTYPE)
        worst, seen = 0.0, set()
        for b in range(T):
            if b % 2 == 0:
                pos = start + (b // 2) * step
                taps = RM.generate(gas, c, room, None, pos, lis, None, mem="device")
                wrote = RM.generate(gas, c, room, None, pos, lis, slots, mem="device")
                assert wrote.tobytes() == taps.tobytes() and (taps["gain"] > 0).sum() >= 4
                q["er_gain"], q["er_delay"] = taps["gain"], taps["delay"]
                seen.add(taps.tobytes())
            x = synth.draw_sources(rng, 1, f)
            mix, pk = c.process_block(x, slots)
            rows = bank.block(q, x)
            e = rel_rms(mix[0], rows.sum(axis=0))
            worst = max(worst, e)
            assert e <= TOL, f"callback {b}: mix rel rms {e:.3e}"
            np.testing.assert_allclose(pk, np.abs(rows).max(axis=1), err_msg=f"callback {b}", **E.PEAK_TOL)
        assert len(seen) == T // 2 and bank.faded() == [T // 2 - 1]
        print(f"fade with generated taps: worst mix rel rms {worst:.3e}")


# ---- 10. the bus and stream entries -------------------------------------------------------------------------------------


@pytest.mark.parametrize("entry", ["buses", "streams_fed"])
def test_other_entries_reach_the_fading_launch(gas, entry):
    """[ER], 9 sources.  gas_process_block_buses over two buses (source s on bus s % 2, no sends): each bus is the sum of
    its sources' reference rows.  gas_process_block_streams with every row fed (float32 stereo): the mix is the
    reference's."""
    K = gas.capi
    F, R, n = 128, 256, 9
    params, srcs = E.inputs(F, R, n, seed=R + F)
    bank = er_fade_ref.ErFadeBank(n, F, R)
    worst = 0.0
    with gas.SpatializerContext(max_sources=n, frames=F, er_ring_frames=R, flags=K.FLAG_ER_TAP_FADE) as c:
        slots = c.source_alloc_many(n, K.KIND_EFFECT, (ER,))
        if entry == "buses":
            routes = K.bus_routes(n)
            routes["dry_bus"] = np.arange(n) % 2
            c.bus_routes_publish(slots, routes)
        for b, (p, x) in enumerate(zip(params, srcs)):
            if b % 3 == 0:
                c.params_publish_batch(slots, p)
            rows = bank.block(p, x)
            if entry == "buses":
                mix, pk = c.process_block_buses(x, slots, 2)
                got = [mix[0, 0], mix[1, 0]]
                want = [rows[0::2].sum(axis=0), rows[1::2].sum(axis=0)]
            else:
                c.source_feed_rows(slots, x)
                mix, pk, hf = c.process_block_streams(slots)
                assert hf.all()
                got, want = [mix[0]], [rows.sum(axis=0)]
            for g, w in zip(got, want):
                e = rel_rms(g, w)
                worst = max(worst, e)
                assert e <= TOL, f"{entry} callback {b}: mix rel rms {e:.3e}"
            np.testing.assert_allclose(pk, np.abs(rows).max(axis=1), err_msg=f"{entry} callback {b}", **E.PEAK_TOL)
    both_roads(bank, len(params))
    print(f"fade through {entry}: worst mix rel rms {worst:.3e}")
