"""gas_source_feed_rows (include/gas_amd.h): a stream callback whose unbound entries take window rows the caller
supplies -- host-decoded playbacks next to device-resident streams in one list.

The definition is the test: the callback's mix, peaks and bus outputs are those of gas_process_block[_buses] over the
rows R, R[i] the sampler's window where entry i is a stream playback and the converted fed row (s / 32768, mono to both
ears) where it is fed.  So the twin method of test_gpu_stream_buses.py (whose helpers are used here): a twin context
with the same slots, parameters, routes and HRIR table runs process_block[_buses] on rows composed in the test -- stream
rows from stream_window_ref.Playback, fed rows converted from the fed data, zeros for an unbound entry that is not fed --
and mix, peaks, has_frames and stream_positions are compared with np.array_equal at every callback.  Fed entries add
no arithmetic, so every case is bitwise (test_gpu_stream_buses.test_fused_form holds the all-stream fused form to its
twin bit for bit; the fused cases here rest on that).

Sources per wave in the fused form: k_hrtf_uni runs min(ceil(n / 8), 256) workgroups of 8 waves over
wave_range(n, wave, waves), so at n = 2049 wave 0 carries entries 0 and 1 and every other wave one."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest

import adpcm_ref as aref
import qoa_ref as qref
import stream_window_ref as wref
import test_gpu_stream_buses as sb

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, BAD_SLOT, FRAME_COUNT, NO_HRTF = -1, -3, -4, -5
CALLBACKS = 8


@dataclass
class Fed:
    """An entry whose slot is bound to no stream: the caller feeds its rows, in this format."""

    fmt: str


def fed_data(seed, cb, i, F, fmt):
    """What callback cb feeds entry i: drawn per (scene, callback, entry), so every run of a scene feeds the same."""
    return wref.make_pcm(np.random.default_rng([seed, cb, i]), F, fmt)


def always(cb, i):
    return True


def gaps(cb, i):
    """Fed, then not fed for one callback, then fed again: every fed entry within eight callbacks, at its own time."""
    return (cb + i // 2) % 5 != 3


class Scene:
    """The reference of one list: per callback the rows R, has_frames, positions and what is fed (entry -> data).
    entries[i] is an sb.PB (a stream playback, started at starts[i]) or a Fed; fed(cb, i) says whether callback cb feeds
    entry i.  bind(i, pb, start) turns a Fed entry into a stream playback from the next step on."""

    def __init__(self, seed, entries, starts, F, fed=always):
        self.seed, self.F, self.fed, self.cb = seed, F, fed, 0
        self.entries = list(entries)
        self.refs = [None if isinstance(e, Fed) else sb.reference(sb.PB(e.create, e.ref, int(s), e.pitch, e.loop), F) for e, s in zip(entries, starts)]

    def bind(self, i, pb, start):
        self.entries[i] = pb
        self.refs[i] = sb.reference(sb.PB(pb.create, pb.ref, int(start), pb.pitch, pb.loop), self.F)

    def step(self):
        F, n = self.F, len(self.entries)
        rows = np.zeros((n, F, 2), np.float32)
        hf = np.zeros(n, bool)
        pos = np.zeros(n, np.uint64)
        feeds = {}
        for i, (e, r) in enumerate(zip(self.entries, self.refs)):
            if r is not None:
                rows[i] = r.block(F, e.pitch if e.pitch is not None else 1.0)
                hf[i], pos[i] = r.has_frames, sb.position(e, r)
            elif self.fed(self.cb, i):
                feeds[i] = fed_data(self.seed, self.cb, i, F, e.fmt)
                rows[i], hf[i] = wref.to_float_stereo(feeds[i]), True
        self.cb += 1
        for a in (rows, hf, pos):
            a.setflags(write=False)
        return rows, hf, pos, feeds


class Steps:
    """The steps of a scene that several tests (or cases of one) run, computed once and shared."""

    _cache = {}

    @classmethod
    def of(cls, key, make, callbacks=CALLBACKS):
        if key not in cls._cache:
            scene = make()
            cls._cache[key] = [scene.step() for _ in range(callbacks)]
        return cls._cache[key]


def feed(ctx, slots, feeds):
    """One call per format present (several calls accumulate)."""
    by_shape = {}
    for i, data in feeds.items():
        by_shape.setdefault((data.dtype.str, data.ndim), []).append(i)
    for idx in by_shape.values():
        ctx.source_feed_rows(np.asarray(slots)[idx], np.stack([feeds[i] for i in idx]))


def twin_call(twin, rows, tslots, n_buses):
    return twin.process_block(rows, tslots) if n_buses is None else twin.process_block_buses(rows, tslots, n_buses)


def stream_call(ctx, slots, n_buses):
    return ctx.process_block_streams(slots) if n_buses is None else ctx.process_block_streams_buses(slots, n_buses)


def run(ctxs, steps, slots, n_buses, before=None):
    """Every stream context against the one named "twin" at every callback; returns the twin's mixes.  The twin's
    caller marks draining what the streams entry marks itself: a playback that ended, an unbound entry left unfed."""
    twin, tslots = ctxs["twin"], slots["twin"]
    n = len(tslots)
    mixes = []
    was = np.ones(n, bool)
    for cb, (rows, hf, pos, feeds) in enumerate(steps):
        if before is not None:
            before(cb)
        want, wpk = twin_call(twin, rows, tslots, n_buses)
        for j in np.flatnonzero(was & ~hf):
            twin.source_set_draining(int(tslots[j]), True)
        was = hf
        for name, ctx in ctxs.items():
            if name == "twin":
                continue
            feed(ctx, slots[name], feeds)
            got, gpk, ghf = stream_call(ctx, slots[name], n_buses)
            if name in ("fused", "rows_first"):  # a fused context may not fall back because an entry is fed
                assert ctx.stream_last_fused() == (name == "fused"), f"{name}, callback {cb}"
            sb.exact((got, gpk, ghf, ctx.stream_positions(n)), (want, wpk, hf, pos), f"{name}, callback {cb} of {len(steps)}")
        mixes.append(want)
    return np.stack(mixes)


def populate(ctxs, kind, chain, entries, starts, params, routes, hrir):
    """Same slots, parameters, routes and HRIRs everywhere; the stream contexts bind the stream entries."""
    slots = {}
    for name, ctx in ctxs.items():
        if hrir is not None:
            ctx.hrtf_load(hrir)
        s = ctx.source_alloc_many(len(entries), kind, chain)
        ctx.params_publish_batch(s, params)
        if routes is not None:
            ctx.bus_routes_publish(s, routes)
        if name != "twin":
            sids = {}  # one stream per distinct playback description, however many entries play it
            for i, e in enumerate(entries):
                if not isinstance(e, Fed):
                    if id(e) not in sids:
                        sids[id(e)] = sb.create_streams(ctx, [e])[0]
                    ctx.source_bind_stream(s[i], sids[id(e)], start_frame=int(starts[i]))
        slots[name] = s
    return slots


def with_fed(pbs, who, starts, fed_first, shift=0):
    """The playbacks of a stream scene with every second entry fed instead (formats in rotation)."""
    entries = []
    for i, w in enumerate(who):
        is_fed = (i % 2 == 0) == fed_first
        entries.append(Fed(wref.FORMATS[(i // 2 + shift) % 4]) if is_fed else pbs[w])
    return entries, list(starts)


def draw_for(rng, entries, F, channels=1, ring=0):
    from godot_audio_spatializer_amd import synth

    p = synth.draw_params(rng, len(entries), dirs=8, channel_count=channels, ring_frames=max(ring, 2 * F), frames=F)
    for i, e in enumerate(entries):
        if not isinstance(e, Fed) and e.pitch is not None:
            p["pitch_scale"][i] = e.pitch
    return p


# ---- fused ----


def wave_entries(n, wave):
    """wave_range of csrc/gas_hrtf_wave.h for k_hrtf_uni's grid."""
    waves = 8 * min((n + 7) // 8, 256)
    base, rem = divmod(n, waves)
    first = wave * base + min(wave, rem)
    return list(range(first, first + base + (wave < rem)))


@pytest.mark.parametrize("F", [128, 512])
@pytest.mark.parametrize("n_buses", [None, 1, 3])
@pytest.mark.parametrize("n,first", [(1, "fed"), (3, "fed"), (3, "stream"), (2049, "fed"), (2049, "stream")])
def test_fused_hrtf_lists_with_fed_entries(gas, monkeypatch, n, first, n_buses, F):
    """Plain [HRTF] lists stay on k_hrtf_uni<SRC_PCM> / k_hrtf_uni<SRC_PCM, BUS2> (three buses: two passes) with every
    second entry fed, in all four formats, each fed entry left unfed for one callback on the way: against the twin and
    against the same list in a GAS_STREAM_ROWS_FIRST=1 context.  The stream entries are test_fused_form's table scene,
    so playbacks end and fade next to fed neighbours.  At n = 2049 the two-source wave holds a fed and a stream source,
    in either order."""
    K = gas.capi
    rng = np.random.default_rng(400 + F)
    pbs, who, starts = sb.table_scene(rng, F, n)
    entries, starts = with_fed(pbs, who, starts, first == "fed")
    if n == 2049:
        pair = wave_entries(n, 0)
        assert pair == [0, 1] and all(len(wave_entries(n, w)) == 1 for w in (1, 2, 2047))
        assert [isinstance(entries[i], Fed) for i in pair] == ([True, False] if first == "fed" else [False, True])
        assert {e.fmt for e in entries if isinstance(e, Fed)} == set(wref.FORMATS)
    params = draw_for(np.random.default_rng(n), entries, F)
    routes = None if n_buses is None else sb.random_routes(K, np.random.default_rng(10 * n + n_buses), n, n_buses)
    steps = Steps.of(("fused", F, n, first), lambda: Scene(7000 + F, entries, starts, F, gaps))
    first_fed = 0 if first == "fed" else 1
    assert steps[2][1][first_fed] and not steps[3][1][first_fed] and steps[4][1][first_fed]  # fed, not fed, fed again
    ctxs = sb.open_contexts(gas, monkeypatch, ("fused", "rows_first", "twin"), n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), entries, starts, params, routes, sb.hrir8())
        mixes = run(ctxs, steps, slots, n_buses)
        assert mixes.any()
    finally:
        sb.close_all(ctxs)


@pytest.mark.parametrize("fmt", wref.FORMATS)
def test_one_fed_source_in_each_format(gas, monkeypatch, fmt):
    """n = 1, F = 128: the whole callback is one fed row, read in its own format by either route."""
    K = gas.capi
    F = 128
    entries, starts = [Fed(fmt)], [0]
    params = draw_for(np.random.default_rng(1), entries, F)
    steps = Steps.of(("one", fmt), lambda: Scene(7100, entries, starts, F, gaps), 5)
    ctxs = sb.open_contexts(gas, monkeypatch, ("fused", "rows_first", "twin"), 1, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), entries, starts, params, None, sb.hrir8())
        mixes = run(ctxs, steps, slots, None)
        assert mixes[0].any() and steps[3][1][0] == 0  # callback 3 finds it unfed
    finally:
        sb.close_all(ctxs)


# ---- rows first ----


@pytest.mark.parametrize("n_buses", [None, 2])
@pytest.mark.parametrize("n", [1, 5, 70])
def test_rows_first_staged_chain(gas, monkeypatch, n, n_buses):
    """[HIGHSHELF, HRTF]: the sampler launch writes the fed rows into the staging rows, the staged chain runs over them."""
    K = gas.capi
    F = 128
    pbs, who, starts, key = sb.small_scene(901, F, n)
    entries, starts = with_fed(pbs, who, starts, True)
    params = draw_for(np.random.default_rng(900 + n), entries, F)
    routes = None if n_buses is None else sb.random_routes(K, np.random.default_rng(n), n, n_buses)
    steps = Steps.of(("staged",) + key, lambda: Scene(7200, entries, starts, F, gaps))
    ctxs = sb.open_contexts(gas, monkeypatch, ("streams", "twin"), n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HIGHSHELF, K.FX_HRTF), entries, starts, params, routes, sb.hrir8())
        assert run(ctxs, steps, slots, n_buses).any()
    finally:
        sb.close_all(ctxs)


@pytest.mark.parametrize("n_buses", [None, 3])
@pytest.mark.parametrize("n", [1, 5, 70])
def test_rows_first_3d_mix_on_two_pairs(gas, monkeypatch, n, n_buses):
    K = gas.capi
    F, channels = 128, 2
    pbs, who, starts, key = sb.small_scene(902, F, n)
    entries, starts = with_fed(pbs, who, starts, False if n > 1 else True, shift=1)
    params = draw_for(np.random.default_rng(910 + n), entries, F, channels)
    routes = None if n_buses is None else sb.random_routes(K, np.random.default_rng(n), n, n_buses, channels)
    steps = Steps.of(("mix",) + key, lambda: Scene(7300, entries, starts, F, gaps))
    ctxs = sb.open_contexts(gas, monkeypatch, ("streams", "twin"), n, F, channels)
    try:
        slots = populate(ctxs, K.KIND_3D_MIX, (), entries, starts, params, routes, None)
        mixes = run(ctxs, steps, slots, n_buses)
        assert mixes.shape[-3:] == (channels, F, 2) and mixes.any()
    finally:
        sb.close_all(ctxs)


@pytest.mark.parametrize("n_buses", [None, 3])
def test_rows_first_hrtf_list_of_every_stream_kind_and_fed_entries(gas, monkeypatch, n_buses):
    """An [HRTF] list with a resampled, an IMA-ADPCM and a QOA playback: the whole list is sampled first, k_sample_adpcm
    and k_sample_qoa run behind k_sample_sources and leave the fed rows alone."""
    K = gas.capi
    F = 128
    rng = np.random.default_rng(920)
    pbs = [sb.plain(rng, 2 * F + 1, "s16_stereo", start=5, pitch=0.97), sb.plain(rng, 3 * F, "f32_mono", start=1)]
    frames = 2 * F + 37
    codes = rng.integers(0, 16, (frames, 2)).astype(np.uint8)
    dec = np.stack([aref.decode_channel(codes[:, k]) for k in range(2)], axis=1)
    pbs.append(sb.PB((aref.pack(codes), K.PCM_IMA_ADPCM, 2, frames), np.ascontiguousarray(dec), start=9))
    qframes = F + 90
    file = qref.random_file(rng, qframes, 1)
    pbs.append(sb.PB((file, K.PCM_QOA, 1, qframes), np.ascontiguousarray(qref.decode(file, 1, qframes)), start=0))
    entries = [Fed("s16_mono"), pbs[0], Fed("f32_stereo"), pbs[2], Fed("s16_stereo"), pbs[3], pbs[1], Fed("f32_mono")]
    starts = [0 if isinstance(e, Fed) else e.start for e in entries]
    n = len(entries)
    params = draw_for(rng, entries, F)
    routes = None if n_buses is None else sb.random_routes(K, rng, n, n_buses)
    steps = Steps.of(("kinds",), lambda: Scene(7400, entries, starts, F, gaps))
    ctxs = sb.open_contexts(gas, monkeypatch, ("streams", "twin"), n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), entries, starts, params, routes, sb.hrir8())
        assert run(ctxs, steps, slots, n_buses).any()
    finally:
        sb.close_all(ctxs)


@pytest.mark.parametrize("n_buses", [None, 2])
@pytest.mark.parametrize("chain_name", ["hrtf", "shelf_hrtf"])
def test_fed_entries_at_any_pitch_scale(gas, monkeypatch, chain_name, n_buses):
    """pitch_scale is the sampler's input: a playback that is bound to no stream has been decoded at its pitch by whoever
    feeds it, and gas_process_block never looks at the field.  Fed entries with pitch_scale 0.7 .. 2 next to plain
    streams at pitch 1: the callback is accepted and equals the twin's, on the fused route and rows first, also in the
    callbacks that find an entry unfed."""
    K = gas.capi
    F, n = 128, 6
    chain = (K.FX_HRTF,) if chain_name == "hrtf" else (K.FX_HIGHSHELF, K.FX_HRTF)
    pbs, who, starts, key = sb.small_scene(903, F, n)
    entries, starts = with_fed(pbs, who, starts, True)
    params = draw_for(np.random.default_rng(990), entries, F)
    params["pitch_scale"][0::2] = (0.7, 1.3, 2.0)
    routes = None if n_buses is None else sb.random_routes(K, np.random.default_rng(n), n, n_buses)
    steps = Steps.of(("pitch",) + key, lambda: Scene(7900, entries, starts, F, gaps))
    names = ("fused", "rows_first", "twin") if chain_name == "hrtf" else ("streams", "twin")
    ctxs = sb.open_contexts(gas, monkeypatch, names, n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, chain, entries, starts, params, routes, sb.hrir8())
        assert run(ctxs, steps, slots, n_buses).any()
    finally:
        sb.close_all(ctxs)


# ---- lifetimes under an unchanged list ----


@pytest.mark.parametrize("route", ["fused", "rows_first"])
def test_lifetimes_under_an_unchanged_list(gas, monkeypatch, route):
    """Ten callbacks of one list (the same_list steady state): entry 0 is fed, left unfed for two callbacks -- the silent
    row, has_frames = 0 -- and fed again; entry 1's stream ends inside callback 2 and fades out next to fed neighbours;
    entry 3 is fed, left alone, and bound to a stream before callback 5; entries 2 and 5 are fed throughout."""
    K = gas.capi
    F, callbacks = 128, 10
    rng = np.random.default_rng(930)
    late = sb.plain(rng, 3 * F + 17, "s16_stereo")
    entries = [Fed("f32_stereo"), sb.plain(rng, 2 * F + 30, "s16_mono"), Fed("s16_stereo"), Fed("f32_mono"), sb.plain(rng, 20 * F, "f32_stereo", start=3), Fed("s16_mono")]
    starts = [0, 0, 0, 0, 3, 0]
    n = len(entries)

    def fed(cb, i):
        return {0: cb not in (3, 4), 3: cb < 4}.get(i, True)

    def make():
        scene, out = Scene(7500, entries, starts, F, fed), []
        for cb in range(callbacks):
            if cb == 5:
                scene.bind(3, late, 2)
            out.append(scene.step())
        return out

    key = ("lifetimes",)
    if key not in Steps._cache:
        Steps._cache[key] = make()
    steps = Steps._cache[key]
    assert [bool(s[1][0]) for s in steps] == [True] * 3 + [False] * 2 + [True] * 5 and not steps[3][0][0].any()
    assert steps[1][1][1] and not steps[2][1][1] and steps[2][0][1].any()  # the stream's last, fading block
    assert not steps[4][1][3] and steps[5][1][3] and steps[5][2][3] == 2 + F
    params = draw_for(rng, entries, F)
    ctxs = sb.open_contexts(gas, monkeypatch, (route, "twin"), n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), entries, starts, params, None, sb.hrir8())

        def before(cb):
            if cb == 5:  # gas_source_bind_stream clears the mark the unfed callback left; the twin's caller does it
                ctx = ctxs[route]
                ctx.source_bind_stream(slots[route][3], sb.create_streams(ctx, [late])[0], start_frame=2)
                ctxs["twin"].source_set_draining(int(slots["twin"][3]), False)

        assert run(ctxs, steps, slots, None, before).any()
    finally:
        sb.close_all(ctxs)


# ---- refusals and the state of a pending row ----


def small(gas, monkeypatch, F=128, load_hrir=True, spare=2):
    """Three entries -- fed, a stream, fed -- of an [HRTF] list, `spare` more slots allocated behind them."""
    K = gas.capi
    rng = np.random.default_rng(940)
    entries = [Fed("f32_stereo"), sb.plain(rng, 30 * F, "s16_stereo", start=1), Fed("s16_mono")]
    starts = [0, 1, 0]
    params = draw_for(rng, entries + [Fed("f32_mono")] * spare, F)
    ctxs = sb.open_contexts(gas, monkeypatch, ("streams", "twin"), len(entries) + spare, F)
    hrir = sb.hrir8()
    slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), entries + [Fed("f32_mono")] * spare, starts + [0] * spare, params, None, hrir if load_hrir else None)
    if not load_hrir:
        ctxs["twin"].hrtf_load(hrir)
    return ctxs, slots, Scene(7600, entries, starts, F), hrir


def raw_feed(ctx, K, slots, rows, fmt, channels, frames, mem=0):
    s = np.ascontiguousarray(slots, np.uint32)
    r = np.ascontiguousarray(rows)
    return ctx.lib.gas_source_feed_rows(ctx.h, s.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), fmt, channels, len(s), frames, mem)


def check(ctxs, slots, rows, hf, pos, n, where):
    """One callback of the first n entries on both sides, nothing fed here."""
    want, wpk = ctxs["twin"].process_block(rows[:n], slots["twin"][:n])
    got, gpk, ghf = ctxs["streams"].process_block_streams(slots["streams"][:n])
    sb.exact((got, gpk, ghf, ctxs["streams"].stream_positions(n)), (want, wpk, hf[:n], pos[:n]), where)


@pytest.mark.parametrize("what", ["no hrtf", "slot twice"])
def test_pending_rows_survive_a_callback_that_fails_validation(gas, monkeypatch, what):
    K = gas.capi
    ctxs, slots, scene, hrir = small(gas, monkeypatch, load_hrir=what != "no hrtf")
    try:
        ctx, s = ctxs["streams"], slots["streams"]
        for cb in range(3):
            rows, hf, pos, feeds = scene.step()
            feed(ctx, s, feeds)
            if cb == (0 if what == "no hrtf" else 1):
                bad = np.ascontiguousarray(s[:3] if what == "no hrtf" else [s[0], s[1], s[0]], np.uint32)
                out = np.full((1, 128, 2), np.nan, np.float32)
                rc = ctx.lib.gas_process_block_streams(ctx.h, bad.ctypes.data_as(C.c_void_p), 3, 128, out.ctypes.data_as(C.c_void_p), None, None, K.MEM_HOST)
                assert rc == (NO_HRTF if what == "no hrtf" else INVALID_ARGUMENT) and not out.any()
                if what == "no hrtf":
                    ctx.hrtf_load(hrir)
            check(ctxs, slots, rows, hf, pos, 3, f"callback {cb}")  # the rows fed before the refusal are used here
            assert hf[0] and hf[2]
    finally:
        sb.close_all(ctxs)


def test_a_second_feed_replaces_the_first_and_calls_accumulate(gas, monkeypatch):
    """Slot 0 is fed three times before each callback, in three formats, next to a row that stays: the last feed counts
    (and the feed table closes the holes the replaced rows leave when it runs out of room)."""
    ctxs, slots, scene, _ = small(gas, monkeypatch)
    try:
        ctx, s = ctxs["streams"], slots["streams"]
        for cb in range(4):
            rows, hf, pos, feeds = scene.step()
            other = np.stack([fed_data(3, cb, k, 128, "f32_stereo") for k in range(2)])
            ctx.source_feed_rows(s[[0, 2]], other)
            ctx.source_feed_rows(s[[2, 0]], other)  # every pending row replaced at once: the table starts over
            ctx.source_feed_rows(s[[2]], feeds[2][None])
            for k, fmt in enumerate(("s16_stereo", "f32_mono")):
                ctx.source_feed_rows(s[[0]], fed_data(1, cb, k, 128, fmt)[None])
            ctx.source_feed_rows(s[[0]], feeds[0][None])
            check(ctxs, slots, rows, hf, pos, 3, f"callback {cb}")
    finally:
        sb.close_all(ctxs)


def test_a_pending_row_of_a_slot_off_the_list_is_dropped(gas, monkeypatch):
    ctxs, slots, scene, _ = small(gas, monkeypatch)
    try:
        ctx, s = ctxs["streams"], slots["streams"]
        rows, hf, pos, feeds = scene.step()
        feed(ctx, s, feeds)  # entries 0 and 2
        check(ctxs, slots, rows, hf, pos, 2, "the list without entry 2")
        ctxs["twin"].source_set_draining(int(slots["twin"][2]), True)
        rows, hf, pos, feeds = scene.step()
        ctx.source_feed_rows(s[[0]], feeds[0][None])
        silent = rows.copy()
        silent[2] = 0
        unfed = hf.copy()
        unfed[2] = False
        check(ctxs, slots, silent, unfed, pos, 3, "entry 2 back on the list, its row gone")
    finally:
        sb.close_all(ctxs)


ERRORS = ["format 2", "format 3", "format 4", "format -1", "channels 0", "channels 3", "mem 2", "bound slot", "slot twice", "slot not in use", "slot out of range", "frame count"]


@pytest.mark.parametrize("what", ERRORS)
def test_every_error_leaves_nothing_taken(gas, monkeypatch, what):
    """Each refused call names the unbound entry 0 (with a good row) as well: the next callback finds it unfed."""
    K = gas.capi
    F = 128
    ctxs, slots, scene, _ = small(gas, monkeypatch)
    try:
        ctx, s = ctxs["streams"], slots["streams"]
        rows, hf, pos, feeds = scene.step()
        good = np.stack([feeds[0], feeds[0]])
        call = dict(slots=[s[0], s[2]], rows=good, fmt=K.PCM_F32, channels=2, frames=F, mem=K.MEM_HOST)
        status = INVALID_ARGUMENT
        if what.startswith("format"):
            call["fmt"] = int(what.split()[1])
        elif what.startswith("channels"):
            call["channels"] = int(what.split()[1])
        elif what == "mem 2":
            call["mem"] = 2
        elif what == "bound slot":
            call["slots"] = [s[0], s[1]]
        elif what == "slot twice":
            call["slots"] = [s[0], s[0]]
        elif what == "slot not in use":
            ctx.source_free(s[4])
            ctx.process_block_streams(s[:0])  # the free takes effect at a block boundary
            call["slots"], status = [s[0], s[4]], BAD_SLOT
        elif what == "slot out of range":
            call["slots"], status = [s[0], 5], BAD_SLOT
        elif what == "frame count":
            call["frames"], status = F - 1, FRAME_COUNT
        assert raw_feed(ctx, K, call["slots"], call["rows"], call["fmt"], call["channels"], call["frames"], call["mem"]) == status
        silent = rows.copy()
        silent[[0, 2]] = 0
        unfed = hf.copy()
        unfed[[0, 2]] = False
        check(ctxs, slots, silent, unfed, pos, 3, what)
    finally:
        sb.close_all(ctxs)


@pytest.mark.parametrize("what", ["free", "reset", "bind_stream"])
def test_free_reset_and_bind_drop_the_pending_row(gas, monkeypatch, what):
    K = gas.capi
    F = 128
    ctxs, slots, scene, _ = small(gas, monkeypatch)
    try:
        ctx, twin, s, t = ctxs["streams"], ctxs["twin"], slots["streams"], slots["twin"]
        rows, hf, pos, feeds = scene.step()
        feed(ctx, s, feeds)
        if what == "free":  # the slot comes back at a block boundary; its next playback must not inherit the row
            # (an empty gas_process_block is that boundary: it applies the free and leaves the feed table alone, so only
            # the free itself can have dropped the row -- and entry 0's row is still pending afterwards)
            ctx.source_free(s[2])
            twin.source_free(t[2])
            none = np.zeros((0, F, 2), np.float32)
            ctx.process_block(none, s[:0])
            twin.process_block(none, t[:0])
            s[2], t[2] = ctx.source_alloc(K.KIND_EFFECT, (K.FX_HRTF,)), twin.source_alloc(K.KIND_EFFECT, (K.FX_HRTF,))
            p = draw_for(np.random.default_rng(5), [Fed("s16_mono")], F)
            ctx.params_publish_batch(s[[2]], p)
            twin.params_publish_batch(t[[2]], p)
        elif what == "reset":
            ctx.source_reset(s[2])
            twin.source_reset(t[2])
        else:  # the stream supplies entry 2's window from here on; entry 0's pending row stays
            pb = sb.plain(np.random.default_rng(6), 9 * F, "f32_mono")
            ctx.source_bind_stream(s[2], sb.create_streams(ctx, [pb])[0], start_frame=0)
            rows, hf, pos, _ = Scene(7600, [scene.entries[0], scene.entries[1], pb], [0, 1, 0], F).step()
            check(ctxs, slots, rows, hf, pos, 3, what)
            assert hf.all() and pos[2] == F
            return
        silent = rows.copy()
        silent[2] = 0
        unfed = hf.copy()
        unfed[2] = False
        check(ctxs, slots, silent, unfed, pos, 3, what)
    finally:
        sb.close_all(ctxs)


@pytest.mark.parametrize("n_buses", [None, 3])
def test_device_memory_form(gas, monkeypatch, n_buses):
    """mem = GAS_MEM_DEVICE for the rows and for the outputs: the host form's bits."""
    import torch

    K = gas.capi
    F = 128
    rng = np.random.default_rng(950)
    pbs, who, starts, _ = sb.small_scene(951, F, 9)
    entries, starts = with_fed(pbs, who, starts, True)
    n = len(entries)
    params = draw_for(rng, entries, F)
    routes = sb.random_routes(K, rng, n, n_buses or 1)
    ctxs = sb.open_contexts(gas, monkeypatch, ("host", "dev"), n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), entries, starts, params, routes, sb.hrir8())
        scene = Scene(7700, entries, starts, F, gaps)
        dev, s32 = ctxs["dev"], np.ascontiguousarray(slots["dev"], np.uint32)
        d_out = torch.full((n_buses or 1, 1, F, 2), float("nan"), device="cuda")
        d_pk = torch.zeros(n, 2, device="cuda")
        for cb in range(6):
            _, _, _, feeds = scene.step()
            feed(ctxs["host"], slots["host"], feeds)
            want, wpk, whf = stream_call(ctxs["host"], slots["host"], n_buses)
            keep = []
            for i, data in feeds.items():  # one call per row, from device memory
                d = torch.from_numpy(data).cuda()
                keep.append(d)
                torch.cuda.synchronize()
                fmt, ch = (K.PCM_S16 if data.dtype == np.int16 else K.PCM_F32), data.ndim
                assert dev.lib.gas_source_feed_rows(dev.h, s32[i:].ctypes.data_as(C.c_void_p), C.c_void_p(d.data_ptr()), fmt, ch, 1, F, K.MEM_DEVICE) == 0
            hf = np.full(n, 7, np.uint8)
            vp = s32.ctypes.data_as(C.c_void_p)
            if n_buses is None:
                rc = dev.lib.gas_process_block_streams(dev.h, vp, n, F, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_pk.data_ptr()), hf.ctypes.data_as(C.c_void_p), K.MEM_DEVICE)
            else:
                rc = dev.lib.gas_process_block_streams_buses(dev.h, vp, n, F, C.c_void_p(d_out.data_ptr()), n_buses, C.c_void_p(d_pk.data_ptr()), hf.ctypes.data_as(C.c_void_p), K.MEM_DEVICE)
            assert rc == 0
            dev.synchronize()
            got = d_out.cpu().numpy() if n_buses is not None else d_out.cpu().numpy()[0]
            sb.exact((got, d_pk.cpu().numpy(), hf.astype(bool), dev.stream_positions(n)), (want, wpk, whf, ctxs["host"].stream_positions(n)), f"callback {cb}")
    finally:
        sb.close_all(ctxs)


def test_an_all_fed_list_is_process_block_on_the_same_rows(gas, monkeypatch):
    K = gas.capi
    F, n = 128, 5
    entries, starts = [Fed(wref.FORMATS[i % 4]) for i in range(n)], [0] * n
    params = draw_for(np.random.default_rng(960), entries, F)
    steps = Steps.of(("all fed",), lambda: Scene(7800, entries, starts, F), 4)
    ctxs = sb.open_contexts(gas, monkeypatch, ("fused", "rows_first", "twin"), n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), entries, starts, params, None, sb.hrir8())
        assert run(ctxs, steps, slots, None).any() and all(s[1].all() for s in steps)
    finally:
        sb.close_all(ctxs)


def test_an_all_stream_list_is_untouched_by_feeds_elsewhere(gas, monkeypatch):
    """The all-stream list of a context that keeps being fed (rows for a slot off the list, dropped callback after
    callback) equals the list of a context that never saw a feed."""
    K = gas.capi
    F, n = 128, 7
    pbs, who, starts, _ = sb.small_scene(971, F, n)
    entries = [pbs[w] for w in who] + [Fed("f32_stereo")]
    params = draw_for(np.random.default_rng(970), entries, F)
    ctxs = sb.open_contexts(gas, monkeypatch, ("fed", "never"), n + 1, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), entries, list(starts) + [0], params, None, sb.hrir8())
        heard = 0
        for cb in range(8):
            ctxs["fed"].source_feed_rows(slots["fed"][[n]], fed_data(2, cb, 0, F, "f32_stereo")[None])
            got = ctxs["fed"].process_block_streams(slots["fed"][:n])
            want = ctxs["never"].process_block_streams(slots["never"][:n])
            sb.exact(got + (ctxs["fed"].stream_positions(n),), want + (ctxs["never"].stream_positions(n),), f"callback {cb}")
            heard += bool(want[0].any())
        assert heard >= 3
    finally:
        sb.close_all(ctxs)


# ---- host layer ----


def host_scene(K, F, k):
    rng = np.random.default_rng(980)
    lengths = [2 * F + 30, 5 * F, 3 * F + 1, 64, 4 * F + 63, F][: 2 * k]
    pcm = [wref.make_pcm(rng, m, "s16_stereo") for m in lengths]
    return pcm, [wref.to_float_stereo(p) for p in pcm]


def test_mixed_host_equals_the_all_array_host(gas):
    """k array playbacks and k device-stream playbacks of the same s16 data in one gas_host_set_mixed host, against a
    host that plays all 2 k as arrays, started in the same order: the mix of every callback and every playback's
    active flag, until all are reaped.

    Bitwise.  An all-device-stream host and an all-array host of these playbacks were compared on the commit before
    this feature and agreed bit for bit in every callback (the window the host builds on the CPU -- lookahead, the f32
    fade products -- is the sampler's, and k_hrtf_uni computes the same bits from float rows and from streams), so no
    tolerance is taken.  The array playbacks carry a pitch_scale other than 1, as an emitter with doppler does."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, k = 128, 3
    pcm, arrays = host_scene(K, F, k)
    params = synth.draw_params(np.random.default_rng(981), 2 * k, dirs=8, frames=F)
    params["pitch_scale"][0::2] = (0.8, 1.25, 2.0)  # the array playbacks': the host hands it to their sampler, the stream callback must not mind
    hrir = sb.hrir8()
    with gas.SpatializerContext(max_sources=2 * k, frames=F) as ca, gas.SpatializerContext(max_sources=2 * k, frames=F) as cm:
        ca.hrtf_load(hrir)
        cm.hrtf_load(hrir)
        ha = K.BatchedSpatializerHost(ca, K.KIND_EFFECT, (K.FX_HRTF,))
        hm = K.BatchedSpatializerHost(cm, K.KIND_EFFECT, (K.FX_HRTF,))
        assert hm.set_mixed(True) == 0
        ia, im = [], []
        for i in range(2 * k):
            ia.append(ha.start_playback_array(arrays[i]))
            im.append(hm.start_playback_array(arrays[i]) if i % 2 == 0 else hm.start_playback_device_stream(cm.stream_create(pcm[i])))
            ha.set_spatializer_parameters(ia[i], params[i])
            hm.set_spatializer_parameters(im[i], params[i])
        heard = 0
        for cb in range(40):
            rca, want = ha.get_mixed_frames(0, F)
            rcm, got = hm.get_mixed_frames(0, F)
            assert rca == 0 and rcm == 0 and np.array_equal(got, want), f"callback {cb}"
            assert [hm.is_playback_active(i) for i in im] == [ha.is_playback_active(i) for i in ia], f"callback {cb}"
            assert [hm.get_playback_position(i) for i in im] == [ha.get_playback_position(i) for i in ia], f"callback {cb}"
            heard += bool(want.any())
            if ha.playback_count() == 0 and hm.playback_count() == 0:
                break
        else:
            raise AssertionError("the playbacks never ended")
        assert heard >= 5
        ha.close()
        hm.close()


def test_set_mixed_is_opt_in_and_comes_first(gas):
    K = gas.capi
    with gas.SpatializerContext(max_sources=4, frames=128) as ctx:
        host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT)
        assert host.set_mixed(True) == 0 and host.set_mixed(False) == 0  # off again: the default
        host.start_playback_array(np.zeros((256, 2), np.float32))
        with pytest.raises(gas.GasError) as ei:
            host.start_playback_device_stream(ctx.stream_create(np.zeros(256, np.int16)))
        assert ei.value.status == -10
        assert host.set_mixed(True) == INVALID_ARGUMENT  # a playback has started
        host.close()
        host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT)
        assert host.set_mixed(True) == 0
        host.start_playback_device_stream(ctx.stream_create(np.zeros(256, np.int16)))
        host.start_playback_array(np.zeros((256, 2), np.float32))
        assert host.set_mixed(False) == INVALID_ARGUMENT
        host.close()
