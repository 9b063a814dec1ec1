"""gas_process_block_streams_buses (include/gas_amd.h): gas_process_block_buses over the windows that
gas_process_block_streams would have produced for the same list.

The yardstick is the library's own float-row bus entry.  A *twin* context has the same slots, parameters, routes and
HRTF table and runs process_block_buses on rows produced by tests/stream_window_ref.py: Playback (which
test_gpu_stream_ends.py pins to the sampler bit for bit; test_gpu_buses.py pins the bus entry to the oracle).  Mix,
peaks, has_frames and stream_positions are compared with np.array_equal at every callback, until every playback that
can end has ended and two callbacks beyond.

Two routes: rows first (k_sample_sources -> k_sample_adpcm -> k_sample_qoa into the staging rows, then
the device path of the bus entry) for 3D-mix sources, staged chains and [HRTF] lists with resampled / compressed
playbacks; fused (k_hrtf_uni<SRC_PCM, BUS2>, one launch per pair of buses) for plain [HRTF] lists.  The fused form is
also held against the same list in a context created with GAS_STREAM_ROWS_FIRST=1.

Sources per wave in the fused form: k_hrtf_uni runs min(ceil(n / 8), 256) workgroups of 8 waves, so n = 2049 is the
first size at which a wave carries two sources (test_gpu_stream_ends.py's header)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest

import adpcm_ref as aref
import qoa_ref as qref
import stream_loop_ref as lref
import stream_window_ref as wref

pytestmark = pytest.mark.gpu

LIMIT = 16  # callbacks a run may take; looped references are unrolled this far
INVALID_ARGUMENT, NO_HRTF, UNSUPPORTED_CHAIN = -1, -5, -6


@dataclass
class PB:
    """One playback: `create` are stream_create's arguments, `ref` the PCM stream_window_ref.Playback reads."""

    create: tuple
    ref: np.ndarray
    start: int = 0
    pitch: float = None  # a number: a resampled playback at that pitch
    loop: tuple = None  # (mode, begin, end)


def plain(rng, frames, fmt, start=0, pitch=None, loop=None):
    pcm = wref.make_pcm(rng, frames, fmt)
    return PB((pcm,), pcm, start, pitch, loop)


def reference(pb, F):
    if pb.loop is not None:  # a looped playback is a plain playback over the unrolled stream, which never ends here
        mode, b, e = pb.loop
        return wref.Playback(lref.unroll(pb.ref, b, e, mode, pb.start + LIMIT * F + 64 + 4 + F), pb.start)
    return wref.Playback(pb.ref, pb.start, resampled=pb.pitch is not None)


def position(pb, ref):
    return int(lref.loop_map(ref.position, pb.loop[1], pb.loop[2], pb.loop[0])) if pb.loop is not None else ref.position


def create_streams(ctx, pbs):
    """One stream per entry of pbs, its playback class and loop set."""
    sids = []
    for pb in pbs:
        sid = ctx.stream_create(*pb.create)
        if pb.pitch is not None:
            ctx.stream_set_resampled(sid, True)
        if pb.loop is not None:
            ctx.stream_set_loop(sid, *pb.loop)
        sids.append(sid)
    return sids


def random_routes(K, rng, n, n_buses, channels=1, more=True):
    """Dry bus anywhere, a send for six in ten, and (more) up to four further sends onto distinct buses."""
    r = K.bus_routes(n)
    r["dry_bus"] = rng.integers(0, n_buses, n)
    for s in range(n):
        order = rng.permutation(n_buses)
        k_sends = int(rng.integers(0, min(n_buses, 1 + K.MAX_MORE_SENDS) + 1)) if more else int(rng.uniform() < 0.6)
        for k in range(k_sends):
            vol = np.zeros((K.MAX_CHANNELS, 2), np.float32)
            vol[:channels] = rng.uniform(0.0, 1.2, (channels, 2))
            if k == 0:
                r["send_bus"][s], r["send"][s] = order[k], vol
            else:
                r["more_bus"][s, k - 1], r["more_send"][s, k - 1] = order[k], vol
    return r


def draw(rng, pbs, F, channels=1, ring=0, dirs=8):
    from godot_audio_spatializer_amd import synth

    p = synth.draw_params(rng, len(pbs), dirs=dirs, channel_count=channels, ring_frames=max(ring, 2 * F), frames=F)
    for i, pb in enumerate(pbs):
        if pb.pitch is not None:
            p["pitch_scale"][i] = pb.pitch
    return p


class Rows:
    """The reference windows of one scene, computed once per (key) and shared: per callback (rows, has_frames,
    positions), until every playback that can end has ended and `past` callbacks beyond."""

    _cache = {}

    @classmethod
    def of(cls, key, pbs, who, starts, F, past=2):
        if key not in cls._cache:
            refs = []
            for i, w in enumerate(who):
                pb = pbs[w]
                refs.append((pb, reference(PB(pb.create, pb.ref, int(starts[i]), pb.pitch, pb.loop), F)))
            steps, after = [], 0
            for cb in range(LIMIT):
                ended = all(not r.has_frames for pb, r in refs if pb.loop is None)
                rows = np.stack([r.block(F, pb.pitch if pb.pitch is not None else 1.0) for pb, r in refs])
                hf = np.array([r.has_frames for _, r in refs])
                pos = np.array([position(pb, r) for pb, r in refs], np.uint64)
                for a in (rows, hf, pos):
                    a.setflags(write=False)
                steps.append((rows, hf, pos))
                after += ended
                if after == past:
                    break
            else:
                raise AssertionError("the scene never ended")
            cls._cache[key] = steps
        return cls._cache[key]


def exact(got, want, where):
    for g, w, what in zip(got, want, ("mix", "peaks", "has_frames", "positions")):
        assert np.array_equal(g, w), f"{what}, {where}"


def run(ctxs, pbs, who, starts, slots, F, n_buses, key, before=None):
    """Every stream context against the one named "twin" at every callback; returns the twin's mixes."""
    twin, tslots = ctxs["twin"], slots["twin"]
    stream_ctxs = {name: ctx for name, ctx in ctxs.items() if name != "twin"}
    steps = Rows.of(key, pbs, who, starts, F)
    n = len(who)
    mixes = []
    was = np.ones(n, bool)
    for cb, (rows, hf, pos) in enumerate(steps):
        if before is not None:
            before(cb)
        want, wpk = twin.process_block_buses(rows, tslots, n_buses)
        for j in np.flatnonzero(was & ~hf):  # the streams entry marks ended playbacks draining; the twin's caller does it
            twin.source_set_draining(int(tslots[j]), True)
        was = hf
        for name, ctx in stream_ctxs.items():
            got, gpk, ghf = ctx.process_block_streams_buses(slots[name], n_buses)
            exact((got, gpk, ghf, ctx.stream_positions(n)), (want, wpk, hf, pos), f"{name}, callback {cb} of {len(steps)}")
        mixes.append(want)
    assert not steps[-1][1][[pbs[w].loop is None for w in who]].any()
    return np.stack(mixes)


def table_scene(rng, F, n):
    """Streams of every length of wref.lengths(F), formats in rotation, and one GAS_LOOP_PINGPONG stream whose seams fall
    inside a block; n playbacks over them, starts from wref.starts (so every (length, start) of wref.cases(F) occurs from
    n = 128 or so on): playbacks end inside a callback (mixed < F), fade out and feed zero rows next to neighbours that
    go on."""
    lens = wref.lengths(F)
    pbs = [plain(rng, L, wref.FORMATS[(i + i // 4) % 4]) for i, L in enumerate(lens)]
    pbs.append(plain(rng, 300, "s16_stereo", loop=(lref.LOOP_PINGPONG, 40, 200)))  # 160-frame loop: a seam in every block
    if n == 1:
        who, starts = [lens.index(2 * F - 64)], [1]
    else:
        who = [len(pbs) - 1] + [(5 * i + 3) % len(lens) for i in range(n - 1)]  # 5 is coprime to the 14 / 16 lengths
        starts = [17] + [wref.starts(lens[w])[(i // len(lens)) % len(wref.starts(lens[w]))] for i, w in enumerate(who[1:])]
    return pbs, who, starts


def open_contexts(gas, monkeypatch, names, n, F, channels=1, ring=0):
    """Contexts by name; "rows_first" is created with GAS_STREAM_ROWS_FIRST=1 (read at context creation)."""
    out = {}
    for name in names:
        if name == "rows_first":
            monkeypatch.setenv("GAS_STREAM_ROWS_FIRST", "1")
        out[name] = gas.SpatializerContext(max_sources=n, frames=F, channel_count=channels, er_ring_frames=ring)
        if name == "rows_first":
            monkeypatch.delenv("GAS_STREAM_ROWS_FIRST")
    return out


def close_all(ctxs):
    for ctx in ctxs.values():
        ctx.close()


def populate(ctxs, kind, chain, pbs, who, starts, params, routes, hrir):
    slots = {}
    for name, ctx in ctxs.items():
        if hrir is not None:
            ctx.hrtf_load(hrir)
        s = ctx.source_alloc_many(len(who), kind, chain)
        ctx.params_publish_batch(s, params)
        ctx.bus_routes_publish(s, routes)
        if name != "twin":
            sids = create_streams(ctx, pbs)
            for i, w in enumerate(who):
                ctx.source_bind_stream(s[i], sids[w], start_frame=int(starts[i]))
        slots[name] = s
    return slots


def small_scene(seed, F, n):
    """n playbacks of their own streams: lengths and starts drawn from wref.cases(F), one of them 3 F + 200 from 0.
    Returns the scene and the key its reference rows are shared under."""
    rng = np.random.default_rng(seed)
    cases = wref.cases(F)
    picks = [cases[int(k)] for k in rng.choice(len(cases), n - 1, replace=False)] + [(3 * F + 200, 0)]
    pbs = [plain(rng, L, wref.FORMATS[i % 4], start=s) for i, (L, s) in enumerate(picks)]
    return pbs, list(range(n)), [pb.start for pb in pbs], ("small", seed, F, n)


def hrir8():
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(7), dirs=8)


# ---- rows first ----


@pytest.mark.parametrize("F", [128, 512])
@pytest.mark.parametrize("n_buses", [1, 2, 6])
@pytest.mark.parametrize("channels", [1, 4])
def test_rows_first_3d_mix(gas, monkeypatch, channels, n_buses, F):
    K = gas.capi
    n = 7
    rng = np.random.default_rng(100 + F)
    pbs, who, starts, key = small_scene(101, F, n)
    params = draw(rng, pbs, F, channels)
    routes = random_routes(K, np.random.default_rng(n_buses), n, n_buses, channels)
    ctxs = open_contexts(gas, monkeypatch, ("streams", "twin"), n, F, channels)
    try:
        slots = populate(ctxs, K.KIND_3D_MIX, (), pbs, who, starts, params, routes, None)
        mixes = run(ctxs, pbs, who, starts, slots, F, n_buses, key)
        assert mixes.shape[1:] == (n_buses, channels, F, 2) and all(mixes[:, b].any() for b in set(routes["dry_bus"]))
    finally:
        close_all(ctxs)


@pytest.mark.parametrize("F", [128, 512])
@pytest.mark.parametrize("n_buses", [2, 3])
@pytest.mark.parametrize("chain_name", ["er_hrtf", "shelf", "shelf_hrtf"])
def test_rows_first_staged_chains(gas, monkeypatch, chain_name, n_buses, F):
    """The staged chains of test_gpu_buses.test_effect_kinds_route_to_buses (its "hrtf" is the fused form, below)."""
    K = gas.capi
    HS, ER, HRTF = K.FX_HIGHSHELF, K.FX_EARLY_REFLECTIONS, K.FX_HRTF
    chain = {"er_hrtf": (ER, HRTF), "shelf": (HS,), "shelf_hrtf": (HS, HRTF)}[chain_name]
    ring = 2048 if ER in chain else 0
    n = 5
    rng = np.random.default_rng(200 + F)
    pbs, who, starts, key = small_scene(201, F, n)
    params = draw(rng, pbs, F, ring=ring)
    routes = random_routes(K, np.random.default_rng(n_buses), n, n_buses)
    ctxs = open_contexts(gas, monkeypatch, ("streams", "twin"), n, F, ring=ring)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, chain, pbs, who, starts, params, routes, hrir8())
        mixes = run(ctxs, pbs, who, starts, slots, F, n_buses, key)
        assert mixes.any()
    finally:
        close_all(ctxs)


@pytest.mark.parametrize("F", [128, 512])
def test_rows_first_hrtf_of_every_stream_kind(gas, monkeypatch, F):
    """An [HRTF] list of s16 and f32, mono and stereo, one resampled playback (pitch 0.97), one IMA-ADPCM and one QOA
    playback: the compressed and the resampled ones send the whole list through the samplers, then the fused two-bus
    form over the rows, two passes for three buses."""
    K = gas.capi
    rng = np.random.default_rng(300 + F)
    pbs = [plain(rng, L, fmt, start=s) for fmt, (L, s) in zip(wref.FORMATS, ((F + 1, 0), (2 * F - 64, 63), (3, 1), (3 * F + 200, 64)))]
    pbs.append(plain(rng, 2 * F + 1, "s16_stereo", start=5, pitch=0.97))
    frames = 2 * F + 37
    codes = rng.integers(0, 16, (frames, 2)).astype(np.uint8)
    dec = np.stack([aref.decode_channel(codes[:, k]) for k in range(2)], axis=1)
    pbs.append(PB((aref.pack(codes), K.PCM_IMA_ADPCM, 2, frames), np.ascontiguousarray(dec), start=9))
    qframes = F + 90
    file = qref.random_file(rng, qframes, 1)
    pbs.append(PB((file, K.PCM_QOA, 1, qframes), np.ascontiguousarray(qref.decode(file, 1, qframes)), start=0))
    n, n_buses = len(pbs), 3
    who, starts = list(range(n)), [pb.start for pb in pbs]
    params = draw(rng, pbs, F)
    routes = random_routes(K, rng, n, n_buses)
    routes["send_bus"][0], routes["send"][0, 0] = 2, (0.7, 0.4)  # somebody reaches the second pass
    ctxs = open_contexts(gas, monkeypatch, ("streams", "twin"), n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), pbs, who, starts, params, routes, hrir8())
        mixes = run(ctxs, pbs, who, starts, slots, F, n_buses, ("kinds", F))
        assert all(mixes[:, b].any() for b in range(n_buses))
    finally:
        close_all(ctxs)


# ---- fused ----


@pytest.mark.parametrize("F", [128, 512])
@pytest.mark.parametrize("n_buses", [1, 2, 3, 6])
@pytest.mark.parametrize("n", [1, 3, 2049])
def test_fused_form(gas, monkeypatch, n, n_buses, F):
    """Plain [HRTF] lists: k_hrtf_uni<SRC_PCM, BUS2> against the twin (float rows, k_hrtf_uni<BUS2>) and against the same
    list in a GAS_STREAM_ROWS_FIRST=1 context, all bitwise: mix, peaks, has_frames, positions.  k_hrtf_uni.hip writes
    its FMAs out, so the stream-sampling and the float-row instantiation compute the same bits at every F."""
    K = gas.capi
    rng = np.random.default_rng(400 + F)
    pbs, who, starts = table_scene(rng, F, n)
    params = draw(np.random.default_rng(n), [pbs[w] for w in who], F)
    routes = random_routes(K, np.random.default_rng(10 * n + n_buses), n, n_buses)
    ctxs = open_contexts(gas, monkeypatch, ("fused", "rows_first", "twin"), n, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), pbs, who, starts, params, routes, hrir8())
        mixes = run(ctxs, pbs, who, starts, slots, F, n_buses, ("table", F, n))
        assert all(mixes[:, b].any() for b in set(routes["dry_bus"]))
    finally:
        close_all(ctxs)


@pytest.mark.parametrize("F", [128, 512])
def test_cursor_moves_in_the_committing_pass_only(gas, monkeypatch, F):
    """Three buses are two passes of the fused form.  A playback that ends inside the block and sends onto bus 2: were
    the cursor advanced by pass 0, pass 1 would sample the block after the end (zeros) and bus 2 would miss the tail."""
    K = gas.capi
    rng = np.random.default_rng(500 + F)
    pbs = [plain(rng, F + 30, "s16_mono"), plain(rng, 2 * F + 63, "f32_stereo", start=1)]
    who, starts = [0, 1], [0, 1]
    params = draw(rng, pbs, F)
    routes = K.bus_routes(2)
    routes["send_bus"], routes["send"][:, 0] = 2, (0.5, 0.25)
    ctxs = open_contexts(gas, monkeypatch, ("fused", "twin"), 2, F)
    try:
        slots = populate(ctxs, K.KIND_EFFECT, (K.FX_HRTF,), pbs, who, starts, params, routes, hrir8())
        mixes = run(ctxs, pbs, who, starts, slots, F, 3, ("commit", F))
        assert mixes[1, 2].any() and mixes[2, 2].any() and not mixes[:, 1].any()  # bus 2 carries the ending blocks
    finally:
        close_all(ctxs)


# ---- failures ----


def raw_call(ctx, K, slots, n_buses, F, channels):
    s = np.ascontiguousarray(slots, np.uint32)
    out = np.full((7, channels, F, 2), np.nan, np.float32)
    pk = np.zeros((max(len(s), 1), 2), np.float32)
    hf = np.full(max(len(s), 1), 7, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = ctx.lib.gas_process_block_streams_buses(ctx.h, vp(s), len(s), F, vp(out), n_buses, vp(pk), vp(hf), K.MEM_HOST)
    return rc, out


@pytest.mark.parametrize("what", ["n_buses 0", "n_buses 7", "kinds mixed", "chain on four pairs", "no hrtf", "slot twice"])
def test_failed_callback_moves_nothing(gas, monkeypatch, what):
    """Each refusal answers its status with a zeroed host `out` and leaves every cursor where it was: the valid calls
    around it equal the twin's, which never saw the failure."""
    K = gas.capi
    F, n, n_buses = 128, 3, 2
    channels = 4 if what == "chain on four pairs" else 1
    mix_list = what == "chain on four pairs"  # the list that runs validly: 3D mix there, [HRTF] elsewhere
    rng = np.random.default_rng(600)
    pbs = [plain(rng, F + 40, "s16_mono"), plain(rng, 2 * F + 1, "f32_stereo", start=3), plain(rng, 3 * F, "s16_stereo")]
    who, starts = [0, 1, 2], [0, 3, 0]
    params = draw(rng, pbs, F, channels)
    routes = random_routes(K, rng, n, n_buses, channels)
    hrir = hrir8()
    ctxs = open_contexts(gas, monkeypatch, ("streams", "twin"), n + 2, F, channels)
    try:
        ctx, twin = ctxs["streams"], ctxs["twin"]
        kind, chain = (K.KIND_3D_MIX, ()) if mix_list else (K.KIND_EFFECT, (K.FX_HRTF,))
        twin.hrtf_load(hrir)
        if what != "no hrtf":
            ctx.hrtf_load(hrir)
        slots = populate({"streams": ctx, "twin": twin}, kind, chain, pbs, who, starts, params, routes, None)
        s = slots["streams"]
        # two more playbacks of the other kind, bound and ready, for the lists that mix kinds
        other = ctx.source_alloc_many(2, *((K.KIND_EFFECT, (K.FX_HRTF,)) if mix_list else (K.KIND_3D_MIX, ())))
        ctx.params_publish_batch(other, params[:2])
        sid = ctx.stream_create(pbs[2].ref)
        for o in other:
            ctx.source_bind_stream(o, sid)
        bad_slots, bad_buses, status = s, n_buses, INVALID_ARGUMENT
        if what == "n_buses 0":
            bad_buses = 0
        elif what == "n_buses 7":
            bad_buses = 7
        elif what == "kinds mixed":
            bad_slots, status = [s[0], other[0], s[1]], UNSUPPORTED_CHAIN
        elif what == "chain on four pairs":
            bad_slots, status = list(other), UNSUPPORTED_CHAIN
        elif what == "no hrtf":
            status = NO_HRTF
        elif what == "slot twice":
            bad_slots = [s[0], s[1], s[0]]
        steps = Rows.of(("fail", F), pbs, who, starts, F)
        for cb, (rows, hf, pos) in enumerate(steps):
            if cb == (0 if what == "no hrtf" else 1):  # in mid-stream, with a cached list behind it
                rc, out = raw_call(ctx, K, bad_slots, bad_buses, F, channels)
                assert rc == status
                assert not out[: min(bad_buses, 6)].any() and np.isnan(out[min(bad_buses, 6):]).all()
                if what == "no hrtf":
                    ctx.hrtf_load(hrir)
            want, wpk = twin.process_block_buses(rows, slots["twin"], n_buses)
            got, gpk, ghf = ctx.process_block_streams_buses(s, n_buses)
            exact((got, gpk, ghf, ctx.stream_positions(n)), (want, wpk, hf, pos), f"callback {cb}")
    finally:
        close_all(ctxs)


# ---- steady state ----


@pytest.mark.parametrize("form", ["3d_mix", "fused", "staged"])
def test_same_list_and_route_changes(gas, monkeypatch, form):
    """The same list callback after callback (no playback ends: the host's steady-state path, which for the staged form
    must still hand the bus entry its list), then a route change between two callbacks: the next one routes by it."""
    K = gas.capi
    F, n, n_buses = 128, 4, 3
    kind, chain = {"3d_mix": (K.KIND_3D_MIX, ()), "fused": (K.KIND_EFFECT, (K.FX_HRTF,)), "staged": (K.KIND_EFFECT, (K.FX_HIGHSHELF, K.FX_HRTF))}[form]
    rng = np.random.default_rng(700)
    pbs = [plain(rng, 7 * F + 5, wref.FORMATS[i], start=i) for i in range(n)]
    who, starts = list(range(n)), list(range(n))
    params = draw(rng, pbs, F)
    routes = K.bus_routes(n)  # everybody dry on bus 0
    moved = K.bus_routes(n)
    moved["dry_bus"] = 1
    moved["send_bus"], moved["send"][:, 0] = 2, (0.5, 0.5)
    ctxs = open_contexts(gas, monkeypatch, ("streams", "twin"), n, F)
    try:
        slots = populate(ctxs, kind, chain, pbs, who, starts, params, routes, hrir8())

        def before(cb):
            if cb == 4:
                ctxs["streams"].bus_routes_publish(slots["streams"], moved)
                ctxs["twin"].bus_routes_publish(slots["twin"], moved)

        mixes = run(ctxs, pbs, who, starts, slots, F, n_buses, ("steady", F), before)
        assert mixes[:4, 0].any() and not mixes[:4, 1:].any()
        assert not mixes[4:, 0].any() and mixes[4, 1].any() and mixes[4, 2].any()
    finally:
        close_all(ctxs)


# ---- GAS_MEM_DEVICE ----


@pytest.mark.parametrize("form", ["3d_mix", "fused"])
def test_device_memory_form(gas, monkeypatch, form):
    """gas_process_block_streams_buses(GAS_MEM_DEVICE) writes the mix and the peaks of the host form, bit for bit."""
    import torch

    K = gas.capi
    F, n, n_buses = 128, 9, 3
    channels = 2 if form == "3d_mix" else 1
    kind, chain = (K.KIND_3D_MIX, ()) if form == "3d_mix" else (K.KIND_EFFECT, (K.FX_HRTF,))
    rng = np.random.default_rng(800)
    pbs, who, starts, _ = small_scene(801, F, n)
    params = draw(rng, pbs, F, channels)
    routes = random_routes(K, rng, n, n_buses, channels)
    ctxs = open_contexts(gas, monkeypatch, ("host", "dev"), n, F, channels)
    try:
        slots = populate(ctxs, kind, chain, pbs, who, starts, params, routes, hrir8())
        d_out = torch.full((n_buses, channels, F, 2), float("nan"), device="cuda")
        d_pk = torch.zeros(n, 2, device="cuda")
        torch.cuda.synchronize()
        dev = ctxs["dev"]
        s32 = np.ascontiguousarray(slots["dev"], np.uint32)
        heard = 0
        for cb in range(8):
            want, wpk, whf = ctxs["host"].process_block_streams_buses(slots["host"], n_buses)
            hf = np.full(n, 7, np.uint8)
            rc = dev.lib.gas_process_block_streams_buses(dev.h, s32.ctypes.data_as(C.c_void_p), n, F, C.c_void_p(d_out.data_ptr()), n_buses, C.c_void_p(d_pk.data_ptr()), hf.ctypes.data_as(C.c_void_p), K.MEM_DEVICE)
            assert rc == 0
            dev.synchronize()
            exact((d_out.cpu().numpy(), d_pk.cpu().numpy(), hf.astype(bool), dev.stream_positions(n)), (want, wpk, whf, ctxs["host"].stream_positions(n)), f"callback {cb}")
            heard += bool(want.any())
        assert heard >= 4 and not whf.any()
    finally:
        close_all(ctxs)
