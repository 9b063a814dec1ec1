"""GAS_PCM_QOA streams (include/gas_amd.h): one context plays the QOA file, a twin context plays qoa_ref.decode(...) of
it as an ordinary GAS_PCM_S16 stream -- the contract is that the two behave alike in every entry.  With empty chains and
zero parameters the mix is the sum of the rows, so out, peaks (one per row), has_frames and gas_stream_positions must be
equal bit for bit after every callback.  test_qoa_reference.py pins qoa_ref to two hand-worked examples (no independent
QOA decoder can be had where these tests run); test_gpu_stream_ends.py and test_gpu_stream_loops.py pin the GAS_PCM_S16
twin.  The design and the driver (run, banded) are test_gpu_stream_adpcm.py's.

Every test packs its cases into one list, one playback per case.  A QOA case plays a prefix of one of four master files
of 11 993 frames (three QOA frames, the last slice partial): `random`, random slices under random full-range state in
every frame header (both rails, predictions that wrap, weights beyond 16 bits), and `speech`, the encoded excerpt; mono
and stereo.  The decode of a prefix is the prefix of the decode, so each master is encoded and decoded once.

k_sample_qoa.hip has two ways to a frame.  The span decode applies while a row's loads stay within qoa_ref.SPAN_CHUNKS
chunks of 80 frames; the cases that exceed it, so that the per-load decode runs by itself, are the L = 5000 loops with a
seam in the window and pitch 8 at F = 512 (448 fresh frames x 8).  test_forced_per_load runs a third of every group
under GAS_QOA_SPAN=0 beside the default."""
import os
from dataclasses import dataclass

import numpy as np
import pytest

import adpcm_ref as aref
import qoa_ref as qref
import stream_window_ref as wref
from test_gpu_stream_adpcm import banded, close_rigs, run, zero_params
from test_gpu_stream_loops import loop_cases

pytestmark = pytest.mark.gpu

SPEECH = os.path.join(os.path.dirname(__file__), "golden", "speech_excerpt_s16.npy")
MASTER_FRAMES = 11993
KINDS = ["random", "speech"]
LONG_LOOP = 5000

_masters = {}
_adpcm = {}


def master(kind, ch):
    """(file, decoded int16 [frames] or [frames][2]) of MASTER_FRAMES frames; computed once and never written to."""
    if (kind, ch) not in _masters:
        if kind == "random":
            file = qref.random_file(np.random.default_rng(70 + ch), MASTER_FRAMES, ch)
        else:
            s = (np.load(SPEECH)[:MASTER_FRAMES].astype(np.int32) * 6).astype(np.int16)  # peaks near 27000
            file = qref.encode(np.stack([s, -np.roll(s, 777)][:ch], axis=1))
        dec = qref.decode(file, ch, MASTER_FRAMES)
        if kind == "random":
            assert dec.min() == -32768 and dec.max() == 32767
        file.setflags(write=False)
        dec.setflags(write=False)
        _masters[(kind, ch)] = (file, dec)
    return _masters[(kind, ch)]


def adpcm_codes(ch):
    if ch not in _adpcm:
        codes = np.random.default_rng(170 + ch).integers(0, 16, (MASTER_FRAMES, ch)).astype(np.uint8)
        _adpcm[ch] = codes[:, 0] if ch == 1 else codes
    return _adpcm[ch]


@dataclass
class PB:
    """One playback: its stream (fmt qoa: a prefix of master(kind, ch); adpcm: a prefix of adpcm_codes(ch); s16 / f32:
    pcm; all but qoa the same in every context), where it starts, its loop (mode, begin, end) and its pitch (None: not
    resampled; a number; "moving")."""

    fmt: str
    ch: int
    frames: int
    start: int = 0
    kind: str = "random"
    loop: tuple = None
    pitch: object = None
    pcm: np.ndarray = None


def setup(ctx, K, pbs, compressed, chain=(), hrir=None):
    if hrir is not None:
        ctx.hrtf_load(hrir)
    slots = ctx.source_alloc_many(len(pbs), K.KIND_EFFECT, chain)
    for slot, pb in zip(slots, pbs):
        if pb.fmt == "qoa":
            file, dec = master(pb.kind, pb.ch)
            if compressed:
                sid = ctx.stream_create(qref.prefix(file, pb.frames), K.PCM_QOA, pb.ch, pb.frames)
                assert ctx.stream_get_info(sid) == (pb.frames, pb.ch, K.PCM_QOA)
            else:
                sid = ctx.stream_create(np.ascontiguousarray(dec[: pb.frames]))
        elif pb.fmt == "adpcm":
            sid = ctx.stream_create(aref.pack(adpcm_codes(pb.ch)[: pb.frames]), K.PCM_IMA_ADPCM, pb.ch, pb.frames)
        else:
            sid = ctx.stream_create(pb.pcm)
        if pb.pitch is not None:
            ctx.stream_set_resampled(sid, True)
        if pb.loop is not None:
            ctx.stream_set_loop(sid, *pb.loop)
        ctx.source_bind_stream(slot, sid, start_frame=pb.start)
    return slots


def open_rigs(gas, monkeypatch, pbs, F, forced=False, chain=(), hrir=None, flags=0):
    """Contexts and their slots: QOA (default paths) [, QOA with GAS_QOA_SPAN=0], the GAS_PCM_S16 twin."""
    K = gas.capi
    ctxs = [gas.SpatializerContext(max_sources=len(pbs), frames=F, flags=flags)]
    if forced:
        monkeypatch.setenv("GAS_QOA_SPAN", "0")  # read at context creation
        ctxs.append(gas.SpatializerContext(max_sources=len(pbs), frames=F, flags=flags))
        monkeypatch.delenv("GAS_QOA_SPAN")
    ctxs.append(gas.SpatializerContext(max_sources=len(pbs), frames=F, flags=flags))
    return [(ctx, setup(ctx, K, pbs, compressed=k < len(ctxs) - 1, chain=chain, hrir=hrir)) for k, ctx in enumerate(ctxs)]


# ---- the three groups of cases ----

EDGES = (qref.SLICE, qref.CHUNK, qref.FRAME)  # 20, 80, 5120


def plain_pbs(F, ch, kind):
    """stream_window_ref.cases(F); lengths on either side of a slice, a chunk and a QOA frame edge (entered shortly
    before the end, so that the fade runs over the edge) and starts on either side of each; one playback through both
    frame edges to the end of the master."""
    cases = wref.cases(F)
    for e in EDGES:
        cases += [(n, max(n - 2 * F, 0)) for n in (e - 1, e, e + 1)]
        cases += [(e + F + 200, s) for s in (e - 1, e, e + 1)]
    cases.append((MASTER_FRAMES, 4700))
    assert any(n % qref.SLICE for n, _ in cases) and any(n % qref.SLICE == 0 for n, _ in cases)  # last slice partial, whole
    return [PB("qoa", ch, n, start, kind) for n, start in cases]


def loop_pbs(mode, ch):
    """loop_cases() of test_gpu_stream_loops.py (L = 1 .. 1500: a whole loop fits the span); L = 5000 with a seam in the
    window of the first callbacks (the end of the loop; for ping-pong also the turn at the end of the period) and from
    frame 0, where the window bounds the span until the seam arrives; a loop that straddles the QOA frame edge."""
    assert LONG_LOOP > qref.SPAN_FRAMES  # a seam in the window: the bounds are the whole loop, beyond the span
    out = []
    for i, (L, b, tail, start) in enumerate(loop_cases()):
        out.append(PB("qoa", ch, b + L + tail, start, KINDS[i % 2], loop=(mode, b, 0 if tail == 0 else b + L)))
    b, L = 123, LONG_LOOP
    for i, start in enumerate((b + L - 300, b + 2 * L - 300, b + L - 1500, 0)):
        out.append(PB("qoa", ch, b + L + 200, start, KINDS[i % 2], loop=(mode, b, b + L)))
    b, L = 5000, 300
    assert b < qref.FRAME < b + L
    for i, start in enumerate((b - 100, b + L // 2, b + L + 50)):
        out.append(PB("qoa", ch, b + L + 200, start, KINDS[i % 2], loop=(mode, b, b + L)))
    return out


def resampled_pbs(F, K):
    """Every pitch of stream_window_ref.PITCHES and the moving one over short streams (the lengths and starts of
    test_gpu_stream_ends.py), one of 9000 frames for the pitches from 2 up, and both loop modes.  At pitch 8 and
    F = 512 the taps of one callback exceed the span; so does the L = 5000 loop with its seam among the taps."""
    if F == 512:
        assert (F - wref.LOOKAHEAD) * max(wref.PITCHES) > qref.SPAN_FRAMES
    out = []
    i = 0
    for pitch in wref.PITCHES + ["moving"]:
        fast = pitch == "moving" or pitch >= 2.0
        for ch in (1, 2):
            for n in (1, 2, 3, 4, 5, 64, F, 2 * F + 1) + ((9000,) if fast else ()):
                for start in sorted({0, max(n - 10, 0)} | ({qref.FRAME - 300} if n == 9000 else set())):
                    out.append(PB("qoa", ch, n, start, KINDS[i % 2], pitch=pitch))
                    i += 1
            for mode in (K.LOOP_FORWARD, K.LOOP_PINGPONG):
                for L, b, tail, start in ((37, 0, 0, 0), (513, 123, 200, 123 + 513 + 50), (LONG_LOOP, 123, 200, 123 + LONG_LOOP - 700)):
                    out.append(PB("qoa", ch, b + L + tail, start, KINDS[i % 2], loop=(mode, b, b + L), pitch=pitch))
                    i += 1
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [512, 128])
@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_plain_bitwise(gas, monkeypatch, ch, F, kind):
    """To two callbacks past the last end: the fade runs over decoded frames."""
    pbs = plain_pbs(F, ch, kind)
    rigs = open_rigs(gas, monkeypatch, pbs, F)
    try:
        ran = run(gas.capi, rigs, pbs, zero_params(gas.capi, len(pbs)), limit=120)
        assert ran >= (MASTER_FRAMES - pbs[-1].start) // F + 2
    finally:
        close_rigs(rigs)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("mode", ["forward", "pingpong"])
def test_loops_bitwise(gas, monkeypatch, mode, ch):
    K = gas.capi
    pbs = loop_pbs({"forward": K.LOOP_FORWARD, "pingpong": K.LOOP_PINGPONG}[mode], ch)
    rigs = open_rigs(gas, monkeypatch, pbs, 512)
    try:
        run(K, rigs, pbs, zero_params(K, len(pbs)), callbacks=6)
    finally:
        close_rigs(rigs)


@pytest.mark.parametrize("F", [512, 128])
def test_resampled_bitwise(gas, monkeypatch, F):
    K = gas.capi
    pbs = resampled_pbs(F, K)
    rigs = open_rigs(gas, monkeypatch, pbs, F)
    try:
        run(K, rigs, pbs, zero_params(K, len(pbs)))
    finally:
        close_rigs(rigs)


@pytest.mark.parametrize("group", ["plain", "loops", "resampled"])
def test_forced_per_load(gas, monkeypatch, group):
    """GAS_QOA_SPAN=0: every load decodes from its record.  The default context, the forced one and the twin give the
    same bits, so the two paths are held against each other and against the decoded stream."""
    K = gas.capi
    F = 512
    if group == "plain":
        pbs = plain_pbs(F, 1, "random")[::3] + plain_pbs(F, 2, "speech")[1::3] + plain_pbs(F, 2, "random")[-1:]
    elif group == "loops":
        pbs = loop_pbs(K.LOOP_FORWARD, 2)[::3] + loop_pbs(K.LOOP_PINGPONG, 1)[1::3] + loop_pbs(K.LOOP_PINGPONG, 2)[-7:]
    else:
        pbs = resampled_pbs(F, K)[::3]
    rigs = open_rigs(gas, monkeypatch, pbs, F, forced=True)
    try:
        run(K, rigs, pbs, zero_params(K, len(pbs)), callbacks=6 if group == "loops" else None)
    finally:
        close_rigs(rigs)


def mixed_pbs(K):
    """70 playbacks: QOA, IMA-ADPCM, GAS_PCM_S16 and GAS_PCM_F32 streams, mono and stereo, plain, looped and resampled."""
    rng = np.random.default_rng(77)
    out = []
    for i in range(70):
        fmt = ("qoa", "s16", "adpcm", "qoa", "f32", "qoa", "adpcm")[i % 7]
        ch = 1 + (i // 7) % 2
        shape = i % 3  # 0 plain, 1 looped, 2 resampled (every other one looped as well)
        frames = 300 + 97 * i if i % 4 else 5 * 512 + 60 * i
        start = int(rng.integers(0, 200))
        loop = None
        if shape == 1 or (shape == 2 and i % 2):
            b = int(rng.integers(0, frames // 2))
            loop = ((K.LOOP_FORWARD, K.LOOP_PINGPONG)[(i // 3) % 2], b, int(rng.integers(b + 1, frames + 1)))
        pitch = (0.5, 0.97, 1.0, 1.06, 2.0, "moving")[(i // 3) % 6] if shape == 2 else None
        pcm = wref.make_pcm(rng, frames, f"{fmt}_{'mono' if ch == 1 else 'stereo'}") if fmt in ("s16", "f32") else None
        out.append(PB(fmt, ch, frames, start, KINDS[i % 2], loop, pitch, pcm))
    return out


def test_mixed_list_bitwise(gas, monkeypatch):
    """Rows of the four formats side by side: k_sample_sources, k_sample_adpcm and k_sample_qoa each leave the others'
    rows alone."""
    K = gas.capi
    pbs = mixed_pbs(K)
    assert {(pb.fmt, pb.ch) for pb in pbs} == {(f, c) for f in ("qoa", "adpcm", "s16", "f32") for c in (1, 2)}
    assert {(pb.fmt, pb.loop is not None, pb.pitch is not None) for pb in pbs} >= {("qoa", a, b) for a in (False, True) for b in (False, True)}
    rigs = open_rigs(gas, monkeypatch, pbs, 512)
    try:
        run(K, rigs, pbs, zero_params(K, len(pbs)), callbacks=10)
        assert not rigs[-1][0].process_block_streams(rigs[-1][1])[2].all()  # some have ended, some go on
    finally:
        close_rigs(rigs)


def test_mixed_list_hrtf(gas, monkeypatch):
    """The same list with [HRTF] chains: the QOA context samples rows first; the twin holds compressed streams too here
    (the ADPCM ones), but the bands are those of the ADPCM test, whose twin may take the fused route: the mix is
    compared with helpers.mix_matches and the peaks within rtol 2e-5 / atol 1e-7."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    pbs = mixed_pbs(K)
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=8)
    params = synth.draw_params(np.random.default_rng(78), len(pbs), dirs=8)
    rigs = open_rigs(gas, monkeypatch, pbs, 512, chain=(K.FX_HRTF,), hrir=hrir)
    try:
        run(K, rigs, pbs, params, callbacks=10, compare=banded)
    finally:
        close_rigs(rigs)


def test_hrtf_list_against_fused_twin(gas, monkeypatch):
    """Plain QOA playbacks with [HRTF] chains and nothing else in the list: the QOA context samples rows first while the
    GAS_PCM_S16 twin takes the fused prologue; the same bands."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    pbs = [PB("qoa", 1 + i % 2, 3000 + 500 * i, 40 * i, KINDS[i % 2]) for i in range(12)]
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=8)
    params = synth.draw_params(np.random.default_rng(79), len(pbs), dirs=8)
    rigs = open_rigs(gas, monkeypatch, pbs, 512, chain=(K.FX_HRTF,), hrir=hrir)
    try:
        run(K, rigs, pbs, params, callbacks=8, compare=banded)
    finally:
        close_rigs(rigs)


def test_host_layer(gas):
    """A QOA device stream through the host layer's stream playbacks, against its GAS_PCM_S16 twin: the host layer
    needed no change."""
    K = gas.capi
    F, frames = 512, 1700
    file, dec = master("speech", 2)
    params = np.zeros(1, K.PARAMS_DTYPE)
    got = []
    for compressed in (True, False):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, ())
            sid = ctx.stream_create(qref.prefix(file, frames), K.PCM_QOA, 2, frames) if compressed else ctx.stream_create(np.ascontiguousarray(dec[:frames]))
            pid = host.start_playback_device_stream(sid, start_frame=30)
            host.set_spatializer_parameters(pid, params[0])
            rows = []
            for cb in range(6):
                rc, mix = host.get_mixed_frames(0, F)
                assert rc == 0
                rows.append((mix.copy(), host.is_playback_active(pid), host.get_playback_position(pid) if host.is_playback_active(pid) else -1))
            got.append(rows)
            host.close()
    for cb, (a, b) in enumerate(zip(*got)):
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], cb
    assert got[0][0][0].any()


def test_lifecycle_and_refusals(gas):
    K = gas.capi
    F = 512
    frames = 5400  # two QOA frames; two full callbacks from frame 33
    file, dec = master("random", 1)
    data = qref.prefix(file, frames)
    stereo = qref.prefix(master("random", 2)[0], frames)
    roomy = np.concatenate([data, np.zeros(2 * len(data), np.uint8)])  # enough bytes for any (channels, frames) below
    with gas.SpatializerContext(max_sources=1, frames=F) as ctx:
        refused = []
        refused += [(what, bad, 1, frames) for what, bad in qref.malformed(data, 1, frames).items()]
        refused += [(what + ", stereo", bad, 2, frames) for what, bad in qref.malformed(stereo, 2, frames).items()]
        refused += [("fewer frames than the header says", roomy, 1, frames - 1), ("a stereo file as mono", stereo, 1, frames), ("a mono file as stereo", roomy, 2, frames)]
        refused += [("channels 3", roomy, 3, frames), ("frames 0", roomy, 1, 0)]
        assert {r[0] for r in refused} >= {"magic", "samples", "channels", "fsamples", "fsize"}
        for what, bad, ch, n in refused:
            with pytest.raises(gas.GasError) as ei:
                ctx.stream_create(bad, K.PCM_QOA, ch, n)
            assert ei.value.status == -1, what  # GAS_ERR_INVALID_ARGUMENT
        with pytest.raises(gas.GasError) as ei:
            ctx.stream_create(roomy, 4, 1, frames)  # an unknown format
        assert ei.value.status == -1
        with pytest.raises(ValueError):
            ctx.stream_create(data[:-1], K.PCM_QOA, 1, frames)
        with pytest.raises(gas.GasError) as ei:
            ctx.stream_get_info(0)  # a refused create leaves no stream
        assert ei.value.status == -3  # GAS_ERR_BAD_SLOT
        sid = ctx.stream_create(data, K.PCM_QOA, 1, frames)
        assert sid == 0 and ctx.stream_get_info(sid) == (frames, 1, 3)
        slot = ctx.source_alloc(K.KIND_EFFECT)
        ctx.params_publish(slot, np.zeros(1, K.PARAMS_DTYPE))
        ctx.source_bind_stream(slot, sid)
        with pytest.raises(gas.GasError) as ei:
            ctx.stream_destroy(sid)  # still bound
        assert ei.value.status == -1
        want = wref.to_float_stereo(np.ascontiguousarray(dec[:frames]))
        mix, _, hf = ctx.process_block_streams([slot])
        assert hf[0] and not mix[0, :64].any() and np.array_equal(mix[0, 64:], want[: F - 64])
        # the slot rebound to a GAS_PCM_S16 stream and back to the QOA one plays each from its start
        pcm = wref.make_pcm(np.random.default_rng(9), 900, "s16_mono")
        plain = ctx.stream_create(pcm)
        for _ in range(2):
            ctx.source_bind_stream(slot, plain, start_frame=5)
            mix, _, hf = ctx.process_block_streams([slot])
            assert hf[0] and not mix[0, :64].any() and np.array_equal(mix[0, 64:], wref.to_float_stereo(pcm)[5:5 + F - 64])
            ctx.source_bind_stream(slot, sid, start_frame=33)
            mix, _, hf = ctx.process_block_streams([slot])
            assert hf[0] and not mix[0, :64].any() and np.array_equal(mix[0, 64:], want[33:33 + F - 64])
            mix, _, hf = ctx.process_block_streams([slot])
            assert hf[0] and np.array_equal(mix[0], want[33 + F - 64:33 + 2 * F - 64])
        ctx.stream_destroy(plain)
        ctx.source_free(slot)
        ctx.process_block_streams([])  # block boundary: the free takes effect
        ctx.stream_destroy(sid)
        with pytest.raises(gas.GasError) as ei:
            ctx.stream_get_info(sid)
        assert ei.value.status == -3
