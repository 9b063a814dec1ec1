"""GAS_PCM_IMA_ADPCM streams (include/gas_amd.h): one context plays the compressed stream, a twin context plays
adpcm_ref.decode(...) of the same data as an ordinary GAS_PCM_S16 stream -- the contract is that the two behave alike in
every entry.  With empty chains and zero parameters the mix is the sum of the rows, so out, peaks (one per row),
has_frames and gas_stream_positions must be equal bit for bit after every callback.  test_adpcm_reference.py pins
adpcm_ref to audioop; test_gpu_stream_ends.py and test_gpu_stream_loops.py pin the GAS_PCM_S16 twin.

Every test packs its cases into one list, one playback per case.  A compressed case plays a prefix of one of four master
code sequences (random codes, which saturate at both rails, and the encoded speech excerpt; mono and stereo): the decode
of a prefix is the prefix of the decode, so each master is decoded once.

k_sample_adpcm.hip has two ways to a frame.  The span decode applies while a row's loads stay within 64 chunks (2048
frames); the cases that exceed it, so that the per-load decode runs by itself, are the L = 5000 loops with a seam in the
window and pitch 8 at F = 512 (448 fresh frames x 8).  test_forced_per_load runs a subset of every group under
GAS_ADPCM_SPAN=0 beside the default."""
import os
from dataclasses import dataclass

import numpy as np
import pytest

import adpcm_ref as aref
import stream_window_ref as wref
from helpers import mix_matches
from test_gpu_stream_loops import loop_cases

pytestmark = pytest.mark.gpu

SPEECH = os.path.join(os.path.dirname(__file__), "golden", "speech_excerpt_s16.npy")
MASTER_FRAMES = 9200
KINDS = ["random", "speech"]

_masters = {}


def master(kind, ch):
    """(codes, decoded int16) of MASTER_FRAMES frames, [frames] or [frames][2]; computed once and never written to."""
    if (kind, ch) not in _masters:
        if kind == "random":
            codes = np.random.default_rng(70 + ch).integers(0, 16, (MASTER_FRAMES, ch)).astype(np.uint8)
        else:
            s = (np.load(SPEECH)[:MASTER_FRAMES].astype(np.int32) * 6).astype(np.int16)  # peaks near 27000
            codes = aref.encode(np.stack([s, -np.roll(s, 777)][:ch], axis=1))
        dec = np.stack([aref.decode_channel(codes[:, k]) for k in range(ch)], axis=1)
        if ch == 1:
            codes, dec = codes[:, 0], dec[:, 0]
        codes.setflags(write=False)
        dec.setflags(write=False)
        _masters[(kind, ch)] = (codes, dec)
    return _masters[(kind, ch)]


@dataclass
class PB:
    """One playback: its stream (fmt adpcm: a prefix of master(kind, ch); s16 / f32: pcm, the same in both contexts),
    where it starts, its loop (mode, begin, end) and its pitch (None: not resampled; a number; "moving")."""

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
        if pb.fmt == "adpcm":
            codes, dec = master(pb.kind, pb.ch)
            if compressed:
                sid = ctx.stream_create(aref.pack(codes[: pb.frames]), K.PCM_IMA_ADPCM, pb.ch, pb.frames)
                assert ctx.stream_get_info(sid) == (pb.frames, pb.ch, K.PCM_IMA_ADPCM)
            else:
                sid = ctx.stream_create(np.ascontiguousarray(dec[: pb.frames]))
        else:
            sid = ctx.stream_create(pb.pcm)
        if pb.pitch is not None:
            ctx.stream_set_resampled(sid, True)
        if pb.loop is not None:
            ctx.stream_set_loop(sid, *pb.loop)
        ctx.source_bind_stream(slot, sid, start_frame=pb.start)
    return slots


def exact(got, want, where):
    for g, w, what in zip(got, want, ("out", "peaks", "has_frames", "positions")):
        assert np.array_equal(g, w), f"{what}, {where}"


def banded(got, want, where):
    """The twin may take another kernel form: helpers.mix_matches at the project's TOL, peaks as the other stream tests."""
    assert mix_matches(got[0][0], want[0][0]), f"out, {where}"
    np.testing.assert_allclose(got[1], want[1], rtol=2e-5, atol=1e-7, err_msg=where)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), where


def run(K, rigs, pbs, params, callbacks=None, past=2, limit=80, compare=exact):
    """rigs: (context, slots) pairs, the twin last.  Runs `callbacks` callbacks, or until `past` callbacks after the
    last playback that can end has ended.  Every context is compared with the twin after every callback."""
    n = len(pbs)
    moving = any(pb.pitch == "moving" for pb in pbs)
    can_end = np.array([pb.loop is None for pb in pbs])
    after, heard = 0, 0
    for cb in range(callbacks if callbacks is not None else limit):
        if cb == 0 or moving:
            p = params.copy()
            p["pitch_scale"] = [1.0 if pb.pitch is None else wref.moving_pitch(cb) if pb.pitch == "moving" else pb.pitch for pb in pbs]
            for ctx, slots in rigs:
                ctx.params_publish_batch(slots, p)
        res = [ctx.process_block_streams(slots) + (ctx.stream_positions(n),) for ctx, slots in rigs]
        for k, got in enumerate(res[:-1]):
            compare(got, res[-1], f"context {k}, callback {cb}")
        heard += bool(res[-1][0].any())
        if callbacks is None:
            after += not res[-1][2][can_end].any()
            if after > past:
                break
    else:
        assert callbacks is not None, "the playbacks never ended"
    assert heard >= 2
    return cb + 1


def open_rigs(gas, monkeypatch, pbs, F, forced=False, chain=(), hrir=None, flags=0):
    """Contexts and their slots: compressed (default paths) [, compressed with GAS_ADPCM_SPAN=0], the GAS_PCM_S16 twin."""
    K = gas.capi
    ctxs = [gas.SpatializerContext(max_sources=len(pbs), frames=F, flags=flags)]
    if forced:
        monkeypatch.setenv("GAS_ADPCM_SPAN", "0")  # read at context creation
        ctxs.append(gas.SpatializerContext(max_sources=len(pbs), frames=F, flags=flags))
        monkeypatch.delenv("GAS_ADPCM_SPAN")
    ctxs.append(gas.SpatializerContext(max_sources=len(pbs), frames=F, flags=flags))
    return [(ctx, setup(ctx, K, pbs, compressed=k < len(ctxs) - 1, chain=chain, hrir=hrir)) for k, ctx in enumerate(ctxs)]


def close_rigs(rigs):
    for ctx, _ in rigs:
        ctx.close()


def zero_params(K, n):
    return np.zeros(n, K.PARAMS_DTYPE)  # empty chain, zero params: every row is copied into the mix


# ---- the three groups of cases ----


def plain_pbs(F, ch, kind):
    """stream_window_ref.cases(F), and starts on either side of a chunk edge under lengths whose last chunk is whole
    (96, 2 F) and partial."""
    cases = wref.cases(F) + [(n, s) for n in (96, F + 1, 2 * F, 2 * F + 63, 3 * F + 200) for s in (31, 32, 33)]
    assert any(n % aref.CHUNK for n, _ in cases) and any(n % aref.CHUNK == 0 for n, _ in cases)
    return [PB("adpcm", ch, n, start, kind) for n, start in cases]


def loop_pbs(mode, ch):
    """loop_cases() of test_gpu_stream_loops.py (L = 1 .. 1500: a whole loop fits the span), and L = 5000 with a seam in
    the window of the first callbacks (the end of the loop; for ping-pong also the turn at the end of the period) and
    from frame 0, where the window bounds the span until the seam arrives."""
    out = []
    for i, (L, b, tail, start) in enumerate(loop_cases()):
        out.append(PB("adpcm", ch, b + L + tail, start, KINDS[i % 2], loop=(mode, b, 0 if tail == 0 else b + L)))
    b, L = 123, 5000
    for i, start in enumerate((b + L - 300, b + 2 * L - 300, b + L - 1500, 0)):
        out.append(PB("adpcm", ch, b + L + 200, start, KINDS[i % 2], loop=(mode, b, b + L)))
    return out


def resampled_pbs(F, K):
    """Every pitch of stream_window_ref.PITCHES and the moving one over short streams (the lengths and starts of
    test_gpu_stream_ends.py), one of 9000 frames for the pitches from 2 up (at 8 and F = 512 the taps of one callback
    span more than 2048 frames), and both loop modes."""
    out = []
    i = 0
    for pitch in wref.PITCHES + ["moving"]:
        fast = pitch == "moving" or pitch >= 2.0
        for ch in (1, 2):
            for n in (1, 2, 3, 4, 5, 64, F, 2 * F + 1) + ((9000,) if fast else ()):
                for start in sorted({0, max(n - 10, 0)}):
                    out.append(PB("adpcm", ch, n, start, KINDS[i % 2], pitch=pitch))
                    i += 1
            for mode in (K.LOOP_FORWARD, K.LOOP_PINGPONG):
                for L, b, tail, start in ((37, 0, 0, 0), (513, 123, 200, 123 + 513 + 50), (5000, 123, 200, 123 + 5000 - 700)):
                    out.append(PB("adpcm", ch, b + L + tail, start, KINDS[i % 2], loop=(mode, b, b + L), pitch=pitch))
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
        ran = run(gas.capi, rigs, pbs, zero_params(gas.capi, len(pbs)))
        assert ran >= (3 * F + 200) // F + 2
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
    """GAS_ADPCM_SPAN=0: every load decodes from its checkpoint.  The default context, the forced one and the twin give
    the same bits, so the two paths are held against each other and against the decoded stream."""
    K = gas.capi
    F = 512
    if group == "plain":
        pbs = plain_pbs(F, 1, "random")[::3] + plain_pbs(F, 2, "speech")[1::3]
    elif group == "loops":
        pbs = loop_pbs(K.LOOP_FORWARD, 2)[::3] + loop_pbs(K.LOOP_PINGPONG, 1)[1::3] + loop_pbs(K.LOOP_PINGPONG, 2)[-4:]
    else:
        pbs = resampled_pbs(F, K)[::3]
    rigs = open_rigs(gas, monkeypatch, pbs, F, forced=True)
    try:
        run(K, rigs, pbs, zero_params(K, len(pbs)), callbacks=6 if group == "loops" else None)
    finally:
        close_rigs(rigs)


def mixed_pbs(K):
    """70 playbacks: compressed, GAS_PCM_S16 and GAS_PCM_F32 streams, mono and stereo, plain, looped and resampled."""
    rng = np.random.default_rng(77)
    out = []
    for i in range(70):
        fmt = ("adpcm", "s16", "adpcm", "f32", "adpcm")[i % 5]
        ch = 1 + (i // 5) % 2
        shape = i % 3  # 0 plain, 1 looped, 2 resampled (every other one looped as well)
        frames = 300 + 97 * i if i % 4 else 5 * 512 + 60 * i
        start = int(rng.integers(0, 200))
        loop = None
        if shape == 1 or (shape == 2 and i % 2):
            b = int(rng.integers(0, frames // 2))
            loop = ((K.LOOP_FORWARD, K.LOOP_PINGPONG)[(i // 3) % 2], b, int(rng.integers(b + 1, frames + 1)))
        pitch = (0.5, 0.97, 1.0, 1.06, 2.0, "moving")[(i // 3) % 6] if shape == 2 else None
        pcm = None if fmt == "adpcm" else wref.make_pcm(rng, frames, f"{fmt}_{'mono' if ch == 1 else 'stereo'}")
        out.append(PB(fmt, ch, frames, start, KINDS[i % 2], loop, pitch, pcm))
    return out


def test_mixed_list_bitwise(gas, monkeypatch):
    """Rows of the three formats side by side: k_sample_sources and k_sample_adpcm each leave the other's rows alone."""
    K = gas.capi
    pbs = mixed_pbs(K)
    assert {(pb.fmt, pb.ch) for pb in pbs} == {(f, c) for f in ("adpcm", "s16", "f32") for c in (1, 2)}
    rigs = open_rigs(gas, monkeypatch, pbs, 512)
    try:
        run(K, rigs, pbs, zero_params(K, len(pbs)), callbacks=10)
        assert not rigs[-1][0].process_block_streams(rigs[-1][1])[2].all()  # some have ended, some go on
    finally:
        close_rigs(rigs)


def test_mixed_list_hrtf(gas, monkeypatch):
    """The same list with [HRTF] chains: the compressed context samples rows first; the twin may take the fused route,
    so the mix is compared with helpers.mix_matches and the peaks within rtol 2e-5 / atol 1e-7."""
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


def test_host_layer(gas):
    """A compressed device stream through the host layer's stream playbacks, against its GAS_PCM_S16 twin."""
    K = gas.capi
    F, frames = 512, 1700
    codes, dec = master("speech", 2)
    params = np.zeros(1, K.PARAMS_DTYPE)
    got = []
    for compressed in (True, False):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, ())
            sid = ctx.stream_create(aref.pack(codes[:frames]), K.PCM_IMA_ADPCM, 2, frames) if compressed else ctx.stream_create(np.ascontiguousarray(dec[:frames]))
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
    codes, dec = master("random", 1)
    frames = 1400  # two full callbacks from frame 33
    data = aref.pack(codes[:frames])
    with gas.SpatializerContext(max_sources=1, frames=F) as ctx:
        sid = ctx.stream_create(data, K.PCM_IMA_ADPCM, 1, frames)
        assert ctx.stream_get_info(sid) == (frames, 1, 2)
        for fmt, ch, n in ((K.PCM_IMA_ADPCM, 1, 0), (K.PCM_IMA_ADPCM, 3, 300), (3, 1, frames), (-1, 1, frames)):
            with pytest.raises(gas.GasError) as ei:
                ctx.stream_create(data, fmt, ch, n)
            assert ei.value.status == -1, (fmt, ch, n)  # GAS_ERR_INVALID_ARGUMENT
        slot = ctx.source_alloc(K.KIND_EFFECT)
        ctx.params_publish(slot, np.zeros(1, K.PARAMS_DTYPE))
        ctx.source_bind_stream(slot, sid)
        with pytest.raises(gas.GasError) as ei:
            ctx.stream_destroy(sid)  # still bound
        assert ei.value.status == -1
        want = wref.to_float_stereo(np.ascontiguousarray(dec[:frames]))
        mix, _, hf = ctx.process_block_streams([slot])
        assert hf[0] and not mix[0, :64].any() and np.array_equal(mix[0, 64:], want[: F - 64])
        # the slot rebound to a GAS_PCM_S16 stream and back to the compressed one plays each from its start
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
        assert ei.value.status == -3  # GAS_ERR_BAD_SLOT
