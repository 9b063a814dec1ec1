"""tests/stream_window_ref.py against the oracle's mixer (gaso_fetch_source through gaso_get_mixed_frames): one playback,
KIND_EFFECT with an empty chain, so the mix is 0 + row.  Rows bit for bit, has_frames and the position equal, over the
whole case table, every playback run until two callbacks past its end.

The oracle has no start frame: a playback started at `start` is the oracle's playback over S[start:], whose position
counts from there.  Frames in front of the start read as zero in both (the oracle's stream_at(j < 0), the zeroed
lookahead)."""
import numpy as np
import pytest

import stream_window_ref as wref
from test_oracle_mixer import Rig

PITCHES, moving_pitch = wref.PITCHES, wref.moving_pitch


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_against_oracle(ob, pcm, start, F, resampled=False, pitch=1.0, where=""):
    pb = wref.Playback(pcm, start, resampled=resampled)
    rig = Rig(ob, ob.KIND_EFFECT, [pb.S[pb.start:]], F)
    rig.pbs[0].resampled = int(resampled)
    for cb, row in wref.run_to_end(pb, F, pitch):
        rig.params["pitch_scale"] = pitch(cb) if callable(pitch) else pitch
        rc, want = rig.get_mixed_frames(0)
        assert rc == 0
        at = f"{where} callback {cb}"
        assert np.array_equal(bits(np.zeros_like(row) + row), bits(want)), at
        assert pb.has_frames == bool(rig.pbs[0].has_frames), at
        opos = (rig.pbs[0].mix_offset >> 16) if resampled else rig.pbs[0].stream_pos
        assert pb.position == pb.start + opos, at
    assert not pb.has_frames and not row.any()
    return cb + 1


def test_fade_table():
    k = np.arange(64)
    np.testing.assert_allclose(wref.ENV, 0.96 ** (k + 1) * (64 - k) / 64, rtol=1e-5)
    assert wref.ENV.dtype == np.float32 and np.all(np.diff(wref.ENV) < 0)


def test_increment():
    assert [wref.increment(p) for p in (0.0, 0.125, 0.5, 1.0, 2.0, 8.0)] == [0, 8192, 32768, 65536, 131072, 524288]
    assert wref.increment(0.97) == int((float(np.float32(48000.0) * np.float32(0.97)) / 48000.0) * 65536.0)


def test_case_table():
    for F in (128, 256, 384, 512):
        c = wref.cases(F)
        assert len(c) == len(set(c)) and all(n >= 1 and s >= 0 for n, s in c)
        assert {n for n, _ in c} == set(wref.lengths(F)) and len(wref.lengths(F)) == (14 if F == 128 else 16)
        for n in wref.lengths(F):
            assert {s for m, s in c if m == n} >= {s for s in (0, n - 1, n, n + 5)}


@pytest.mark.parametrize("F", [128, 256, 384, 512])
@pytest.mark.parametrize("fmt", wref.FORMATS)
def test_plain_window_matches_oracle(ob, fmt, F):
    rng = np.random.default_rng(31)
    for n, start in wref.cases(F):
        pcm = wref.make_pcm(rng, n, fmt)
        cbs = check_against_oracle(ob, pcm, start, F, where=f"len {n} start {start}")
        assert cbs == max(n - start, 0) // F + 3  # the callback it ends in, and two more


@pytest.mark.parametrize("F", [128, 512])
@pytest.mark.parametrize("pitch", PITCHES + ["moving"])
def test_resampled_window_matches_oracle(ob, pitch, F):
    rng = np.random.default_rng(32)
    p = moving_pitch if pitch == "moving" else pitch
    for fmt in ("s16_mono", "f32_stereo"):
        for n, start in wref.cases(F):
            pcm = wref.make_pcm(rng, n, fmt)
            check_against_oracle(ob, pcm, start, F, resampled=True, pitch=p, where=f"{fmt} len {n} start {start}")


def test_pitch_zero_holds(ob):
    """Increment 0: the playback never ends and the position holds."""
    F = 128
    pcm = wref.make_pcm(np.random.default_rng(33), 300, "s16_stereo")
    pb = wref.Playback(pcm, 17, resampled=True)
    rig = Rig(ob, ob.KIND_EFFECT, [pb.S[17:]], F)
    rig.pbs[0].resampled = 1
    for cb, pitch in enumerate((1.0, 0.0, 0.0, 0.0)):  # one block in motion first, so that what is held is not silence
        rig.params["pitch_scale"] = pitch
        row = pb.block(F, pitch)
        rc, want = rig.get_mixed_frames(0)
        assert rc == 0 and np.array_equal(bits(np.zeros_like(row) + row), bits(want)), cb
        assert pb.has_frames and rig.pbs[0].has_frames and pb.position == 17 + F and rig.pbs[0].mix_offset == F << 16
    assert row.any() and np.all(row == row[0])  # the lookahead regenerated at increment 0 too
