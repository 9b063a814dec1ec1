"""tests/adpcm_ref.py, the decoder the GPU tests of GAS_PCM_IMA_ADPCM compare with, against Python's audioop.adpcm2lin:
an independent implementation of the IMA/DVI standard.  One adaptation: audioop puts the first sample of a byte in the
high nibble, the engine's data in the low one (swap_nibbles).  PIN_CODES / PIN_SAMPLES were generated once from audioop,
so the decoder stays pinned on a Python without that module."""
import os

import numpy as np
import pytest

import adpcm_ref as aref

SPEECH = os.path.join(os.path.dirname(__file__), "golden", "speech_excerpt_s16.npy")

PIN_CODES = [3, 10, 1, 3, 5, 4, 14, 12, 14, 15, 1, 2, 13, 1, 2, 2, 14, 5, 4, 2, 7, 9, 12, 9, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 0, 0, 0, 0, 0, 0, 15, 1, 7, 9, 11, 0, 3, 7, 1, 15, 10, 12]
PIN_SAMPLES = [4, 1, 2, 6, 14, 26, 6, -19, -64, -157, -118, -58, -179, -131, -58, 8, -149, 88, 372, 563, 1084, 861, 249, 3, 1123, 3526, 8679, 19729, 32767, 32767, 32767, 32767, 32767, 32767, 32767, 32767, -28669, -32768, -32768, -32768, -32768, -32768, -32768, -32768, -32768, -32768, -28673, -24949, -21564, -18487, -15689, -13146, -32768, -20482, 32767, 20481, -5588, -2203, 19340, 32767, 32767, -23096, -32768, -32768]


def audioop_decode(codes):
    """One channel's codes through audioop.adpcm2lin (16-bit output, initial state None = (0, 0))."""
    audioop = pytest.importorskip("audioop")
    out, _ = audioop.adpcm2lin(aref.swap_nibbles(aref.pack(codes)).tobytes(), 2, None)
    return np.frombuffer(out, np.int16)[: len(codes)]


def test_inline_pin():
    assert np.array_equal(aref.decode_channel(PIN_CODES), PIN_SAMPLES)
    assert np.array_equal(aref.decode(aref.pack(PIN_CODES), 1, len(PIN_CODES)), PIN_SAMPLES)


def test_inline_pin_is_audioops():
    assert np.array_equal(audioop_decode(np.array(PIN_CODES, np.uint8)), PIN_SAMPLES)


def test_random_codes_reach_rails_and_clamps():
    codes = np.random.default_rng(1).integers(0, 16, 6000).astype(np.uint8)
    got, states = aref.decode_channel(codes, want_states=True)
    assert got.min() == -32768 and got.max() == 32767
    assert states[:, 1].min() == 0 and states[:, 1].max() == 88
    assert np.array_equal(got, audioop_decode(codes))


def test_speech_encoded():
    speech = np.load(SPEECH)
    codes = aref.encode(speech)
    assert codes.shape == speech.shape and codes.max() <= 15
    got = aref.decode_channel(codes)
    assert np.array_equal(got, audioop_decode(codes))
    # the codec follows the signal (4 bits per sample: a loose bound, this is no quality test)
    err = got.astype(np.float64) - speech
    assert np.sqrt(np.mean(err**2)) < 0.1 * np.sqrt(np.mean(speech.astype(np.float64) ** 2))


@pytest.mark.parametrize("frames", [1, 2, 31, 32, 33, 63, 65, 1001])
@pytest.mark.parametrize("channels", [1, 2])
def test_packing_odd_counts_and_stereo(channels, frames):
    rng = np.random.default_rng(100 * channels + frames)
    codes = rng.integers(0, 16, (frames, channels)).astype(np.uint8)
    codes = codes[:, 0] if channels == 1 else codes
    data = aref.pack(codes)
    assert data.dtype == np.uint8 and data.size == ((frames + 1) // 2) * channels
    for i in (0, frames // 2, frames - 1):  # the layout as include/gas_amd.h states it
        for c in range(channels):
            n = (data[(i >> 1) * channels + c] >> (4 * (i & 1))) & 15
            assert n == (codes[i] if channels == 1 else codes[i, c])
    assert np.array_equal(aref.unpack(data, channels, frames), codes)
    got = aref.decode(data, channels, frames)
    assert got.shape == codes.shape and got.dtype == np.int16
    for c in range(channels):
        col = codes if channels == 1 else codes[:, c]
        assert np.array_equal(got if channels == 1 else got[:, c], audioop_decode(col))


@pytest.mark.parametrize("frames", [1, 32, 33, 100, 2049])
def test_chunks_from_recorded_states(frames):
    """Decoding every chunk from its checkpoint equals decoding straight through: what makes the format random-access."""
    codes = np.random.default_rng(frames).integers(0, 16, frames).astype(np.uint8)
    straight = aref.decode_channel(codes)
    ck = aref.checkpoints(codes)
    assert ck.shape == ((frames + aref.CHUNK - 1) // aref.CHUNK, 2) and tuple(ck[0]) == (0, 0)
    assert np.abs(ck[:, 0]).max() <= 32768 and ck[:, 1].max() <= 88  # fits int16 / uint8 records
    parts = [aref.decode_channel(codes[k * aref.CHUNK:(k + 1) * aref.CHUNK], state=ck[k]) for k in range(len(ck))]
    assert np.array_equal(np.concatenate(parts), straight)
