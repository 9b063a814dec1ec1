"""tests/qoa_ref.py, the decoder the GPU tests of GAS_PCM_QOA compare with.  No independent QOA decoder can be had where
these tests run (no ffmpeg, no sox, no soundfile), so the decoder is pinned to two examples worked by hand from the
public specification, not taken from any code: PIN A, one slice from the state encoders start with, and PIN B, a
48-byte file whose header state makes predictions wrap and whose second slice is partial.  They are one person's
restatement of the specification, not a third-party implementation."""
import os

import numpy as np
import pytest

import qoa_ref as qref

SPEECH = os.path.join(os.path.dirname(__file__), "golden", "speech_excerpt_s16.npy")

PIN_A_SLICE = 0x50A6F59036FD3948  # sf 5, codes 0 2 4 6 7 5 3 1 0 0 6 6 7 7 2 3 4 5 1 0
PIN_A_SAMPLES = [104, 553, 1625, 3681, 4861, 5503, 5847, 6094, 6434, 6883, 8322, 10957, 13135, 14668, 16580, 18329, 20737, 22893, 24983, 27145]
PIN_A_WEIGHTS = [3, 3, -8189, 16387]
PIN_B_FILE = bytes.fromhex("716f61660000001b0100bb80001b002880007fffb1e079187fff800075307148fc7f0ea9b11d3b083547670000000000")
PIN_B_SAMPLES = [-32768, 32767, -32768, 32767, -32768, 32767, -32768, 32767, -32768, 32767, 32767, -32768, -32768, -32768, 14616, -32768, -32768, 32767, 32767, 32767, -12975, 32767, 32767, -32768, -32768, -32768, 13323]
PIN_B_WEIGHTS = [31025, -31246, 28796, 30146]


def test_pin_a():
    assert PIN_A_SLICE >> 60 == 5
    assert [(PIN_A_SLICE >> (57 - 3 * k)) & 7 for k in range(20)] == [0, 2, 4, 6, 7, 5, 3, 1, 0, 0, 6, 6, 7, 7, 2, 3, 4, 5, 1, 0]
    h, w = [0, 0, 0, 0], list(qref.INITIAL_WEIGHTS)
    got, wrapped = qref.decode_slice(h, w, PIN_A_SLICE)
    assert got == PIN_A_SAMPLES and w == PIN_A_WEIGHTS and h == PIN_A_SAMPLES[-4:] and wrapped == 0


def test_pin_b():
    assert len(PIN_B_FILE) == 48 == qref.file_bytes(27, 1)
    got = qref.decode_full(PIN_B_FILE)
    assert got["samples"][:, 0].tolist() == PIN_B_SAMPLES
    assert got["weights"] == [PIN_B_WEIGHTS]
    assert got["wrapped"] > 0
    assert np.array_equal(qref.decode(PIN_B_FILE, 1, 27), PIN_B_SAMPLES)


def test_dequantisation_table():
    assert qref.SCALE == [1, 7, 21, 45, 84, 138, 211, 304, 421, 562, 731, 928, 1157, 1419, 1715, 2048]
    assert qref.DEQ[0].tolist() == [1, -1, 3, -3, 5, -5, 7, -7]
    assert qref.DEQ[1].tolist() == [5, -5, 18, -18, 32, -32, 49, -49]
    assert qref.DEQ[15].tolist() == [1536, -1536, 5120, -5120, 9216, -9216, 14336, -14336]


def test_random_files_reach_rails_and_wrap():
    file = qref.random_file(np.random.default_rng(70), 3 * qref.FRAME, 1)
    got = qref.decode_full(file)
    assert got["samples"].min() == -32768 and got["samples"].max() == 32767
    assert got["wrapped"] > 0
    assert np.abs(got["records"][:, :, 4:]).max() > 32767  # inside a frame the weights outgrow int16
    assert np.abs(got["records"][:, :, 4:]).max() < 2**31 and np.abs(got["records"][:, :, :4]).max() <= 32768


@pytest.mark.parametrize("channels", [1, 2])
def test_state_does_not_cross_a_frame_edge(channels):
    """The second frame's header altered: only samples from 5120 on change.  A decoder that carries its state across the
    edge ignores the header, and is told from the right one by the unaltered file already."""
    n = qref.FRAME + 700
    file = qref.random_file(np.random.default_rng(71), n, channels)
    at = 8 + qref.frame_bytes(qref.FRAME, channels) + 8  # the second frame's state
    other = file.copy()
    other[at:at + 16 * channels] ^= 0x55
    a, b = qref.decode_full(file)["samples"], qref.decode_full(other)["samples"]
    assert np.array_equal(a[:qref.FRAME], b[:qref.FRAME])
    assert not np.array_equal(a[qref.FRAME:], b[qref.FRAME:])
    wrong_a, wrong_b = qref.decode_full(file, carry=True)["samples"], qref.decode_full(other, carry=True)["samples"]
    assert np.array_equal(wrong_a, wrong_b) and not np.array_equal(wrong_a, a)
    assert np.array_equal(wrong_a[:qref.FRAME], a[:qref.FRAME])


def test_speech_encoded():
    speech = (np.load(SPEECH).astype(np.int32) * 6).astype(np.int16)
    file = qref.encode(speech)
    assert file.dtype == np.uint8 and file.size == qref.file_bytes(len(speech), 1)
    got = qref.decode_full(file)
    dec = got["samples"][:, 0]
    assert dec.min() > -32768 and dec.max() < 32767 and got["wrapped"] == 0
    # the codec follows the signal (a loose bound, this is no quality test)
    err = dec.astype(np.float64) - speech
    assert np.sqrt(np.mean(err**2)) < 0.1 * np.sqrt(np.mean(speech.astype(np.float64) ** 2))


def test_encode_stereo_interleaves_slices():
    rng = np.random.default_rng(5)
    s = (8000 * np.sin(np.arange(150)[:, None] * [0.05, 0.11]) + rng.integers(-50, 50, (150, 2))).astype(np.int16)
    both = qref.decode(qref.encode(s), 2, 150)
    for c in range(2):
        assert np.array_equal(both[:, c], qref.decode(qref.encode(s[:, c]), 1, 150))


@pytest.mark.parametrize("n", [1, 19, 20, 21, 79, 80, 81, 5119, 5120, 5121, 11993])
def test_chunks_from_recorded_states(n):
    """Decoding every 80-frame chunk from its recorded state equals decoding straight through: what makes the format
    random-access.  The prefix of a file decodes to the prefix of its decode."""
    channels = 1 + n % 2
    master = qref.random_file(np.random.default_rng(72), 11993, channels)
    file = qref.prefix(master, n)
    assert file.size == qref.file_bytes(n, channels)
    straight = qref.decode_full(file)
    assert np.array_equal(straight["samples"], qref.decode_full(master)["samples"][:n])
    rec = straight["records"]
    assert rec.shape == ((n + qref.CHUNK - 1) // qref.CHUNK, channels, 8)
    _, frames = qref.parse(file)
    for c in range(channels):
        parts = []
        for k in range(len(rec)):
            h, w = rec[k, c, :4].tolist(), rec[k, c, 4:].tolist()
            slices = frames[k * qref.CHUNK // qref.FRAME][4]
            first = (k * qref.CHUNK % qref.FRAME) // qref.SLICE
            left = min(qref.CHUNK, n - k * qref.CHUNK)
            for j in range((left + qref.SLICE - 1) // qref.SLICE):
                parts += qref.decode_slice(h, w, slices[first + j][c], min(qref.SLICE, left - j * qref.SLICE))[0]
        assert parts == straight["samples"][:, c].tolist()


def test_malformed_list():
    file = qref.random_file(np.random.default_rng(73), 5200, 2)
    bad = qref.malformed(file, 2, 5200)
    assert sorted(bad) == ["channels", "fsamples", "fsize", "magic", "samples"]
    assert all(len(b) == len(file) and not np.array_equal(b, file) for b in bad.values())
