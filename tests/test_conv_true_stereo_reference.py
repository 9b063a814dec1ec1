"""tests/conv_ts_ref.py checked by hand, against np.convolve and against conv_ref, without a GPU: the true-stereo rule of
include/gas_amd.h (channel c = 2 i + e from input ear i to output ear e), its partition model, the whole-signal FFT
form that stands in for the direct form in one long GPU case, and fades between states of different channel counts."""
import numpy as np
import pytest

from conv_fade_ref import fade_s
from conv_ref import ConvRef, run_blocks
from conv_ts_ref import TrueStereoFadeRef, TrueStereoPartitionModel, TrueStereoRef, whole_signal

F = 128


def noise(rng, blocks, frames=F):
    return [rng.uniform(-1, 1, (frames, 2)) for _ in range(blocks)]


@pytest.mark.parametrize("dry,wet", [(0.0, 1.0), (0.25, 0.75)])
def test_streaming_reference_is_np_convolve_per_pair_of_ears(dry, wet):
    rng = np.random.default_rng(1)
    ir = rng.standard_normal((4, 2 * F + 5))
    blocks = noise(rng, 5)
    x = np.concatenate(blocks)
    got = run_blocks(TrueStereoRef(ir, dry, wet), blocks).reshape(-1, 2)
    for e in range(2):
        want = dry * x[:, e] + wet * sum(np.convolve(x[:, i], ir[2 * i + e])[: x.shape[0]] for i in range(2))
        np.testing.assert_allclose(got[:, e], want, rtol=0, atol=1e-11)


@pytest.mark.parametrize("c", range(4))
def test_a_unit_tap_in_one_channel_routes_one_ear_to_one_ear(c):
    rng = np.random.default_rng(2)
    ir = np.zeros((4, 3))
    ir[c, 0] = 1.0
    blocks = noise(rng, 3)
    y = run_blocks(TrueStereoRef(ir), blocks)
    x = np.stack(blocks)
    np.testing.assert_array_equal(y[:, :, c & 1], x[:, :, c >> 1])
    assert not y[:, :, 1 - (c & 1)].any()


def test_delayed_cross_feed_by_hand():
    """LR = a unit tap at 2: the right ear hears the left input two frames late, the left ear nothing."""
    ir = np.zeros((4, 3))
    ir[1, 2] = 1.0
    x = np.zeros((F, 2))
    x[0] = (1.0, 5.0)
    y = TrueStereoRef(ir).process(x)
    want = np.zeros((F, 2))
    want[2, 1] = 1.0
    np.testing.assert_array_equal(y, want)


@pytest.mark.parametrize("channels", [1, 2])
def test_diagonal_four_channels_equal_conv_ref_exactly(channels):
    rng = np.random.default_rng(3)
    h = rng.standard_normal((channels, F + 7))
    four = np.stack([h[0], np.zeros(F + 7), np.zeros(F + 7), h[-1]])
    blocks = noise(rng, 4)
    want = run_blocks(ConvRef(h, 0.5, 0.75), blocks)
    np.testing.assert_array_equal(run_blocks(TrueStereoRef(four, 0.5, 0.75), blocks), want)
    np.testing.assert_array_equal(run_blocks(TrueStereoRef(h, 0.5, 0.75), blocks), want)  # one and two channels pass through


@pytest.mark.parametrize("k_ir", [1, 11, 18])
def test_partition_model_equals_the_direct_form_across_a_ring_wrap(k_ir):
    """F = 128, a ring of K = 18 spectra per input ear, 40 blocks: the ring wraps twice."""
    rng = np.random.default_rng(10 + k_ir)
    taps = 5 if k_ir == 1 else k_ir * F - 7
    ir = rng.standard_normal((4, taps)) / 16
    blocks = noise(rng, 40)
    mod = TrueStereoPartitionModel(F, 18 * F, ir, 0.25, 0.75)
    assert mod.K == 18 and mod.k_ir == k_ir
    ref = TrueStereoRef(ir, 0.25, 0.75)
    for b, x in enumerate(blocks):
        assert np.abs(mod.process(x) - ref.process(x)).max() <= 1e-12, b


def test_partition_model_hard_switch_keeps_the_history():
    rng = np.random.default_rng(4)
    two, four = rng.standard_normal((2, 3 * F)) / 16, rng.standard_normal((4, 2 * F + 1)) / 16
    mod, ref = TrueStereoPartitionModel(F, 3 * F, two), TrueStereoRef(two)
    for b, x in enumerate(noise(rng, 9)):
        if b in (3, 6):
            mod.set_ir(four if b == 3 else two), ref.set_ir(four if b == 3 else two)
        assert np.abs(mod.process(x) - ref.process(x)).max() <= 1e-12, b


@pytest.mark.parametrize("channels", [1, 2, 4])
def test_whole_signal_fft_equals_the_direct_form(channels):
    rng = np.random.default_rng(5)
    ir = rng.standard_normal((channels, 5 * F - 9)) / 16
    blocks = noise(rng, 9)
    want = run_blocks(TrueStereoRef(ir, 0.25, 0.75), blocks).reshape(-1, 2)
    assert np.abs(whole_signal(ir, np.concatenate(blocks), 0.25, 0.75) - want).max() <= 1e-12


def test_fade_from_mono_to_four_channels_is_the_lerp_written_out():
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((1, 5)), rng.standard_normal((4, 2 * F + 3)) / 16
    blocks = noise(rng, 7)
    r, ra, rb = TrueStereoFadeRef(F, a, 0.5, 0.5), ConvRef(a, 0.5, 0.5), TrueStereoRef(b, 0.25, 1.0)
    for i, x in enumerate(blocks):
        if i == 2:
            r.fade_to(b, 0.25, 1.0, 3)
            assert r.fade_remaining() == 3 and len(r.named()) == 2
        ya, yb = ra.process(x), rb.process(x)
        if i < 2:
            want = ya
        elif i < 5:
            s = fade_s(F, 3, i - 2)[:, None]
            want = (1.0 - s) * ya + s * yb
        else:
            want = yb
        assert np.abs(r.process(x) - want).max() <= 1e-12, i
    assert r.fade_remaining() == 0
    np.testing.assert_array_equal(r.process(blocks[0]), rb.process(blocks[0]))  # state B exactly, over the one history


def test_fade_state_machine_with_four_channel_states():
    """A pending four-channel target, a hard switch (fade_blocks = 0) and a reset mid-fade, as conv_fade_ref has them."""
    rng = np.random.default_rng(7)
    a, b, c = rng.standard_normal((4, 9)) / 4, rng.standard_normal((2, F + 5)) / 8, rng.standard_normal((4, 2 * F)) / 8
    blocks = noise(rng, 8)
    r = TrueStereoFadeRef(F, a)
    ra, rb, rc = TrueStereoRef(a), TrueStereoRef(b, 0.5, 0.5), TrueStereoRef(c, 0.0, 2.0)
    r.fade_to(b, 0.5, 0.5, 2)
    r.fade_to(c, 0.0, 2.0, 3)  # pending
    assert r.fade_remaining() == 5 and len(r.named()) == 3
    for i, x in enumerate(blocks):
        ya, yb, yc = ra.process(x), rb.process(x), rc.process(x)
        if i < 2:
            s = fade_s(F, 2, i)[:, None]
            want = (1 - s) * ya + s * yb
        elif i < 5:
            s = fade_s(F, 3, i - 2)[:, None]
            want = (1 - s) * yb + s * yc
        else:
            want = yc
        assert np.abs(r.process(x) - want).max() <= 1e-12, i
    r.fade_to(a, 0.0, 1.0, 0)
    np.testing.assert_array_equal(r.process(blocks[0]), ra.process(blocks[0]))
    r.fade_to(c, 0.25, 1.0, 4)
    r.process(blocks[1])
    r.reset()
    assert r.fade_remaining() == 0
    np.testing.assert_array_equal(r.process(blocks[2]), TrueStereoRef(c, 0.25, 1.0).process(blocks[2]))
