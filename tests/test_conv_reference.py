"""tests/conv_ref.py checked against numpy and by hand, without a GPU: the streaming reference is a plain convolution of
the whole sequence, and the float64 model of the device's partitions and ring computes the same thing."""
import numpy as np
import pytest

from conv_ref import ConvRef, PartitionModel, run_blocks


def whole(blocks, ir, dry, wet):
    """np.convolve over the concatenated blocks, cut back into blocks."""
    x = np.concatenate(blocks).astype(np.float64)
    h = np.atleast_2d(np.asarray(ir, dtype=np.float64))
    y = np.stack([dry * x[:, e] + wet * np.convolve(x[:, e], h[min(e, h.shape[0] - 1)])[: x.shape[0]] for e in range(2)], axis=1)
    return y.reshape(len(blocks), -1, 2)


def noise(rng, blocks, F):
    return [rng.uniform(-1, 1, (F, 2)) for _ in range(blocks)]


@pytest.mark.parametrize("channels", [1, 2])
def test_streaming_reference_is_np_convolve(channels):
    rng = np.random.default_rng(1)
    F = 128
    blocks = noise(rng, 7, F)
    ir = rng.standard_normal((channels, 2 * F + 5))
    got = run_blocks(ConvRef(ir, dry=0.25, wet=0.5), blocks)
    np.testing.assert_allclose(got, whole(blocks, ir, 0.25, 0.5), rtol=0, atol=1e-12)


@pytest.mark.parametrize("F", [128, 384])
def test_partition_model_equals_the_reference(F):
    rng = np.random.default_rng(2)
    blocks = noise(rng, 8, F)  # the ring of three partitions wraps twice
    for taps in (1, F - 1, F, F + 1, 3 * F - 1):
        ir = rng.standard_normal((2, taps)) / np.sqrt(taps)
        want = run_blocks(ConvRef(ir, 0.5, 0.75), blocks)
        got = run_blocks(PartitionModel(F, 3 * F - 1, ir, 0.5, 0.75), blocks)
        assert np.abs(got - want).max() <= 1e-12, (F, taps)
        np.testing.assert_allclose(want, whole(blocks, ir, 0.5, 0.75), rtol=0, atol=1e-12)


def test_partition_model_switches_and_resets_like_the_reference():
    rng = np.random.default_rng(3)
    F = 128
    blocks = noise(rng, 9, F)
    long_ir, short_ir = rng.standard_normal((2, 3 * F)) / 16, rng.standard_normal((1, 5))
    ref, mod = ConvRef(short_ir), PartitionModel(F, 3 * F, short_ir)
    for b, x in enumerate(blocks):
        if b == 3:  # the longer IR reaches into history the shorter one never used
            ref.set_ir(long_ir), mod.set_ir(long_ir)
        if b == 5:
            ref.set_levels(0.5, 2.0), mod.set_levels(0.5, 2.0)
        if b == 6:
            ref.set_ir(short_ir), mod.set_ir(short_ir)
        if b == 7:
            ref.reset(), mod.reset()
        assert np.abs(mod.process(x) - ref.process(x)).max() <= 1e-12, b


@pytest.mark.parametrize("make", [lambda ir: ConvRef(ir), lambda ir: PartitionModel(128, 256, ir)])
def test_hand_worked_cases(make):
    F = 128
    x = [np.arange(b * F, (b + 1) * F, dtype=np.float64)[:, None] * np.array([1.0, -2.0]) + 1.0 for b in range(3)]
    flat = np.concatenate(x)
    # a delta IR hands the input through
    np.testing.assert_allclose(run_blocks(make([1.0]), x), np.stack(x), atol=1e-9)
    # a one-tap delay: y[t] = x[t - 1], zero at t = 0, the last frame of a block arriving first in the next
    y = run_blocks(make([0.0, 1.0]), x).reshape(-1, 2)
    np.testing.assert_allclose(y[0], 0.0, atol=1e-9)
    np.testing.assert_allclose(y[1:], flat[:-1], atol=1e-9)
    np.testing.assert_allclose(y[F], x[0][F - 1], atol=1e-9)
    # hard switch from the delay to a delta between blocks 1 and 2: block 2 comes through undelayed, from its first frame
    m = make([0.0, 1.0])
    m.process(x[0])
    np.testing.assert_allclose(m.process(x[1]), flat[F - 1 : 2 * F - 1], atol=1e-9)
    m.set_ir([1.0])
    np.testing.assert_allclose(m.process(x[2]), x[2], atol=1e-9)
