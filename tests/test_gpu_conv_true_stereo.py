"""Four-channel ("true stereo") impulse responses on the GPU against tests/conv_ts_ref.py's float64 references.

Tolerance: helpers.TOL (1e-5 relative RMS), the convolvers' band, here per block of an instance; bitwise where a test
says so.  Every comparison prints its figure and the worst seen so far before it asserts."""
import numpy as np
import pytest

from conv_ts_ref import TrueStereoFadeRef, TrueStereoRef, whole_signal
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

WORST = [0.0]


def noise(rng, blocks, n, F):
    return [rng.uniform(-1, 1, (n, F, 2)).astype(np.float32) for _ in range(blocks)]


def decaying(rng, channels, taps):
    return (rng.standard_normal((channels, taps)) * np.exp(-4.0 * np.arange(taps) / taps)).astype(np.float32)


def diagonal(h):
    """[h_L, h_R] or [h] -> the four-channel IR without cross-feed, [h_L, 0, 0, h_R]."""
    z = np.zeros_like(h[0])
    return np.stack([h[0], z, z, h[-1]])


def close(name, got, want):
    """got, want [blocks][F][2]: every block within the bar."""
    errs = [rel_rms(g, w) for g, w in zip(got, want)]
    WORST[0] = max(WORST[0], max(errs))
    print(f"{name}: worst block rel rms {max(errs):.3g} (worst so far in this file {WORST[0]:.3g})")
    assert max(errs) <= TOL, (name, int(np.argmax(errs)), max(errs))


def status(call, *a):
    with pytest.raises(Exception) as ei:
        call(*a)
    return ei.value.status


@pytest.mark.parametrize("c", range(4))
def test_routing(gas, c):
    F = 128
    rng = np.random.default_rng(40 + c)
    ir = np.zeros((4, 1), np.float32)
    ir[c, 0] = 1.0
    blocks = noise(rng, 3, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, F)
        conv = ctx.conv_create(ctx.conv_ir_load(ir))
        y = np.stack([ctx.conv_process([conv], x)[0] for x in blocks])
    x = np.stack([b[0] for b in blocks])
    close(f"routing channel {c}", y[:, :, c & 1][..., None], x[:, :, c >> 1][..., None])
    assert not y[:, :, 1 - (c & 1)].any()  # exactly zero


@pytest.mark.parametrize("channels", [2, 1])
@pytest.mark.parametrize("one_call", [True, False])
def test_diagonal_is_bitwise_the_narrower_ir(gas, channels, one_call):
    """[h_L, 0, 0, h_R] against the two-channel [h_L, h_R], and [h, 0, 0, h] against the one-channel h: 18 partitions,
    two chunks, the second a tail only."""
    F = 128
    rng = np.random.default_rng(50 + channels)
    h = decaying(rng, channels, 17 * F + 3)
    blocks = noise(rng, 24, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 17 * F + 3)
        wide, narrow = ctx.conv_create(ctx.conv_ir_load(diagonal(h))), ctx.conv_create(ctx.conv_ir_load(h))
        for x in blocks:
            if one_call:
                o = ctx.conv_process([wide, narrow], np.concatenate([x, x]))
            else:
                o = np.concatenate([ctx.conv_process([wide], x), ctx.conv_process([narrow], x)])
            assert np.array_equal(o[0], o[1])
            assert o.any()


def test_against_the_reference_across_a_ring_wrap(gas):
    """F = 128, a reservation of 18 F: one, eleven and eighteen partitions in one call, 40 blocks."""
    F = 128
    rng = np.random.default_rng(60)
    irs = [decaying(rng, 4, t) for t in (5, 11 * F - 7, 17 * F + 3)]
    blocks = noise(rng, 40, len(irs), F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(len(irs), 18 * F)
        convs = [ctx.conv_create(ctx.conv_ir_load(h)) for h in irs]
        ctx.conv_set_levels(convs[1], 0.25, 0.75)
        outs = [ctx.conv_process(convs, x) for x in blocks]
    for i, h in enumerate(irs):
        ref = TrueStereoRef(h, 0.25, 0.75) if i == 1 else TrueStereoRef(h)
        close(f"ring wrap taps {h.shape[1]}", [o[i] for o in outs], [ref.process(x[i]) for x in blocks])


@pytest.mark.parametrize("F", [384, 512])
def test_against_the_reference_at_larger_blocks(gas, F):
    rng = np.random.default_rng(F)
    h = decaying(rng, 4, 2 * F + 5)
    blocks = noise(rng, 6, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, 3 * F)
        conv = ctx.conv_create(ctx.conv_ir_load(h))
        outs = [ctx.conv_process([conv], x)[0] for x in blocks]
    ref = TrueStereoRef(h)
    close(f"F {F}", outs, [ref.process(x[0]) for x in blocks])


def test_many_uneven_chunks(gas):
    """520 partitions: chunk length 17, 31 chunks, the last of 10.  524 calls; the last four blocks, which hear the whole
    IR, against the float64 FFT of the whole signal (pinned to the direct form by the CPU tests)."""
    F, calls = 128, 524
    taps = 520 * F - 9
    rng = np.random.default_rng(70)
    h = decaying(rng, 4, taps)
    x = rng.uniform(-1, 1, (calls, 1, F, 2)).astype(np.float32)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, taps)
        assert ctx.conv_ir_get_info(ctx.conv_ir_load(h)) == (4, taps)
        conv = ctx.conv_create(0)
        tail = [ctx.conv_process([conv], b)[0] for b in x][-4:]
    want = whole_signal(h, x.reshape(-1, 2)).reshape(calls, F, 2)[-4:]
    close("31 chunks", tail, want)


def test_24_instances_of_one_two_and_four_channels(gas):
    """Eight instances each of one, two and four channels, every channel count with every length.  One call naming all
    is bitwise 24 calls of one instance, and a second run gives the same bits."""
    F, n = 128, 24
    rng = np.random.default_rng(80)
    irs = [decaying(rng, (1, 2, 4)[i % 3], (5, F + 1, 17 * F + 3)[(i // 3) % 3]) for i in range(n)]
    blocks = noise(rng, 6, n, F)
    outs = []
    for one_per_call in (False, False, True):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_conv(n, 17 * F + 3)
            convs = [ctx.conv_create(ctx.conv_ir_load(h)) for h in irs]
            if one_per_call:
                outs.append(np.stack([np.concatenate([ctx.conv_process([k], x[i : i + 1]) for i, k in enumerate(convs)]) for x in blocks]))
            else:
                outs.append(np.stack([ctx.conv_process(convs, x) for x in blocks]))
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], outs[2])
    for i, h in enumerate(irs):
        ref = TrueStereoRef(h)
        close(f"24 instances[{i}] {h.shape}", outs[0][:, i], [ref.process(x[i]) for x in blocks])


def test_hard_switch_keeps_the_history(gas):
    F = 128
    rng = np.random.default_rng(90)
    two, four = decaying(rng, 2, 3 * F), decaying(rng, 4, 2 * F + 1)
    blocks = noise(rng, 9, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, 3 * F)
        ids = {2: ctx.conv_ir_load(two), 4: ctx.conv_ir_load(four)}
        conv = ctx.conv_create(ids[2])
        ref = TrueStereoRef(two)
        got, want = [], []
        for b, x in enumerate(blocks):
            if b in (3, 6):
                ctx.conv_set_ir(conv, ids[4 if b == 3 else 2]), ref.set_ir(four if b == 3 else two)
            got.append(ctx.conv_process([conv], x)[0])
            want.append(ref.process(x[0]))
    close("two -> four -> two channels", got, want)


class Rig:
    """One instance and its TrueStereoFadeRef, given the same calls.  irs: name -> (array, id in the context)."""

    def __init__(self, ctx, irs, F, name, dry=0.0, wet=1.0):
        self.ctx, self.irs = ctx, irs
        self.conv = ctx.conv_create(irs[name][1])
        ctx.conv_set_levels(self.conv, dry, wet)
        self.ref = TrueStereoFadeRef(F, irs[name][0], dry, wet)

    def fade_to(self, name, dry, wet, n):
        self.ctx.conv_fade_to(self.conv, self.irs[name][1], dry, wet, n)
        self.ref.fade_to(self.irs[name][0], dry, wet, n)

    def remaining(self):
        got = self.ctx.conv_fade_remaining(self.conv)
        assert got == self.ref.fade_remaining()
        return got

    def process(self, x):
        return self.ctx.conv_process([self.conv], x)[0], self.ref.process(x[0])


FADE_PAIRS = {"mono to four": ((1, 5), (4, 17 * 128 + 3)), "four to two": ((4, 17 * 128 + 3), (2, 128 + 9)), "four to four": ((4, 128 + 9), (4, 11 * 128 - 7))}


@pytest.mark.parametrize("pair", sorted(FADE_PAIRS))
def test_fades_between_channel_counts(gas, pair):
    """A -> B over N = 3 calls: every block against the fade reference; from call N + 1 on bitwise a hard switch to B."""
    F, N = 128, 3
    (ch_a, taps_a), (ch_b, taps_b) = FADE_PAIRS[pair]
    rng = np.random.default_rng(100 + len(pair) + taps_a)
    a, b = decaying(rng, ch_a, taps_a), decaying(rng, ch_b, taps_b)
    blocks = noise(rng, 8, 1, F)
    outs = []
    for n in (N, 0):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_conv(1, 17 * F + 3)
            irs = {"a": (a, ctx.conv_ir_load(a)), "b": (b, ctx.conv_ir_load(b))}
            r = Rig(ctx, irs, F, "a", 0.5, 0.5)
            got, want = [], []
            for i, x in enumerate(blocks):
                if i == 2:
                    r.fade_to("b", 0.25, 1.0, n)
                    if n:
                        assert status(ctx.conv_ir_free, irs["a"][1]) == -1 and status(ctx.conv_ir_free, irs["b"][1]) == -1
                assert r.remaining() == (max(0, 2 + n - i) if i >= 2 else 0)
                g, w = r.process(x)
                got.append(g), want.append(w)
            close(f"{pair}, over {n}", got, want)
            assert r.remaining() == 0
            ctx.conv_ir_free(irs["a"][1])  # the instance is in state B
            assert status(ctx.conv_ir_free, irs["b"][1]) == -1
            outs.append(np.stack(got))
    faded, hard = outs
    assert np.array_equal(faded[:2], hard[:2])
    assert np.array_equal(faded[2 + N :], hard[2 + N :])
    assert not np.array_equal(faded[3], hard[3])


def test_level_only_fade_and_a_pending_four_channel_target(gas):
    F = 128
    rng = np.random.default_rng(110)
    blocks = noise(rng, 13, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 3 * F)
        arrays = {"a": decaying(rng, 4, 2 * F + 3), "b": decaying(rng, 2, F + 5), "c": decaying(rng, 4, 3 * F)}
        irs = {k: (h, ctx.conv_ir_load(h)) for k, h in arrays.items()}
        ida, idb, idc = (irs[k][1] for k in "abc")
        r = Rig(ctx, irs, F, "a", 0.75, -0.5)
        got, want, seen = [], [], []
        for i, x in enumerate(blocks):
            if i == 1:  # level only: one wet sum over the four-channel IR serves both states
                r.fade_to("a", 0.0, 1.0, 3)
                assert status(ctx.conv_ir_free, ida) == -1
            if i == 5:
                r.fade_to("b", 0.5, 0.5, 3)
            if i == 6:  # a pending four-channel target: A, B and pending are all named
                r.fade_to("c", 0.25, 1.0, 2)
                assert [status(ctx.conv_ir_free, k) for k in (ida, idb, idc)] == [-1, -1, -1]
            if i == 8:  # the fade to b has made its last call: a is free to go, b is the state, c the target
                ctx.conv_ir_free(ida)
                assert [status(ctx.conv_ir_free, k) for k in (idb, idc)] == [-1, -1]
            seen.append(r.remaining())
            g, w = r.process(x)
            got.append(g), want.append(w)
        close("level only, then a pending target", got, want)
        assert seen == [0, 3, 2, 1, 0, 3, 2 + 2, 1 + 2, 2, 1, 0, 0, 0]
        ctx.conv_ir_free(idb)  # fade_remaining is 0: only c is named
        assert status(ctx.conv_ir_free, idc) == -1
        twin = ctx.conv_create(idc)  # c is still loaded and usable
        ctx.conv_set_levels(twin, 0.25, 1.0)
        ref = TrueStereoRef(arrays["c"], 0.25, 1.0)
        close("the twin", [ctx.conv_process([twin], x)[0] for x in blocks[:2]], [ref.process(x[0]) for x in blocks[:2]])


def test_in_place_device_memory(gas):
    import torch

    F, n = 256, 3
    rng = np.random.default_rng(120)
    irs = [decaying(rng, ch, 2 * F + 1) for ch in (4, 2, 4)]
    blocks = noise(rng, 4, n, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2 * n, 3 * F)
        ids = [ctx.conv_ir_load(h) for h in irs]
        dev, host = [ctx.conv_create(i) for i in ids], [ctx.conv_create(i) for i in ids]
        for k in dev + host:
            ctx.conv_set_levels(k, 0.5, 1.0)
        d = [torch.from_numpy(x).cuda() for x in blocks]
        torch.cuda.synchronize()
        for t in d:
            assert ctx.conv_process(dev, t) is t  # out == in, only enqueued
        ctx.synchronize()
        got = [t.cpu().numpy() for t in d]
        for g, x in zip(got, blocks):
            assert np.array_equal(g, ctx.conv_process(host, x))
    for i, h in enumerate(irs):
        ref = TrueStereoRef(h, 0.5, 1.0)
        close(f"in place[{i}]", [g[i] for g in got], [ref.process(x[i]) for x in blocks])


def test_abi_behaviour(gas):
    F = 128
    rng = np.random.default_rng(130)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, 2 * F)
        for channels in (3, 5, 8):
            assert status(ctx.conv_ir_load, np.zeros((channels, 4), np.float32)) == -1
        bad = decaying(rng, 4, 2 * F)
        bad[3, 2 * F - 1] = np.inf
        assert status(ctx.conv_ir_load, bad) == -1
        assert status(ctx.conv_ir_load, np.zeros((4, 2 * F + 1), np.float32)) == -1  # longer than the reservation
        assert status(ctx.conv_ir_get_info, 0) == -3  # nothing was loaded
        ids = {ch: ctx.conv_ir_load(decaying(rng, ch, taps)) for ch, taps in ((4, 4), (1, 2 * F), (2, F + 1))}
        assert ctx.conv_ir_get_info(ids[4]) == (4, 4)
        assert ctx.conv_ir_get_info(ids[1]) == (1, 2 * F)
        assert ctx.conv_ir_get_info(ids[2]) == (2, F + 1)
        assert status(ctx.conv_ir_get_info, 3) == -3
        assert ctx.lib.gas_conv_ir_get_info(ctx.h, ids[4], None, None) == 0  # either output may be NULL
        assert ctx.lib.gas_conv_ir_get_info(None, ids[4], None, None) == -1
        ctx.conv_ir_free(ids[2])
        assert status(ctx.conv_ir_get_info, ids[2]) == -3
        ctx.conv_ir_free(ids[4]), ctx.conv_ir_free(ids[1])
        ctx.reserve_conv(0, 0)  # the refusals left nothing behind
