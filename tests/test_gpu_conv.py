"""The bus convolvers (gas_conv_*) on the GPU against tests/conv_ref.py's float64 direct-form reference.

Tolerance: helpers.TOL (1e-5 relative RMS over an instance's whole output), the project's band for its 1024-point f32
transforms; bitwise where a test says so.  Every case prints its figure before it asserts."""
import numpy as np
import pytest

from conv_ref import ConvRef
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu


def noise(rng, blocks, n, F):
    return [rng.uniform(-1, 1, (n, F, 2)).astype(np.float32) for _ in range(blocks)]


def decaying(rng, channels, taps):
    return (rng.standard_normal((channels, taps)) * np.exp(-4.0 * np.arange(taps) / taps)).astype(np.float32)


def close(name, got, want):
    err = rel_rms(got, want)
    print(f"{name}: rel rms {err:.3g}")
    assert err <= TOL, (name, err)


def check(name, outs, refs, blocks):
    """outs: per block [n][F][2]; refs: one ConvRef per instance, fed its row of every block."""
    for i, r in enumerate(refs):
        want = np.stack([r.process(x[i]) for x in blocks])
        close(f"{name}[{i}]", np.stack([o[i] for o in outs]), want)


def test_delta_and_scaled_delta_ir(gas):
    F = 128
    rng = np.random.default_rng(1)
    blocks = noise(rng, 3, 2, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, F)
        irs = [np.array([1.0], np.float32), np.array([[0.5], [-0.25]], np.float32)]
        convs = [ctx.conv_create(ctx.conv_ir_load(h)) for h in irs]
        for dry, wet in ((0.0, 1.0), (1.0, 0.0), (0.5, 0.25)):
            for k in convs:
                ctx.conv_reset(k)
                ctx.conv_set_levels(k, dry, wet)
            outs = [ctx.conv_process(convs, x) for x in blocks]
            if wet == 0.0:  # the wet path contributes an exact zero
                for o, x in zip(outs, blocks):
                    np.testing.assert_array_equal(o, np.float32(dry) * x)
            check(f"delta dry {dry} wet {wet}", outs, [ConvRef(h, dry, wet) for h in irs], blocks)


@pytest.mark.parametrize("F,taps", [(128, (1, 127, 128, 129, 256, 383)), (256, (256, 257)), (384, (384, 385)), (512, (512, 513))])
def test_partition_edges(gas, F, taps):
    """IR lengths on both sides of a partition edge; two-channel IRs with different ears, and a one-channel IR that
    gives both ears the same filter (bitwise what the two-channel IR of two equal channels gives)."""
    rng = np.random.default_rng(F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(3 * len(taps), 3 * F)
        irs = []
        for t in taps:
            two, one = decaying(rng, 2, t), decaying(rng, 1, t)
            irs += [two, one, np.concatenate([one, one])]
        convs = [ctx.conv_create(ctx.conv_ir_load(h)) for h in irs]
        blocks = noise(rng, 6, len(convs), F)
        for x in blocks:
            x[2::3] = x[1::3]  # the one-channel IR and its two-channel twin hear the same input
        outs = [ctx.conv_process(convs, x) for x in blocks]
        check(f"edges F {F}", outs, [ConvRef(h) for h in irs], blocks)
        for o in outs:
            np.testing.assert_array_equal(o[1::3], o[2::3])


def test_ring_wrap(gas):
    F = 128
    rng = np.random.default_rng(5)
    ir = decaying(rng, 2, 5 * F)
    blocks = noise(rng, 13, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, 5 * F)
        convs = [ctx.conv_create(ctx.conv_ir_load(ir))]
        check("ring wrap", [ctx.conv_process(convs, x) for x in blocks], [ConvRef(ir)], blocks)


def test_long_ir(gas):
    """41 partitions: three chunks of the multiply-accumulate, the last one short."""
    F = 128
    taps = 40 * F + 17
    rng = np.random.default_rng(6)
    ir = decaying(rng, 2, taps)
    blocks = noise(rng, 45, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, taps)
        convs = [ctx.conv_create(ctx.conv_ir_load(ir))]
        check("long ir", [ctx.conv_process(convs, x) for x in blocks], [ConvRef(ir)], blocks)


def test_24_instances_in_one_call(gas):
    """Shared and distinct IRs from 1 tap to the reservation.  One call naming all of them is bitwise the same
    instances processed one per call in a second context; an instance left out of a call resumes as if no time had
    passed."""
    F, n, R = 128, 24, 20 * 128 + 3
    rng = np.random.default_rng(7)
    lens = [1, 2, F - 1, F, F + 1, 5 * F + 9, 17 * F, R]  # 17 and 21 partitions: two chunks
    irs = [decaying(rng, 1 + i % 2, t) for i, t in enumerate(lens)]
    which = [i % len(irs) for i in range(n)]
    blocks = noise(rng, 4, n, F)
    skip_block, skipped = 2, 5
    outs = []
    for one_per_call in (False, True):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_conv(n, R)
            ids = [ctx.conv_ir_load(h) for h in irs]
            convs = [ctx.conv_create(ids[w]) for w in which]
            got = []
            for b, x in enumerate(blocks):
                named = [i for i in range(n) if not (b == skip_block and i == skipped)]
                o = np.zeros_like(x)
                if one_per_call:
                    for i in named:
                        o[i] = ctx.conv_process([convs[i]], x[i : i + 1])[0]
                else:
                    o[named] = ctx.conv_process([convs[i] for i in named], x[named])
                got.append(o)
            with pytest.raises(gas.GasError) as ei:  # the pool is empty
                ctx.conv_create(ids[0])
            assert ei.value.status == -2
            outs.append(got)
    np.testing.assert_array_equal(np.stack(outs[0]), np.stack(outs[1]))
    for i in range(n):
        r = ConvRef(irs[which[i]])
        mine = [b for b in range(len(blocks)) if not (b == skip_block and i == skipped)]
        want = np.stack([r.process(blocks[b][i]) for b in mine])
        close(f"24 instances[{i}]", np.stack([outs[0][b][i] for b in mine]), want)


def test_ir_switching_and_level_changes(gas):
    """gas_conv_set_ir to a longer and to a shorter IR mid-run: a hard switch over the history the instance holds;
    new levels apply at the next call."""
    F = 128
    rng = np.random.default_rng(8)
    short, long_, mid = decaying(rng, 1, 5), decaying(rng, 2, 3 * F), decaying(rng, 2, F + 1)
    blocks = noise(rng, 9, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, 3 * F)
        ids = {k: ctx.conv_ir_load(h) for k, h in (("short", short), ("long", long_), ("mid", mid))}
        conv = ctx.conv_create(ids["short"])
        ref = ConvRef(short)
        got, want = [], []
        for b, x in enumerate(blocks):
            if b == 2:
                ctx.conv_set_levels(conv, 0.75, -0.5), ref.set_levels(0.75, -0.5)
            if b == 3:
                ctx.conv_set_ir(conv, ids["long"]), ref.set_ir(long_)
            if b == 6:
                ctx.conv_set_ir(conv, ids["mid"]), ref.set_ir(mid)
            if b == 7:
                ctx.conv_set_levels(conv, 0.0, 1.0), ref.set_levels(0.0, 1.0)
            got.append(ctx.conv_process([conv], x)[0])
            want.append(ref.process(x[0]))
            close(f"switching block {b}", got[-1], want[-1])


def test_reset_and_recycling(gas):
    """gas_conv_reset is bitwise a fresh instance; destroy plus create recycles a zeroed ring."""
    F = 128
    rng = np.random.default_rng(9)
    ir = decaying(rng, 2, 3 * F)
    a, b = noise(rng, 4, 1, F), noise(rng, 4, 1, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2, 3 * F)
        h = ctx.conv_ir_load(ir)
        fresh = ctx.conv_create(h)
        want = [ctx.conv_process([fresh], x) for x in b]
        conv = ctx.conv_create(h)
        for x in a:
            ctx.conv_process([conv], x)
        ctx.conv_reset(conv)
        for x, w in zip(b, want):
            np.testing.assert_array_equal(ctx.conv_process([conv], x), w)
        ctx.conv_destroy(conv)
        again = ctx.conv_create(h)
        assert again == conv  # the same ring, handed out again
        for x, w in zip(b, want):
            np.testing.assert_array_equal(ctx.conv_process([again], x), w)
        check("reset", want, [ConvRef(ir)], b)


def test_in_place_device_memory(gas):
    import torch

    F, n = 256, 3
    rng = np.random.default_rng(10)
    irs = [decaying(rng, 2, 2 * F + 1) for _ in range(n)]
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
            np.testing.assert_array_equal(g, ctx.conv_process(host, x))
        check("in place", got, [ConvRef(h, 0.5, 1.0) for h in irs], blocks)


def test_bus_mix_to_convolver_without_a_synchronise(gas):
    """Eight [HRTF] sources onto two buses in device memory, bus 1 convolved straight from that `out`, four callbacks
    enqueued back to back; against the reference over the bus rows a host-memory run of the same scene returns."""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, n, dirs, cbs = 128, 8, 16, 4
    rng = np.random.default_rng(11)
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=dirs)
    p = synth.draw_params(rng, n, dirs=dirs, frames=F)
    srcs = [synth.draw_sources(rng, n, F) for _ in range(cbs)]
    routes = K.bus_routes(n)
    routes["send_bus"] = 1
    routes["send"][:, 0, :] = 0.5
    ir = decaying(rng, 2, 3 * F + 7)

    def scene(ctx):
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
        ctx.params_publish_batch(slots, p)
        ctx.bus_routes_publish(slots, routes)
        return slots

    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        slots = scene(ctx)
        bus1 = [ctx.process_block_buses(s, slots, 2)[0][1] for s in srcs]  # [C = 1][F][2] each
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        slots = np.ascontiguousarray(scene(ctx), np.uint32)
        ctx.reserve_conv(1, 4 * F)
        conv = ctx.conv_create(ctx.conv_ir_load(ir))
        d_src = [torch.from_numpy(s).cuda() for s in srcs]
        d_bus = torch.zeros(cbs, 2, 1, F, 2, device="cuda")
        d_wet = torch.zeros(cbs, 1, F, 2, device="cuda")
        d_pk = torch.zeros(n, 2, device="cuda")
        torch.cuda.synchronize()
        for b in range(cbs):
            assert ctx.lib.gas_process_block_buses(ctx.h, d_src[b].data_ptr(), slots.ctypes.data, n, F, d_bus[b].data_ptr(), 2, d_pk.data_ptr(), K.MEM_DEVICE) == 0
            ctx.conv_process([conv], d_bus[b, 1], out=d_wet[b])
        ctx.synchronize()
        wet = d_wet.cpu().numpy()
    check("bus 1 -> convolver", [w for w in wet], [ConvRef(ir)], bus1)


def test_waiting_callbacks_run_first(gas):
    """GAS_FLAG_BATCHED_LAUNCH | GAS_FLAG_PIPELINED_MIX: two callbacks still wait for their batch when the convolver is
    given the second one's `out`; it must hear that mix, not what the buffer held before."""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, n, dirs = 512, 2048, 16
    rng = np.random.default_rng(14)
    ir = decaying(rng, 2, F + 9)
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PIPELINED_MIX | K.FLAG_BATCHED_LAUNCH) as ctx:
        ctx.hrtf_load(synth.synthetic_hrir(np.random.default_rng(7), dirs=dirs))
        ctx.set_batch_depth(3)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
        ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=dirs))
        ctx.reserve_conv(1, 2 * F)
        conv = ctx.conv_create(ctx.conv_ir_load(ir))
        d_src = [torch.from_numpy(synth.draw_sources(rng, n, F)).cuda() for _ in range(2)]
        d_out = torch.zeros(2, 1, F, 2, device="cuda")
        d_wet = torch.zeros(1, F, 2, device="cuda")
        d_pk = torch.zeros(2, n, 2, device="cuda")
        torch.cuda.synchronize()
        for t in range(2):
            assert ctx.process_block_raw(d_src[t].data_ptr(), slots if t == 0 else None, n, F, d_out[t].data_ptr(), d_pk[t].data_ptr(), K.MEM_DEVICE) == 0
        ctx.conv_process([conv], d_out[1], out=d_wet)
        ctx.synchronize()
        mix = d_out[1].cpu().numpy()
        assert np.abs(mix).max() > 0
        close("behind waiting callbacks", d_wet.cpu().numpy()[0], ConvRef(ir).process(mix[0]))


def test_refusals_change_nothing(gas):
    K = gas.capi
    F = 128
    rng = np.random.default_rng(12)
    ir = decaying(rng, 2, 2 * F)
    blocks = noise(rng, 3, 2, F)

    def status(call, *a):
        with pytest.raises(gas.GasError) as ei:
            call(*a)
        return ei.value.status

    def refused(ctx, want, convs, n, x, frames=F):
        out = np.full((max(n, 1), frames, 2), np.nan, np.float32)
        assert ctx.conv_process_raw(convs, n, x.ctypes.data, out.ctypes.data, frames, K.MEM_HOST) == want
        assert not out[: min(n, 24)].any()  # a refused host-memory call leaves zeros

    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        # nothing reserved
        assert status(ctx.conv_ir_load, ir) == -6
        assert status(ctx.conv_create, 0) == -6
        refused(ctx, -3, [0], 1, blocks[0])
        assert status(ctx.reserve_conv, 25, F) == -1
        assert status(ctx.reserve_conv, 1, (1 << 20) + 1) == -1
        assert status(ctx.reserve_conv, 1, 0) == -1
        ctx.reserve_conv(2, 2 * F)
        # IRs
        assert status(ctx.conv_ir_load, np.zeros((2, 2 * F + 1), np.float32)) == -1  # longer than the reservation
        assert status(ctx.conv_ir_load, np.zeros((3, 4), np.float32)) == -1
        assert status(ctx.conv_ir_load, np.zeros((1, 0), np.float32)) == -1
        bad = ir.copy()
        bad[1, 7] = np.inf
        assert status(ctx.conv_ir_load, bad) == -1
        bad[1, 7] = np.nan
        assert status(ctx.conv_ir_load, bad) == -1
        h = ctx.conv_ir_load(ir)
        assert status(ctx.reserve_conv, 0, 0) == -1  # an IR is held
        assert status(ctx.conv_create, h + 1) == -3
        a, b = ctx.conv_create(h), ctx.conv_create(h)
        assert status(ctx.conv_create, h) == -2
        assert status(ctx.reserve_conv, 4, 2 * F) == -1  # instances are held
        assert status(ctx.conv_ir_free, h) == -1  # in use
        assert status(ctx.conv_ir_free, h + 1) == -3
        for call, args in ((ctx.conv_destroy, (7,)), (ctx.conv_reset, (7,)), (ctx.conv_set_ir, (7, h)), (ctx.conv_set_ir, (a, h + 1)), (ctx.conv_set_levels, (7, 0.0, 1.0))):
            assert status(call, *args) == -3
        assert status(ctx.conv_set_levels, a, np.nan, 1.0) == -1
        assert status(ctx.conv_set_levels, a, 0.0, np.inf) == -1
        # process: every refusal between two good blocks, which must come out as if nothing had happened
        first = ctx.conv_process([a, b], blocks[0])
        refused(ctx, -4, [a, b], 2, np.zeros((2, 2 * F, 2), np.float32), frames=2 * F)
        refused(ctx, -1, [a, a], 2, blocks[1])
        refused(ctx, -3, [a, 2], 2, blocks[1])
        refused(ctx, -1, list(range(25)), 25, np.zeros((25, F, 2), np.float32))
        assert ctx.conv_process_raw(None, 0, 0, 0, F, K.MEM_HOST) == 0  # n == 0
        assert ctx.conv_process_raw([a], 1, blocks[1].ctypes.data, blocks[1].ctypes.data, F, 7) == -1
        second = ctx.conv_process([a, b], blocks[1])
        check("around refusals", [first, second], [ConvRef(ir), ConvRef(ir)], blocks[:2])
        # released once nothing is held
        ctx.conv_destroy(a), ctx.conv_destroy(b)
        ctx.conv_ir_free(h)
        ctx.reserve_conv(0, 0)
        assert status(ctx.conv_ir_load, ir) == -6


def test_unreserved_bystander(gas):
    """A context that reserved (and used) convolvers returns bitwise the gas_process_block output of one that did not."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, n, dirs = 128, 48, 16
    rng = np.random.default_rng(13)
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=dirs)
    p = synth.draw_params(rng, n, dirs=dirs, frames=F)
    srcs = [synth.draw_sources(rng, n, F) for _ in range(3)]
    ir = decaying(rng, 2, 3 * F)
    outs = []
    for reserve in (False, True):
        with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
            ctx.hrtf_load(hrir)
            slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
            ctx.params_publish_batch(slots, p)
            if reserve:
                ctx.reserve_conv(2, 3 * F)
                conv = ctx.conv_create(ctx.conv_ir_load(ir))
            got = []
            for s in srcs:
                got.append(ctx.process_block(s, slots))
                if reserve:
                    ctx.conv_process([conv], got[-1][0])
            outs.append(got)
    for (m0, p0), (m1, p1) in zip(*outs):
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(p0, p1)
