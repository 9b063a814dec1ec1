"""gas_conv_fade_to on the GPU against tests/conv_fade_ref.py's float64 reference of the header's fade rule.

Tolerance: helpers.TOL (1e-5 relative RMS over an instance's whole output), the band tests/test_gpu_conv.py uses;
bitwise where a test says so.  Every case prints its figure before it asserts."""
import numpy as np
import pytest

from conv_fade_ref import ConvFadeRef
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


def status(call, *a):
    with pytest.raises(Exception) as ei:
        call(*a)
    return ei.value.status


class Rig:
    """One instance of a context and its ConvFadeRef, given the same calls.  irs: name -> (array, id in the context)."""

    def __init__(self, ctx, irs, F, name, dry=0.0, wet=1.0):
        self.ctx, self.irs = ctx, irs
        self.conv = ctx.conv_create(irs[name][1])
        ctx.conv_set_levels(self.conv, dry, wet)
        self.ref = ConvFadeRef(F, irs[name][0], dry, wet)

    def fade_to(self, name, dry, wet, n):
        self.ctx.conv_fade_to(self.conv, self.irs[name][1], dry, wet, n)
        self.ref.fade_to(self.irs[name][0], dry, wet, n)

    def set_ir(self, name):
        self.ctx.conv_set_ir(self.conv, self.irs[name][1])
        self.ref.set_ir(self.irs[name][0])

    def set_levels(self, dry, wet):
        self.ctx.conv_set_levels(self.conv, dry, wet)
        self.ref.set_levels(dry, wet)

    def reset(self):
        self.ctx.conv_reset(self.conv)
        self.ref.reset()

    def remaining(self):
        got = self.ctx.conv_fade_remaining(self.conv)
        assert got == self.ref.fade_remaining()
        return got


def load(ctx, **arrays):
    return {k: (h, ctx.conv_ir_load(h)) for k, h in arrays.items()}


def run(ctx, rigs, blocks, events=None, name="fade"):
    """events: block index -> callable run before that block's call.  Returns per rig the stacked output, checked
    against the rig's reference."""
    got, want = [], []
    for b, x in enumerate(blocks):
        if events and b in events:
            events[b]()
        for r in rigs:
            r.remaining()
        got.append(ctx.conv_process([r.conv for r in rigs], x))
        want.append(np.stack([r.ref.process(x[i]) for i, r in enumerate(rigs)]))
    for r in rigs:
        r.remaining()
    got, want = np.stack(got), np.stack(want)
    for i in range(len(rigs)):
        close(f"{name}[{i}]", got[:, i], want[:, i])
        for b in range(len(blocks)):
            print(f"  {name}[{i}] block {b}: rel rms {rel_rms(got[b, i], want[b, i]):.3g}")
    return got


@pytest.mark.parametrize("F", [128, 384, 512])
def test_lengths_and_chunk_splits(gas, F):
    """A: 5 taps, one channel, one partition.  B: 17 F + 3 taps, two channels, 18 partitions -- two chunks, the second
    short.  A -> B over three calls; at F = 128 then B -> A over one."""
    rng = np.random.default_rng(20 + F)
    taps_b = 17 * F + 3
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, taps_b)
        irs = load(ctx, a=decaying(rng, 1, 5), b=decaying(rng, 2, taps_b))
        r = Rig(ctx, irs, F, "a")
        events = {2: lambda: r.fade_to("b", 0.25, 0.5, 3)}
        if F == 128:
            events[7] = lambda: r.fade_to("a", 0.0, 1.0, 1)
        run(ctx, [r], noise(rng, 10 if F == 128 else 6, 1, F), events, f"lengths F {F}")
        assert r.remaining() == 0


def test_ring_wrap_inside_a_fade(gas):
    F = 128
    rng = np.random.default_rng(31)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, 3 * F)
        irs = load(ctx, a=decaying(rng, 2, 3 * F), b=decaying(rng, 2, 3 * F))
        r = Rig(ctx, irs, F, "a")
        run(ctx, [r], noise(rng, 9, 1, F), {2: lambda: r.fade_to("b", 0.0, 1.0, 5)}, "ring wrap")


def test_after_the_fade_bitwise_a_hard_switch(gas):
    F = 128
    rng = np.random.default_rng(32)
    a, b = decaying(rng, 1, F + 9), decaying(rng, 2, 17 * F + 3)
    blocks = noise(rng, 8, 1, F)
    outs = []
    for n in (3, 0):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_conv(1, 17 * F + 3)
            irs = load(ctx, a=a, b=b)
            r = Rig(ctx, irs, F, "a", 0.5, 0.5)
            outs.append(run(ctx, [r], blocks, {2: lambda: r.fade_to("b", 0.25, 1.0, n)}, f"fade over {n}")[:, 0])
    faded, hard = outs
    np.testing.assert_array_equal(faded[:2], hard[:2])
    np.testing.assert_array_equal(faded[5:], hard[5:])
    assert not np.array_equal(faded[2], hard[2])
    # the first block of the fade starts at s = 0: against the reference alone (run() checked the whole output)
    ref = ConvFadeRef(F, a, 0.5, 0.5)
    for x in blocks[:2]:
        ref.process(x[0])
    ref.fade_to(b, 0.25, 1.0, 3)
    close("first block of the fade", faded[2], ref.process(blocks[2][0]))


def test_24_fading_instances_in_one_call(gas):
    """The partial sums' sizing at its maximum: 24 instances, every one fading between two IRs of its own pair of
    lengths, from 1 tap to the reservation.  One call naming all is bitwise one call per instance in a second context."""
    F, n, R = 128, 24, 20 * 128 + 3
    rng = np.random.default_rng(33)
    lens = [1, 2, F - 1, F, F + 1, 5 * F + 9, 17 * F, R]  # 17 and 21 partitions: two chunks
    arrays = {str(i): decaying(rng, 1 + i % 2, t) for i, t in enumerate(lens)}
    pairs = [(str(i % 8), str((i * 3 + 1 + i // 8) % 8)) for i in range(n)]  # (A, B): shorter, longer and equal lengths
    assert any(lens[int(p)] == R or lens[int(q)] == R for p, q in pairs)
    blocks = noise(rng, 5, n, F)
    outs, want = [], []
    for one_per_call in (False, True):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_conv(n, R)
            irs = load(ctx, **arrays)
            rigs = [Rig(ctx, irs, F, p) for p, _ in pairs]
            got = []
            for b, x in enumerate(blocks):
                if b == 1:
                    for i, (r, (_, q)) in enumerate(zip(rigs, pairs)):
                        r.fade_to(q, 0.25, 0.75, 2 + i % 3)
                if b in (1, 2):
                    assert all(r.remaining() > 0 for r in rigs)
                if one_per_call:
                    got.append(np.concatenate([ctx.conv_process([r.conv], x[i : i + 1]) for i, r in enumerate(rigs)]))
                else:
                    got.append(ctx.conv_process([r.conv for r in rigs], x))
                for i, r in enumerate(rigs):
                    w = r.ref.process(x[i])  # both contexts' references follow their instances
                    if not one_per_call:
                        want.append(w)
            outs.append(np.stack(got))
    want = np.stack(want).reshape(len(blocks), n, F, 2)
    for i in range(n):
        close(f"24 fading[{i}]", outs[0][:, i], want[:, i])
    np.testing.assert_array_equal(outs[0], outs[1])


def test_level_only_fade(gas):
    """ir unchanged, dry and wet changing sign on the way: (0.75, -0.5) -> (0, 1)."""
    F = 128
    rng = np.random.default_rng(34)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(1, 3 * F)
        irs = load(ctx, a=decaying(rng, 2, 2 * F + 3))
        r = Rig(ctx, irs, F, "a", 0.75, -0.5)
        run(ctx, [r], noise(rng, 6, 1, F), {1: lambda: r.fade_to("a", 0.0, 1.0, 3)}, "level only")
        ctx.conv_destroy(r.conv)
        ctx.conv_ir_free(irs["a"][1])  # both references went with the instance


def test_in_place_device_memory(gas):
    import torch

    F, n = 256, 3
    rng = np.random.default_rng(35)
    blocks = noise(rng, 5, n, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(2 * n, 3 * F)
        irs = load(ctx, **{str(i): decaying(rng, 1 + i % 2, 2 * F + 1 - i) for i in range(n + 1)})
        dev, host = [[Rig(ctx, irs, F, str(i), 0.5, 1.0) for i in range(n)] for _ in range(2)]
        d = [torch.from_numpy(x).cuda() for x in blocks]
        torch.cuda.synchronize()
        for b, t in enumerate(d):
            if b == 1:
                for i, r in enumerate(dev):
                    ctx.conv_fade_to(r.conv, irs[str(i + 1)][1], 0.0, 1.0, 3)  # the references follow the host run below
            assert ctx.conv_process([r.conv for r in dev], t) is t  # out == in, only enqueued
        ctx.synchronize()
        got = np.stack([t.cpu().numpy() for t in d])
        events = {1: lambda: [r.fade_to(str(i + 1), 0.0, 1.0, 3) for i, r in enumerate(host)]}
        np.testing.assert_array_equal(got, run(ctx, host, blocks, events, "in place"))


def test_state_machine(gas):
    F = 128
    rng = np.random.default_rng(36)
    blocks = noise(rng, 12, 4, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(6, 3 * F)
        irs = load(ctx, a=decaying(rng, 2, 9), b=decaying(rng, 2, F + 5), c=decaying(rng, 1, 3 * F), d=decaying(rng, 2, 3))
        pend, skip, cut, rst = (Rig(ctx, irs, F, "a") for _ in range(4))
        rigs = [pend, skip, cut, rst]
        fresh = {}
        got, want, seen = [], [], []
        for b, x in enumerate(blocks):
            if b == 1:
                for r in rigs:
                    r.fade_to("b", 0.5, 0.5, 3)
            if b == 2:  # two more targets during the fade: the latest is kept and starts when this fade has ended
                pend.fade_to("c", 1.0, 1.0, 5)
                assert pend.remaining() == 2 + 5
                pend.fade_to("d", 0.0, 2.0, 2)
                assert pend.remaining() == 2 + 2
            if b == 3:
                cut.set_ir("c")  # ends the fade in B = (b, 0.5, 0.5), then switches the IR
                assert cut.remaining() == 0
                rst.fade_to("d", 0.25, -1.0, 4)
                rst.reset()  # the final state is the pending target's
                assert rst.remaining() == 0
                fresh["conv"] = ctx.conv_create(irs["d"][1])
                ctx.conv_set_levels(fresh["conv"], 0.25, -1.0)
                fresh["out"] = []
            named = [i for i, r in enumerate(rigs) if not (r is skip and b == 2)]  # a call that does not name `skip`
            seen.append([r.remaining() for r in rigs])
            o = ctx.conv_process([rigs[i].conv for i in named], x[named])
            row_o, row_w = np.zeros_like(x), np.zeros((4, F, 2))
            for j, i in enumerate(named):
                row_o[i], row_w[i] = o[j], rigs[i].ref.process(x[i])
            got.append(row_o), want.append(row_w)
            if b >= 3:
                fresh["out"].append(ctx.conv_process([fresh["conv"]], x[3:4])[0])
        got, want = np.stack(got), np.stack(want)
        for i, nm in enumerate(("pending", "skipped call", "set_ir mid-fade", "reset mid-fade")):
            close(f"state machine: {nm}", got[:, i], want[:, i])
        np.testing.assert_array_equal(got[3:, 3], np.stack(fresh["out"]))  # bitwise a fresh instance in the final state
        assert [s[0] for s in seen] == [0, 3, 4, 3, 2, 1, 0, 0, 0, 0, 0, 0]
        assert [s[1] for s in seen] == [0, 3, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0]  # the skipped call did not advance it
        assert [s[2] for s in seen] == [0, 3, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def test_ir_lifetime_and_refusals(gas):
    F = 128
    rng = np.random.default_rng(37)
    blocks = noise(rng, 6, 2, F)
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
        ctx.reserve_conv(3, 2 * F)
        irs = load(ctx, a=decaying(rng, 2, 9), b=decaying(rng, 2, F + 5), c=decaying(rng, 1, 2 * F))
        ida, idb, idc = (irs[k][1] for k in "abc")
        r, twin = Rig(ctx, irs, F, "a"), Rig(ctx, irs, F, "a")  # the twin hears the same input and none of the refusals

        def both(x):
            o = ctx.conv_process([r.conv, twin.conv], np.stack([x[0], x[0]]))
            np.testing.assert_array_equal(o[0], o[1])
            close("around refusals", o[0], r.ref.process(x[0]))
            twin.ref.process(x[0])

        both(blocks[0])
        for rig in (r, twin):
            rig.fade_to("b", 0.5, 0.5, 3)
        both(blocks[1])
        # refusals mid-fade: nothing changes
        assert status(ctx.conv_fade_to, r.conv, idc, 0.0, 1.0, 4097) == -1
        assert status(ctx.conv_fade_to, r.conv, idc, np.nan, 1.0, 2) == -1
        assert status(ctx.conv_fade_to, r.conv, idc, 0.0, np.inf, 0) == -1
        assert status(ctx.conv_fade_to, 7, idc, 0.0, 1.0, 2) == -3
        assert status(ctx.conv_fade_to, r.conv, 9, 0.0, 1.0, 2) == -3
        assert status(ctx.conv_fade_to, r.conv, 9, 0.0, 1.0, 0) == -3
        assert status(ctx.conv_fade_remaining, 7) == -3
        assert ctx.lib.gas_conv_fade_remaining(ctx.h, r.conv, None) == -1
        assert r.remaining() == 2 and twin.remaining() == 2
        ctx.conv_ir_free(idc)  # no refused call took a reference
        irs["c"] = (irs["c"][0], ctx.conv_ir_load(irs["c"][0]))
        idc = irs["c"][1]
        both(blocks[2])
        # A's, B's and a pending target's IR are all named
        for rig in (r, twin):
            rig.fade_to("c", 0.0, 1.0, 2)
        for i in (ida, idb, idc):
            assert status(ctx.conv_ir_free, i) == -1
        both(blocks[3])  # the first fade's last call: A is no longer named by r or twin
        assert r.remaining() == 2
        ctx.conv_ir_free(ida)
        assert status(ctx.conv_ir_free, idb) == -1 and status(ctx.conv_ir_free, idc) == -1
        both(blocks[4])
        # destroy mid-fade releases B's and the new target's
        ctx.conv_destroy(r.conv), ctx.conv_destroy(twin.conv)
        ctx.conv_ir_free(idb), ctx.conv_ir_free(idc)
        # the cap itself is legal
        h = ctx.conv_ir_load(irs["a"][0])
        k = ctx.conv_create(h)
        ctx.conv_fade_to(k, h, 1.0, 0.0, 4096)
        assert ctx.conv_fade_remaining(k) == 4096
        ctx.conv_set_levels(k, 0.0, 1.0)  # ends it
        assert ctx.conv_fade_remaining(k) == 0


def test_settled_bystanders(gas):
    """A call that mixes fading and settled instances: the settled ones are bitwise what a call without the fading
    ones gives, and the fading ones bitwise what a call without the settled ones gives."""
    F = 128
    rng = np.random.default_rng(38)
    blocks = noise(rng, 5, 6, F)
    fading = [1, 2, 4]
    outs = {}
    for mode in ("mixed", "settled alone", "fading alone"):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            ctx.reserve_conv(6, 20 * F + 3)
            r2 = np.random.default_rng(39)
            irs = load(ctx, **{str(i): decaying(r2, 1 + i % 2, t) for i, t in enumerate((5, 17 * F + 3, F + 1, 20 * F + 3))})
            rigs = [Rig(ctx, irs, F, str(i % 4), 0.25, 0.75) for i in range(6)]
            named = {"mixed": list(range(6)), "settled alone": [i for i in range(6) if i not in fading], "fading alone": fading}[mode]
            got, want = [], []
            for b, x in enumerate(blocks):
                if b == 1:
                    for i in fading:
                        rigs[i].fade_to(str((i + 1) % 4) if i != 4 else "0", 0.0, 1.0, 3)  # instance 4: a level-only fade
                o = np.zeros_like(x)
                o[named] = ctx.conv_process([rigs[i].conv for i in named], x[named])
                got.append(o)
                if mode == "mixed":
                    want.append(np.stack([r.ref.process(x[i]) for i, r in enumerate(rigs)]))
            outs[mode] = np.stack(got)
            if mode == "mixed":
                for i in range(6):
                    close(f"bystander mix[{i}]", outs[mode][:, i], np.stack(want)[:, i])
    settled = [i for i in range(6) if i not in fading]
    np.testing.assert_array_equal(outs["mixed"][:, settled], outs["settled alone"][:, settled])
    np.testing.assert_array_equal(outs["mixed"][:, fading], outs["fading alone"][:, fading])
