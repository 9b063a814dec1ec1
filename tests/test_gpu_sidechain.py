"""The compressor's sidechain on the GPU (gas_sidechain_set, gas_fx_dyn_settings.compressor_sidechain, k_fx_dyn.hip)
against the numpy restatement tests/fx_sidechain_ref.py, composed with the oracle's existing kinds for mixed chains.
Shapes are the smallest that cross the kernel's seams: 64 sources per workgroup, 32 frames per tile."""
import numpy as np
import pytest

import fx_dyn_ref as ref
import fx_sidechain_ref as sc
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HS, ER, HRTF, LP, AMP = 1, 2, 3, 4, 9
DIST, COMP = 11, 12
NK = sc.MAX_SIDECHAINS
INVALID, FRAME_COUNT = -1, -4


def _hrir(dirs=32, seed=5):
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(seed), dirs=dirs)


class ChainRef:
    """A playback chain's reference (the composition test_gpu_fx_dyn.py uses): runs of the existing kinds through
    BatchOracle (one source per oracle where a new kind follows, for its rows; all sources in one oracle for a last
    run), the distortion through fx_dyn_ref, the compressor through fx_sidechain_ref with the callback's key blocks."""

    def __init__(self, ob, chain, n, frames, hrir=None, ring=0):
        self.stages = []
        segs = []
        for j, k in enumerate(chain):
            dyn = k in (DIST, COMP)
            if segs and not dyn and not segs[-1][0]:
                segs[-1][1].append(j)
            else:
                segs.append((dyn, [j]))
        for si, (dyn, pos) in enumerate(segs):
            if dyn:
                j = pos[0]
                self.stages.append(("comp", sc.KeyedStage(j, n)) if chain[j] == COMP else ("dist", ref.DynStage(DIST, j, n)))
                continue
            sub = tuple(chain[j] for j in pos)
            mk = lambda m: ob.BatchOracle(ob.KIND_EFFECT, m, frames, chain=sub, hrir=hrir, er_ring_frames=max(ring, 1))  # noqa: E731
            if si == len(segs) - 1:
                self.stages.append(("last", mk(n)))
            else:
                self.stages.append(("rows", [mk(1) for _ in range(n)]))

    def comp(self, k=0):
        return [obj for kind, obj in self.stages if kind == "comp"][k]

    def rows(self, src, settings, keys):
        """The rows behind a chain of the dyn kinds only."""
        x = np.asarray(src, np.float32)
        for kind, obj in self.stages:
            assert kind in ("comp", "dist")
            x = obj.block(x, keys, settings) if kind == "comp" else obj.block(x, settings)
        return x

    def block(self, params, src, settings, keys):
        """-> (mix64 [F][2], peaks [n][2])."""
        import oracle.binding as ob

        p = params.astype(ob.PARAMS_DTYPE)
        x = np.asarray(src, np.float32)
        for kind, obj in self.stages:
            if kind == "comp":
                x = obj.block(x, keys, settings)
            elif kind == "dist":
                x = obj.block(x, settings)
            elif kind == "rows":
                x = np.stack([o.block(p[s : s + 1], x[s : s + 1])[0][0] for s, o in enumerate(obj)])
            else:
                _, peaks, r64 = obj.block(p, x, want64=True)
                return r64[0], peaks
        return x.astype(np.float64).sum(axis=0), np.abs(x).max(axis=1)


def _tone(amp, b, F, period=96.0):
    return (amp * np.sin(2 * np.pi * (np.arange(F) + b * F) / period)).astype(np.float32)


def make_keys(rng, b, F):
    """Eight distinct keys of block b.  draw_settings' thresholds lie in -60 .. 0 dB (0.001 .. 1): key 0 is over most of
    them, key 1 under all of them, key 6 between; key 2 is silent; keys 3 and 4 have one ear only; key 5 changes level
    every 20 frames, so attack and release both fall inside a 32-frame tile; key 7 is noise whose level moves per block."""
    k = np.zeros((NK, F, 2), np.float32)
    k[0] = _tone(0.9, b, F)[:, None]
    k[1] = _tone(0.0005, b, F, 50.0)[:, None]
    k[3, :, 0] = _tone(0.5, b, F, 70.0)
    k[4, :, 1] = _tone(0.3, b, F, 40.0)
    loud = (np.arange(F) // 20) % 2 == 0
    k[5] = (np.where(loud, 0.8, 0.002) * np.where(np.arange(F) % 2 == 0, 1.0, -1.0)).astype(np.float32)[:, None]
    k[6] = _tone(0.05, b, F, 33.0)[:, None] * np.array([1.0, -0.5], np.float32)
    k[7] = (rng.uniform(-1, 1, (F, 2)) * [0.01, 0.9, 0.9, 0.03, 0.0, 0.5, 0.002, 0.7, 0.1][b % 9]).astype(np.float32)
    return k


def set_keys(ctx, keys):
    for k in range(NK):
        ctx.sidechain_set(k, keys[k])


def keyed_settings(rng, n, gas, position=0, sidechain=None, **kw):
    """draw_settings plus a random sidechain per position; `sidechain` fixes the one at `position`."""
    s = ref.draw_settings(rng, n, gas.capi, **kw)
    s["compressor_sidechain"] = sc.draw_sidechains(rng, n, gas.capi.MAX_EFFECTS)
    if sidechain is not None:
        s["compressor_sidechain"][:, position] = sidechain
    return s


def _ctx(gas, n, F, chain, **kw):
    from godot_audio_spatializer_amd import synth

    ctx = gas.SpatializerContext(max_sources=n + 3, frames=F, **kw)
    slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
    p = synth.draw_params(np.random.default_rng(0), n, dirs=8, frames=F)
    ctx.params_publish_batch(slots, p)
    return ctx, slots, p


def _check(mix, peaks, want, rpeaks, what):
    err = rel_rms(mix, want)
    print(f"{what}: rel_rms {err:.3g}")
    assert err <= TOL, f"{what}: {err}"
    np.testing.assert_allclose(peaks, rpeaks, rtol=2e-5, atol=1e-7, err_msg=what)


@pytest.mark.parametrize("n,frames", [(1, 128), (63, 256), (64, 512), (65, 128), (130, 256)])
def test_keyed_compressor_alone(gas, ob, n, frames):
    """Source i on sidechain i % 9 (a workgroup holds the keyless case and all eight keys), keys re-set from host memory
    every block, settings re-published at blocks 1, 4 and 7 (all sources, then half of them with a new random key while
    rundb carries over)."""
    from godot_audio_spatializer_amd import synth

    rng = np.random.default_rng(100 + n)
    own = (np.arange(n) % 9).astype(np.uint32)
    with gas.SpatializerContext(max_sources=n + 3, frames=frames) as ctx:
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, (COMP,))
        r = ChainRef(ob, (COMP,), n, frames)
        settings = gas.capi.fx_dyn_settings_defaults(n)  # block 0: the resource defaults, keyed
        settings["compressor_sidechain"][:, 0] = own
        ctx.fx_dyn_settings_publish(slots, settings)
        saw_attack = saw_release = False
        for b in range(9):
            if b % 3 == 0:
                p = synth.draw_params(rng, n, dirs=8, frames=frames)
                ctx.params_publish_batch(slots, p)
            if b in (1, 4, 7):
                who = np.arange(n) if b == 1 else rng.choice(n, max(1, n // 2), replace=False)
                new = keyed_settings(rng, len(who), gas, sidechain=own[who] if b == 1 else None)
                ctx.fx_dyn_settings_publish(slots[who], new)
                settings[who] = new
            keys = make_keys(rng, b, frames)
            set_keys(ctx, keys)
            src = synth.draw_sources(rng, n, frames)
            keyed = settings["compressor_sidechain"][:, 0] != 0
            before = r.comp().rundb.copy()
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks = r.block(p, src, settings, keys)
            after = r.comp().rundb
            saw_attack = saw_attack or bool((after > before)[keyed].any())
            saw_release = saw_release or bool(((after < before) & (before > 0))[keyed].any())
            _check(mix[0], peaks, want, rpeaks, f"n={n} F={frames} block {b}")
        assert saw_attack and saw_release  # (n = 1: source 0 is keyless until block 4 gives it a key)


@pytest.mark.parametrize("frames,key", [(128, 4), (512, 7)])
def test_own_row_key_is_the_keyless_result_bitwise(gas, frames, key):
    """Two playbacks with identical settings and input, one keyless, one keyed on a key that holds the input row: the
    same peaks from gas_process_block and the same rows from gas_process_frames_1, to the bit."""
    rng = np.random.default_rng(7 + frames)
    ctx, slots, _ = _ctx(gas, 2, frames, (COMP,))
    with ctx:
        one = ref.draw_settings(rng, 1, gas.capi, edges=False)
        one["compressor_threshold_db"] = -30.0
        s = np.concatenate([one, one])
        s["compressor_sidechain"][1, 0] = key + 1
        ctx.fx_dyn_settings_publish(slots, s)
        worked = False
        for b in range(3):
            amp = [0.9, 0.01, 0.6][b]
            row = (rng.uniform(-1, 1, (frames, 2)) * amp).astype(np.float32)
            ctx.sidechain_set(key, row)
            mix, peaks = ctx.process_block(np.stack([row, row]), slots)
            np.testing.assert_array_equal(peaks[0], peaks[1])
            worked = worked or bool(np.abs(peaks[0] - np.abs(row).max(axis=0)).max() > 1e-3)
            row = (rng.uniform(-1, 1, (frames, 2)) * amp).astype(np.float32)
            ctx.sidechain_set(key, row)
            a = ctx.process_frames_1(int(slots[0]), row)
            c = ctx.process_frames_1(int(slots[1]), row)
            np.testing.assert_array_equal(a, c)
        assert worked  # the compressor did change the signal


def test_key_persists_until_replaced_and_null_zeroes_it(gas, ob):
    F, n = 128, 3
    rng = np.random.default_rng(21)
    ctx, slots, p = _ctx(gas, n, F, (COMP,))
    with ctx:
        s = keyed_settings(rng, n, gas, sidechain=3)
        s["compressor_threshold_db"] = -30.0
        ctx.fx_dyn_settings_publish(slots, s)
        r = ChainRef(ob, (COMP,), n, F)
        keys = np.zeros((NK, F, 2), np.float32)
        for b in range(5):
            if b == 0:
                keys[2] = rng.uniform(-0.9, 0.9, (F, 2)).astype(np.float32)
                ctx.sidechain_set(2, keys[2])
            elif b == 2:
                keys[2] = 0.0
                ctx.sidechain_set(2, None)
            # blocks 1, 3 and 4: no call -- the key's last block again
            src = rng.uniform(-0.1, 0.1, (n, F, 2)).astype(np.float32)
            before = r.comp().rundb.copy()
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks = r.block(p, src, s, keys)
            if b == 1:
                assert (r.comp().rundb > 0).all()  # still detecting on the loud key
            if b >= 2:
                assert (r.comp().rundb < before).all()  # released under the silent key
            _check(mix[0], peaks, want, rpeaks, f"block {b}")


@pytest.mark.parametrize("chain,frames", [((COMP, AMP, COMP), 128), ((COMP, HRTF), 256)])
def test_keys_by_chain_position(gas, ob, chain, frames):
    from godot_audio_spatializer_amd import synth

    n = 48
    rng = np.random.default_rng(31 + frames)
    hrir = _hrir() if HRTF in chain else None
    with gas.SpatializerContext(max_sources=n, frames=frames) as ctx:
        if hrir is not None:
            ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, gas.capi.KIND_EFFECT, chain)
        r = ChainRef(ob, chain, n, frames, hrir=hrir)
        s = keyed_settings(rng, n, gas, sidechain=1 + np.arange(n) % 4)
        if chain.count(COMP) == 2:
            s["compressor_sidechain"][:, 2] = 5 + np.arange(n) % 4  # other keys at the second compressor
        ctx.fx_dyn_settings_publish(slots, s)
        for b in range(4):
            p = synth.draw_params(rng, n, dirs=32, frames=frames)
            ctx.params_publish_batch(slots, p)
            keys = make_keys(rng, b + 1, frames)
            set_keys(ctx, keys)
            src = synth.draw_sources(rng, n, frames)
            mix, peaks = ctx.process_block(src, slots)
            want, rpeaks = r.block(p, src, s, keys)
            _check(mix[0], peaks, want, rpeaks, f"{chain} block {b}")
        assert all(st.rundb.max() > 0 for kind, st in r.stages if kind == "comp")


def test_device_memory_key_is_the_previous_callbacks_out(gas, ob):
    """One of the context's own mixes as a key: the device `out` of block b - 1 goes into key 0 with GAS_MEM_DEVICE, in
    stream order in front of block b, with no synchronisation in between."""
    import torch

    K = gas.capi
    F, n, blocks = 128, 65, 5
    rng = np.random.default_rng(41)
    ctx, slots, p = _ctx(gas, n, F, (COMP,))
    with ctx:
        s = keyed_settings(rng, n, gas, sidechain=np.where(np.arange(n) % 3 == 0, 0, 1))
        s["compressor_threshold_db"] = -40.0
        ctx.fx_dyn_settings_publish(slots, s)
        srcs = [(rng.uniform(-1, 1, (n, F, 2)) * 0.005).astype(np.float32) for _ in range(blocks)]  # -46 dB each
        d_src = [torch.from_numpy(x).cuda() for x in srcs]
        d_out = torch.zeros(blocks, 1, F, 2, device="cuda")
        d_peaks = torch.zeros(blocks, n, 2, device="cuda")
        torch.cuda.synchronize()
        for b in range(blocks):
            if b > 0:
                assert ctx.sidechain_set_raw(0, d_out[b - 1].data_ptr(), K.MEM_DEVICE) == 0
            assert ctx.process_block_raw(d_src[b].data_ptr(), slots if b == 0 else None, n, F, d_out[b].data_ptr(), d_peaks[b].data_ptr(), K.MEM_DEVICE) == 0
        ctx.synchronize()
        outs, pks = d_out.cpu().numpy(), d_peaks.cpu().numpy()
        r = ChainRef(ob, (COMP,), n, F)
        keys = np.zeros((NK, F, 2), np.float32)
        for b in range(blocks):
            if b > 0:
                keys[0] = outs[b - 1][0]  # the same block, fed from the host
            want, rpeaks = r.block(p, srcs[b], s, keys)
            _check(outs[b][0], pks[b], want, rpeaks, f"block {b}")
        keyed = s["compressor_sidechain"][:, 0] != 0
        assert r.comp().rundb[keyed].max() > 0 and (r.comp().rundb[~keyed] == 0).all()  # the mix of 65 sources gets over -40 dB, one source does not


def test_keyed_chains_on_two_buses(gas, ob):
    """gas_process_block_buses runs the chains staged: keyed [COMPRESSOR] to bus 0 or 1 dry and to the other by a send."""
    from godot_audio_spatializer_amd import synth

    F, n = 128, 65
    rng = np.random.default_rng(51)
    ctx, slots, p = _ctx(gas, n, F, (COMP,))
    with ctx:
        s = keyed_settings(rng, n, gas, sidechain=np.arange(n) % 9)
        ctx.fx_dyn_settings_publish(slots, s)
        routes = gas.capi.bus_routes(n)
        routes["dry_bus"] = np.where(np.arange(n) % 3 == 0, 1, 0)
        routes["send_bus"] = np.where(np.arange(n) % 3 == 0, 0, 1)
        routes["send"] = rng.uniform(0, 1, (n, 1, 1)).astype(np.float32) * np.ones((4, 2), np.float32)
        ctx.bus_routes_publish(slots, routes)
        r = ChainRef(ob, (COMP,), n, F)
        for b in range(3):
            keys = make_keys(rng, b + 1, F)
            set_keys(ctx, keys)
            src = synth.draw_sources(rng, n, F)
            out, peaks = ctx.process_block_buses(src, slots, 2)
            y = r.rows(src, s, keys).astype(np.float64)
            for bus in range(2):
                w = (routes["dry_bus"] == bus).astype(np.float64) + (routes["send_bus"] == bus) * routes["send"][:, 0, 0].astype(np.float64)
                want = (y * w[:, None, None]).sum(axis=0)
                assert rel_rms(out[bus, 0], want) <= TOL, f"block {b} bus {bus}"
            np.testing.assert_allclose(peaks, np.abs(y).max(axis=1), rtol=2e-5, atol=1e-7)
        assert r.comp().rundb.max() > 0


def test_keyed_chains_over_device_streams(gas, ob):
    """gas_process_block_streams samples the rows first (tests/stream_window_ref.py), then runs the keyed chain."""
    import stream_window_ref as sw

    F, n = 128, 65
    rng = np.random.default_rng(61)
    ctx, slots, p = _ctx(gas, n, F, (COMP,))
    with ctx:
        s = keyed_settings(rng, n, gas, sidechain=np.arange(n) % 9)
        ctx.fx_dyn_settings_publish(slots, s)
        pbs = []
        for i, slot in enumerate(slots):
            pcm = sw.make_pcm(rng, [200, 300, 5 * F][i % 3], "f32_stereo" if i % 2 else "f32_mono")
            ctx.source_bind_stream(slot, ctx.stream_create(pcm))
            pbs.append(sw.Playback(pcm))
        r = ChainRef(ob, (COMP,), n, F)
        for b in range(4):
            keys = make_keys(rng, b + 1, F)
            set_keys(ctx, keys)
            rows = np.stack([pb.block(F) for pb in pbs])
            mix, peaks, _ = ctx.process_block_streams(slots)
            want, rpeaks = r.block(p, rows, s, keys)
            _check(mix[0], peaks, want, rpeaks, f"block {b}")
        assert r.comp().rundb.max() > 0


def test_errors_change_nothing(gas, ob):
    K = gas.capi
    F, n = 128, 2
    rng = np.random.default_rng(71)
    ctx, slots, p = _ctx(gas, n, F, (COMP,))
    with ctx:
        s = keyed_settings(rng, n, gas, sidechain=1)
        s["compressor_threshold_db"] = -30.0
        ctx.fx_dyn_settings_publish(slots, s)
        r = ChainRef(ob, (COMP,), n, F)
        keys = np.zeros((NK, F, 2), np.float32)
        keys[0] = _tone(0.9, 0, F)[:, None]
        ctx.sidechain_set(0, keys[0])

        def block(what, sl=slots, pp=p, ss=s, rr=r):
            src = rng.uniform(-0.05, 0.05, (len(sl), F, 2)).astype(np.float32)
            mix, peaks = ctx.process_block(src, sl)
            want, rpeaks = rr.block(pp, src, ss, keys)
            _check(mix[0], peaks, want, rpeaks, what)

        block("first block")
        other = np.full((F + 128, 2), 0.001, np.float32)  # would release the compressor if any of the calls took it
        assert ctx.sidechain_set_raw(NK, other.ctypes.data, K.MEM_HOST) == INVALID
        block("after key 8")
        assert ctx.sidechain_set_raw(0, other.ctypes.data, K.MEM_HOST, frames=F + 128) == FRAME_COUNT
        block("after a frame count off by 128")
        assert ctx.sidechain_set_raw(0, other.ctypes.data, 7) == INVALID
        assert ctx.sidechain_set_raw(0, None, 7) == INVALID
        block("after a bad mem")
        with pytest.raises(gas.GasError) as ei:
            ctx.sidechain_set(NK, other[:F])
        assert ei.value.status == INVALID
        # a sidechain of 9 at a position the chain does not use: nothing of the publish is taken
        bad = s.copy()
        bad["compressor_sidechain"][:, 0] = 0
        bad["compressor_threshold_db"] = 0.0
        bad["compressor_sidechain"][1, 3] = NK + 1
        with pytest.raises(gas.GasError) as ei:
            ctx.fx_dyn_settings_publish(slots, bad)
        assert ei.value.status == INVALID
        block("after the refused publish")
        assert r.comp().rundb.min() > 0  # the loud key was heard all along
        # a freed and re-allocated slot starts at the defaults: keyless, although key 0 is still loud
        ctx.source_free(int(slots[1]))
        one = ChainRef(ob, (COMP,), 1, F)
        one.comp().rundb[:] = r.comp().rundb[:1]
        block("one source", sl=slots[:1], pp=p[:1], ss=s[:1], rr=one)
        again = ctx.source_alloc(K.KIND_EFFECT, (COMP,))
        assert again == slots[1]
        ctx.params_publish(again, p[1])
        keys[0] = _tone(4.0, 1, F)[:, None]  # over the default threshold of 0 dB: a slot still keyed would duck
        ctx.sidechain_set(0, keys[0])
        fresh = ChainRef(ob, (COMP,), 1, F)
        block("re-allocated slot", sl=np.array([again], np.uint32), pp=p[1:2], ss=K.fx_dyn_settings_defaults(1), rr=fresh)
        assert fresh.comp().rundb[0] == 0  # -26 dB input under the default threshold of 0 dB: nothing detected


def test_set_between_queued_callbacks_flushes_and_does_not_reorder(gas):
    """GAS_FLAG_PIPELINED_MIX | GAS_FLAG_BATCHED_LAUNCH, depth 4: gas_sidechain_set between queued callbacks runs the
    waiting ones first; every out is bitwise what the same sequence gives without the calls."""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, n, blocks = 128, 2048, 10
    rng = np.random.default_rng(81)
    hrir = synth.synthetic_hrir(rng, dirs=16)
    p = synth.draw_params(rng, n, dirs=16, frames=F)
    srcs = [synth.draw_sources(rng, n, F) for _ in range(blocks)]
    key = rng.uniform(-1, 1, (F, 2)).astype(np.float32)
    results = []
    for interleave in (False, True):
        with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PIPELINED_MIX | K.FLAG_BATCHED_LAUNCH) as ctx:
            ctx.hrtf_load(hrir)
            ctx.set_batch_depth(4)
            slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
            ctx.params_publish_batch(slots, p)
            d_src = [torch.from_numpy(x).cuda() for x in srcs]
            d_out = torch.zeros(blocks, 1, F, 2, device="cuda")
            d_peaks = torch.zeros(blocks, n, 2, device="cuda")
            torch.cuda.synchronize()
            for b in range(blocks):
                assert ctx.process_block_raw(d_src[b].data_ptr(), slots if b == 0 else None, n, F, d_out[b].data_ptr(), d_peaks[b].data_ptr(), K.MEM_DEVICE) == 0
                if interleave and b == 0:
                    ctx.sidechain_set(3, key)  # one callback waiting
                if interleave and b == 2:
                    ctx.sidechain_set(0, None)  # two waiting
                if interleave and b == 5:
                    assert ctx.sidechain_set_raw(1, d_out[4].data_ptr(), K.MEM_DEVICE) == 0  # an earlier out, still a pending sum
                if interleave and b == 6:
                    ctx.sidechain_set(7, key)
            ctx.synchronize()
            results.append((d_out.cpu().numpy(), d_peaks.cpu().numpy()))
    assert np.abs(results[0][0]).max() > 0
    np.testing.assert_array_equal(results[0][0], results[1][0])
    np.testing.assert_array_equal(results[0][1], results[1][1])


def test_host_layer_sets_a_key_before_the_mix(gas):
    """gas_host_set_sidechain, then gas_host_get_mixed_frames, on a [COMPRESSOR] host with a keyless and a keyed playback:
    the reference applied to the windows the same host delivers for an empty chain, one playback at a time."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, cbs = 128, 6
    rng = np.random.default_rng(91)
    streams = [rng.uniform(-0.01, 0.01, (F * 12, 2)).astype(np.float32) for _ in range(2)]  # -40 dB: under the threshold
    params = synth.draw_params(rng, 2, dirs=8, frames=F)
    s = keyed_settings(rng, 2, gas, sidechain=[0, 3], edges=False)
    s["compressor_threshold_db"] = -30.0
    keys = [make_keys(rng, cb, F)[0 if cb == 2 else 7] for cb in range(cbs)]  # noise of moving level, once the loud tone

    def run(chain, which):
        with gas.SpatializerContext(max_sources=4, frames=F) as ctx:
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, chain)
            for i in which:
                pid = host.start_playback_array(streams[i])
                host.set_spatializer_parameters(pid, params[i])
                if chain:
                    assert host.set_effect_dyn_settings(pid, s[i : i + 1]) == 0
            outs = []
            for cb in range(cbs):
                if chain and cb != 4:  # callback 4 detects on callback 3's key again
                    assert host.set_sidechain(2, keys[cb]) == 0
                rc, out = host.get_mixed_frames(0, F)
                assert rc == 0
                outs.append(out.copy())
            if chain:
                assert host.set_sidechain(NK, keys[0]) == INVALID and host.set_sidechain(0, keys[0][:64]) == FRAME_COUNT
            host.close()
        return np.stack(outs)

    windows = np.stack([run((), [0]), run((), [1])])  # [2][cbs][F][2]
    got = run((COMP,), [0, 1])
    stage = sc.KeyedStage(0, 2)
    held = np.zeros((NK, F, 2), np.float32)
    for cb in range(cbs):
        if cb != 4:
            held[2] = keys[cb]
        y = stage.block(windows[:, cb], held, s)
        want = y.astype(np.float64).sum(axis=0)
        assert rel_rms(got[cb], want) <= TOL, f"callback {cb}: {rel_rms(got[cb], want)}"
    assert stage.rundb[1] > 0 and stage.rundb[0] == 0
