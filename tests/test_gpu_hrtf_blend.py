"""GAS_FLAG_HRTF_INTERPOLATE on the GPU: every HRTF stage convolves with a blend of up to four HRIR rows
(k_hrtf_ols_blend / k_hrtf_rows_blend), against the composed reference of hrtf_blend_ref.py -- the weighted sum of the
oracle's single-direction renders, whose premise test_hrtf_blend_reference.py checks on the CPU."""
import numpy as np
import pytest

import hrtf_blend_ref as ref
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

ER, HRTF, AMPLIFY = 2, 3, 9
BAD_ARG = -1
DIRS = 32
PEAK_TOL = dict(rtol=2e-5, atol=1e-7)  # test_gpu_fx_stereo.py's bounds for peaks


def _hrir(dirs=DIRS, seed=5):
    from godot_audio_spatializer_amd import synth

    return synth.synthetic_hrir(np.random.default_rng(seed), dirs=dirs)


def run_blend(gas, ob, chain, n, F, blocks, seed, flags=0, draining=(), blends_of=None, check=True, amp_db=None, mix_only=False, blend_slots=True):
    """`blocks` callbacks of n sources of one chain on a flagged context, blends re-published every block, each block
    checked against the composed reference.  Returns the mixes [blocks][F][2] (and the peaks)."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    rng = np.random.default_rng(seed)
    hrir = _hrir()
    ring = 4096 if ER in chain else 0
    mixes, all_peaks = [], []
    with gas.SpatializerContext(max_sources=n, frames=F, er_ring_frames=ring, flags=K.FLAG_HRTF_INTERPOLATE | flags) as ctx:
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
        for s in draining:
            ctx.source_set_draining(int(slots[s]), True)
        composed = ref.BlendReference(ob, n, F, chain, hrir) if check else None
        if amp_db is not None:
            j = chain.index(AMPLIFY)
            fx = ctx.fx_settings_defaults(n)
            fx["amplify_volume_db"][:, j] = amp_db
            ctx.fx_settings_publish(slots, fx)
            for s in range(n):
                for o in composed.oracles[s]:
                    o.set_fx_settings(0, j, volume_db=amp_db)
        for b in range(blocks):
            p = synth.draw_params(rng, n, dirs=DIRS, frames=F)
            blends = blends_of(rng, b, p) if blends_of else synth.draw_blends(rng, n, DIRS)
            ctx.params_publish_batch(slots, p)
            if blend_slots:
                ctx.publish_hrtf_blend(slots, blends)
            src = synth.draw_sources(rng, n, F)
            mix, peaks = ctx.process_block(src, slots)
            mixes.append(mix[0])
            all_peaks.append(peaks)
            if check:
                rows, rpeaks, want = composed.block(p, blends, src)
                err = rel_rms(mix[0], want)
                print(f"chain {chain} F {F} n {n} block {b}: mix rel rms {err:.3e}")
                assert err <= TOL, f"block {b}: {err}"
                if mix_only:
                    continue
                pk = np.ones(n, bool)
                if flags & K.FLAG_PEAKS_DRAINING_ONLY:
                    pk[:] = False
                    pk[list(draining)] = True
                    assert np.all(np.isposinf(peaks[~pk])), f"block {b}"
                np.testing.assert_allclose(peaks[pk], rpeaks[pk], err_msg=f"block {b}", **PEAK_TOL)
    return np.stack(mixes), np.stack(all_peaks)


@pytest.mark.parametrize("F", [512, 128])
def test_plain_hrtf_exact_peaks(gas, ob, F):
    run_blend(gas, ob, (HRTF,), 24, F, 4, seed=F)


@pytest.mark.parametrize("F", [512, 128])
def test_plain_hrtf_peaks_of_draining_sources_only(gas, ob, F):
    """The frequency-domain form (one forward transform per source, the blend applied to the spectral product) and the
    exact-peak form in one launch."""
    run_blend(gas, ob, (HRTF,), 24, F, 4, seed=F + 1, flags=gas.capi.FLAG_PEAKS_DRAINING_ONLY, draining=range(0, 24, 2))


def test_er_hrtf_at_the_cfg5_shape(gas, ob):
    run_blend(gas, ob, (ER, HRTF), 8, 256, 4, seed=3)
    run_blend(gas, ob, (ER, HRTF), 8, 256, 4, seed=4, flags=gas.capi.FLAG_PEAKS_DRAINING_ONLY, draining=(1, 6))


@pytest.mark.parametrize("chain", [(AMPLIFY, HRTF), (HRTF, AMPLIFY)])
def test_staged_chains(gas, ob, chain):
    """The HRTF as the last stage and mid-chain (gas_launch_hrtf_rows), the amplifier off its default."""
    run_blend(gas, ob, chain, 24, 512, 4, seed=5, amp_db=-4.5)


def test_the_all_zero_row_is_the_one_row_blend(gas, ob):
    """A flagged context whose slots never got a blend row and one whose blends are {hrtf_dir, 1, 0, 0, 0}: the same code
    path, bitwise equal; both within TOL of the unflagged context (another kernel, so not bitwise)."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F, blocks, seed = 24, 512, 4, 9
    for flags in (0, K.FLAG_PEAKS_DRAINING_ONLY):
        dr = range(0, n, 3) if flags else ()
        never, pk_never = run_blend(gas, ob, (HRTF,), n, F, blocks, seed, flags=flags, draining=dr, blends_of=lambda rng, b, p: np.zeros(n, K.HRTF_BLEND_DTYPE), blend_slots=False)
        explicit, pk_explicit = run_blend(gas, ob, (HRTF,), n, F, blocks, seed, flags=flags, draining=dr, blends_of=lambda rng, b, p: ref.one_row(p["hrtf_dir"]), check=False)
        np.testing.assert_array_equal(never, explicit)
        np.testing.assert_array_equal(pk_never, pk_explicit)
        rng = np.random.default_rng(seed)
        with gas.SpatializerContext(max_sources=n, frames=F, flags=flags) as ctx:
            ctx.hrtf_load(_hrir())
            slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
            for s in dr:
                ctx.source_set_draining(int(slots[s]), True)
            for b in range(blocks):
                p = synth.draw_params(rng, n, dirs=DIRS, frames=F)
                ctx.params_publish_batch(slots, p)
                mix, peaks = ctx.process_block(synth.draw_sources(rng, n, F), slots)
                assert rel_rms(never[b], mix[0]) <= TOL, b
                np.testing.assert_allclose(pk_never[b], peaks, **PEAK_TOL)


def test_blocks_carry_state_under_changing_blends(gas, ob):
    """F = 128: the 256 taps span two blocks of history, so a history bug shows by block 3; new directions every block."""
    run_blend(gas, ob, (HRTF,), 24, 128, 6, seed=13)
    run_blend(gas, ob, (HRTF,), 24, 128, 6, seed=14, flags=gas.capi.FLAG_PEAKS_DRAINING_ONLY, draining=(0, 5))


def test_one_source_half_and_half(gas):
    """The smallest case: weights (0.5, 0.5, 0, 0) on two directions against the mean of two single-direction renders on
    unflagged contexts (hrtf_dir alone, the kernels that existed before)."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F = 512
    outs = {}
    for name, d, w in (("both", (3, 17, 0, 0), (0.5, 0.5, 0, 0)), ("a", (3, 0, 0, 0), (1, 0, 0, 0)), ("b", (17, 0, 0, 0), (1, 0, 0, 0))):
        rng = np.random.default_rng(2)
        with gas.SpatializerContext(max_sources=1, frames=F, flags=K.FLAG_HRTF_INTERPOLATE if name == "both" else 0) as ctx:
            ctx.hrtf_load(_hrir())
            slots = ctx.source_alloc_many(1, K.KIND_EFFECT, (HRTF,))
            if name == "both":
                blend = np.zeros(1, K.HRTF_BLEND_DTYPE)
                blend["dir"][0], blend["weight"][0] = d, w
                ctx.publish_hrtf_blend(slots, blend)
            got = []
            for b in range(3):
                p = synth.draw_params(rng, 1, dirs=DIRS)
                p["hrtf_dir"] = d[0]
                ctx.params_publish_batch(slots, p)
                got.append(ctx.process_block(synth.draw_sources(rng, 1, F), slots)[0][0])
            outs[name] = np.stack(got).astype(np.float64)
    want = 0.5 * (outs["a"] + outs["b"])
    assert rel_rms(outs["both"], want) <= TOL
    assert rel_rms(outs["a"], want) > 0.1  # the two directions differ: the blend is not either of them


def test_more_than_one_workgroup(gas, ob):
    """2049 sources at F = 128 (the composed reference costs four oracles per source): several workgroups, several
    sources per wave, the partial-mix reduction.  Mix only."""
    run_blend(gas, ob, (HRTF,), 2049, 128, 1, seed=21, flags=gas.capi.FLAG_PEAKS_DRAINING_ONLY, draining=range(0, 2049, 64), mix_only=True)


def _pose_at(az, el, r=2.0):
    return np.array([r * np.cos(el) * np.sin(az), r * np.sin(el), -r * np.cos(el) * np.cos(az)], np.float32)


def test_calc_spatialization_writes_the_bilinear_row(gas):
    """No read-back of blend rows exists, so the weights are read through the audio: after one silent block (the previous
    gain is then the gain), an impulse renders gain x sum_i w_i hrir[dir_i]; least squares over the numpy rule's four
    corner HRIRs gives the weights the kernel used.  Bound 1e-6 absolute: the weights are f32 roundings of f64 values
    (6e-8), the f32 render adds about 1e-7 of the peak tap."""
    K = gas.capi
    n_az, n_el, F = 8, 5, 128
    dirs = n_az * n_el
    hrir = _hrir(dirs=dirs, seed=8)
    caz, cel = 2 * np.pi / n_az, np.pi / (n_el - 1)
    cases = [
        ("centre front", 0.0, 0.0),
        ("centre right", np.pi / 2, 0.0),
        ("centre behind", np.pi, 0.0),
        ("37% / 62%", (1 + 0.37) * caz, -np.pi / 2 + (2 + 0.62) * cel),
        ("62% / 37%", (5 + 0.62) * caz - 2 * np.pi, -np.pi / 2 + (0 + 0.37) * cel),
        ("azimuth wrap", (n_az - 1 + 0.37) * caz, -np.pi / 2 + (1 + 0.62) * cel),
        ("azimuth wrap, negative angle", -0.3 * caz, 0.1),
        ("top row", 2.37 * caz, np.pi / 2),
        ("bottom row", 4.62 * caz, -np.pi / 2),
    ]
    n = len(cases)
    poses = np.zeros(n, K.POSE_DTYPE)
    for i, (_, az, el) in enumerate(cases):
        poses["position"][i] = _pose_at(az, el)
        if cases[i][0].startswith("centre"):  # exactly on the axis: sin(pi) and cos(pi / 2) are not 0 in floating point
            poses["position"][i][np.abs(poses["position"][i]) < 1e-6] = 0.0
    poses["forward"][:, 2] = 1.0
    poses["pitch_scale"] = 1.0
    poses["max_db"] = 3.0
    cfgs = K.default_spat3d_config(1)
    cfgs["hrtf_n_az"], cfgs["hrtf_n_el"] = n_az, n_el
    listeners = np.zeros(1, K.LISTENER_DTYPE)
    listeners["basis"][0] = np.eye(3, dtype=np.float32)
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_HRTF_INTERPOLATE) as ctx:
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
        ctx.publish_hrtf_blend(slots, ref.one_row(np.full(n, 7)))  # an earlier publish: the launch's rows replace it
        params = ctx.calc_spatialization(cfgs, poses, listeners, slots)
        assert (params["hrtf_gain"] > 0).all()
        impulse = np.zeros((1, F, 2), np.float32)
        impulse[0, 0] = 1.0
        for i, (name, _, _) in enumerate(cases):
            x, y, z = (float(v) for v in poses["position"][i])  # the direction the kernel sees: from the f32 position
            az, el = np.arctan2(x, -z), np.arctan2(y, np.hypot(x, z))
            d, w = ref.bilinear_blend(az, el, n_az, n_el)
            ctx.process_block(np.zeros((1, F, 2), np.float32), slots[i : i + 1])
            out = np.concatenate([ctx.process_block(impulse if b == 0 else 0 * impulse, slots[i : i + 1])[0][0] for b in range(2)])  # 256 taps
            cells = sorted(set(int(c) for c in d))
            A = np.stack([np.concatenate([hrir[c, 0], hrir[c, 1]]).astype(np.float64) for c in cells], axis=1) * float(params["hrtf_gain"][i])
            est, res, _, _ = np.linalg.lstsq(A, np.concatenate([out[:, 0], out[:, 1]]).astype(np.float64), rcond=None)
            want = np.array([w[d == c].sum() for c in cells])
            print(f"{name}: cells {cells} weights {est} want {want}")
            np.testing.assert_allclose(est, want, atol=1e-6, err_msg=name)
            assert np.abs(A @ est - np.concatenate([out[:, 0], out[:, 1]])).max() <= 1e-6, name  # nothing outside the four corners
            if name.startswith("centre"):
                k = int(np.argmax(want))
                assert want[k] > 1 - 1e-9 and cells[k] == int(params["hrtf_dir"][i]), name
            if name in ("top row", "bottom row"):
                assert (want > 1e-6).sum() == 2 and all(c // n_az == (n_el - 1 if name == "top row" else 0) for c, x in zip(cells, want) if x > 1e-6)
        # a later publish replaces the launch's row
        ctx.publish_hrtf_blend(slots[:1], ref.one_row([9]))
        ctx.process_block(np.zeros((1, F, 2), np.float32), slots[:1])
        out = np.concatenate([ctx.process_block(impulse if b == 0 else 0 * impulse, slots[:1])[0][0] for b in range(2)])
        np.testing.assert_allclose(out[:, 0], hrir[9, 0] * params["hrtf_gain"][0], atol=1e-6)


def test_refusals(gas):
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, n = 128, 4
    rng = np.random.default_rng(1)
    good = synth.draw_blends(rng, n, DIRS)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:  # no flag: no blend table
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
        with pytest.raises(gas.GasError) as e:
            ctx.publish_hrtf_blend(slots, good)
        assert e.value.status == BAD_ARG
    for other in (K.FLAG_HRTF_CROSSFADE, K.FLAG_DIRECTION_RUNS, K.FLAG_DIRECTION_ORDER, K.FLAG_XCD_ORDER):
        with pytest.raises(gas.GasError) as e:
            gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_HRTF_INTERPOLATE | other)
        assert e.value.status == BAD_ARG, other
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_HRTF_INTERPOLATE) as ctx:
        ctx.hrtf_load(_hrir())
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
        p = synth.draw_params(rng, n, dirs=DIRS, frames=F)
        ctx.params_publish_batch(slots, p)
        ctx.publish_hrtf_blend(slots, good)
        src = synth.draw_sources(rng, n, F)
        for field, value in (("weight", -0.25), ("weight", np.nan), ("weight", np.inf), ("dir", DIRS)):
            bad = synth.draw_blends(rng, n, DIRS)  # other rows than `good`: taking any of them would show
            k = int(np.flatnonzero(bad["weight"][n - 1])[0])
            bad[field][n - 1, k] = value
            with pytest.raises(gas.GasError) as e:
                ctx.publish_hrtf_blend(slots, bad)
            assert e.value.status == BAD_ARG, (field, value)
        ok = good.copy()  # a direction beyond the set on an entry of weight 0 is not read
        k = int(np.flatnonzero(ok["weight"][0] == 0)[0]) if (ok["weight"][0] == 0).any() else None
        if k is not None:
            ok["dir"][0, k] = 1 << 30
        ctx.publish_hrtf_blend(slots, ok)
        got = ctx.process_block(src, slots)[0]
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_HRTF_INTERPOLATE) as ctx:  # the previous settings' render
        ctx.hrtf_load(_hrir())
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
        ctx.params_publish_batch(slots, p)
        ctx.publish_hrtf_blend(slots, good)
        np.testing.assert_array_equal(ctx.process_block(src, slots)[0], got)  # a refused call took nothing


def test_freed_slot_starts_without_a_blend(gas):
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F = 128
    rng = np.random.default_rng(6)
    p = synth.draw_params(rng, 1, dirs=DIRS, frames=F)
    src = synth.draw_sources(rng, 1, F)
    with gas.SpatializerContext(max_sources=1, frames=F, flags=K.FLAG_HRTF_INTERPOLATE) as ctx:
        ctx.hrtf_load(_hrir())
        s = ctx.source_alloc(K.KIND_EFFECT, (HRTF,))
        ctx.params_publish(s, p[0])
        fresh = ctx.process_block(src, [s])[0]
        ctx.source_reset(s)
        b = np.zeros(1, K.HRTF_BLEND_DTYPE)
        b["dir"][0, 1], b["weight"][0, 1] = (int(p["hrtf_dir"][0]) + 5) % DIRS, 0.8
        ctx.publish_hrtf_blend([s], b)
        blended = ctx.process_block(src, [s])[0]
        assert rel_rms(blended, fresh) > 0.1
        ctx.source_reset(s)  # zeroes the DSP state, keeps the blend
        np.testing.assert_array_equal(ctx.process_block(src, [s])[0], blended)
        ctx.source_free(s)
        ctx.process_block(np.zeros((0, F, 2), np.float32), [])  # the block boundary
        s2 = ctx.source_alloc(K.KIND_EFFECT, (HRTF,))
        assert s2 == s
        ctx.params_publish(s2, p[0])
        np.testing.assert_array_equal(ctx.process_block(src, [s2])[0], fresh)


def test_streams(gas, ob):
    """gas_process_block_streams, 8 PCM sources, F = 512: the stream-sampling form of the kernel.  The streams outlast the
    test, so the window of block b is the stream delayed by the 64-frame lookahead (zeros in front of its start)."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F, blocks = 8, 512, 4
    rng = np.random.default_rng(17)
    hrir = _hrir()
    length = F * blocks + 256
    pcms = [(rng.uniform(-0.5, 0.5, length if i % 3 else (length, 2)) * (32767 if i % 2 else 1)).astype(np.int16 if i % 2 else np.float32) for i in range(n)]
    floats = []
    for a in pcms:
        f = a.astype(np.float32) / np.float32(32768.0) if a.dtype == np.int16 else a
        floats.append(np.concatenate([np.zeros((64, 2), np.float32), np.stack([f, f], axis=1) if f.ndim == 1 else f]))
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_HRTF_INTERPOLATE | K.FLAG_PEAKS_DRAINING_ONLY) as ctx:
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
        for s, a in zip(slots, pcms):
            ctx.source_bind_stream(s, ctx.stream_create(a))
        composed = ref.BlendReference(ob, n, F, (HRTF,), hrir)
        for b in range(blocks):
            p = synth.draw_params(rng, n, dirs=DIRS)
            blends = synth.draw_blends(rng, n, DIRS)
            ctx.params_publish_batch(slots, p)
            ctx.publish_hrtf_blend(slots, blends)
            got, peaks, hf = ctx.process_block_streams(slots)
            src = np.stack([f[b * F : (b + 1) * F] for f in floats])
            _, _, want = composed.block(p, blends, src)
            assert hf.all() and np.all(np.isposinf(peaks))
            assert rel_rms(got[0], want) <= TOL, b


def test_two_buses(gas, ob):
    """gas_process_block_buses over [HRTF] sources: on a flagged context the chains run staged (k_hrtf_rows_blend), the
    rows are mixed per bus with the dry weight and send[0]."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    n, F, n_buses = 24, 512, 2
    rng = np.random.default_rng(19)
    hrir = _hrir()
    routes = K.bus_routes(n)
    routes["dry_bus"] = rng.integers(0, n_buses, n)
    routes["send_bus"] = np.where(rng.uniform(size=n) < 0.7, rng.integers(0, n_buses, n), K.BUS_NONE)
    routes["send"][:, 0, :] = rng.uniform(0.0, 1.2, (n, 2)).astype(np.float32)
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_HRTF_INTERPOLATE) as ctx:
        ctx.hrtf_load(hrir)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
        ctx.bus_routes_publish(slots, routes)
        composed = ref.BlendReference(ob, n, F, (HRTF,), hrir)
        for b in range(3):
            p = synth.draw_params(rng, n, dirs=DIRS)
            blends = synth.draw_blends(rng, n, DIRS)
            ctx.params_publish_batch(slots, p)
            ctx.publish_hrtf_blend(slots, blends)
            src = synth.draw_sources(rng, n, F)
            got, peaks = ctx.process_block_buses(src, slots, n_buses)
            rows, rpeaks, _ = composed.block(p, blends, src)
            np.testing.assert_allclose(peaks, rpeaks, **PEAK_TOL)
            for bus in range(n_buses):
                for ear in range(2):
                    w = (routes["dry_bus"] == bus) + np.where(routes["send_bus"] == bus, routes["send"][:, 0, ear].astype(np.float64), 0.0)
                    assert rel_rms(got[bus, 0, :, ear], (rows[:, :, ear] * w[:, None]).sum(axis=0)) <= TOL, (b, bus, ear)


def test_host_layer_setter(gas):
    """BatchedSpatializerHost + gas_host_set_hrtf_blend: a two-row blend equals the weighted sum of what the same host
    renders with each row alone (same context type, fresh contexts)."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F = 256
    rng = np.random.default_rng(23)
    stream = rng.uniform(-0.8, 0.8, (F * 10, 2)).astype(np.float32)
    params = synth.draw_params(rng, 1, dirs=DIRS, frames=F)
    rows = {"both": ((4, 0, 21, 0), (0.3, 0, 0.6, 0)), "a": ((4, 0, 0, 0), (1, 0, 0, 0)), "b": ((21, 0, 0, 0), (1, 0, 0, 0)), "none": None}
    got = {}
    for name, row in rows.items():
        with gas.SpatializerContext(max_sources=4, frames=F, flags=K.FLAG_HRTF_INTERPOLATE) as ctx:
            ctx.hrtf_load(_hrir())
            host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, (HRTF,))
            pid = host.start_playback_array(stream)
            host.set_spatializer_parameters(pid, params[0])
            if row:
                b = np.zeros(1, K.HRTF_BLEND_DTYPE)
                b["dir"][0], b["weight"][0] = row
                assert host.set_hrtf_blend(pid, b) == 0
                b["weight"][0, 1] = -1.0
                assert host.set_hrtf_blend(pid, b) == BAD_ARG  # refused when queued
            outs = []
            for cb in range(5):
                rc, out = host.get_mixed_frames(0, F)
                assert rc == 0
                outs.append(out.copy())
            host.close()
        got[name] = np.stack(outs).astype(np.float64)
    assert rel_rms(got["both"], 0.3 * got["a"] + 0.6 * got["b"]) <= TOL
    assert rel_rms(got["both"], got["none"]) > 0.1
    with gas.SpatializerContext(max_sources=4, frames=F) as ctx:  # a context without the flag
        host = K.BatchedSpatializerHost(ctx, K.KIND_EFFECT, (HRTF,))
        pid = host.start_playback_array(stream)
        assert host.set_hrtf_blend(pid, np.zeros(1, K.HRTF_BLEND_DTYPE)) == BAD_ARG
        host.close()


def test_two_runs_are_bitwise_equal(gas, ob):
    K = gas.capi
    a = run_blend(gas, ob, (HRTF,), 70, 256, 3, seed=31, flags=K.FLAG_PEAKS_DRAINING_ONLY, draining=(3, 44), check=False)
    b = run_blend(gas, ob, (HRTF,), 70, 256, 3, seed=31, flags=K.FLAG_PEAKS_DRAINING_ONLY, draining=(3, 44), check=False)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
