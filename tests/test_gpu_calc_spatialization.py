"""batched parameter generation on the device vs the oracle's restatement of
calculate_spatialization's arithmetic (audio_spatializer_3d.cpp:103-151, 277-479, 903-938)."""
import numpy as np
import pytest

import calc_spat_ref

pytestmark = pytest.mark.gpu


def random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float32)


def scene(gas, rng, n, n_listeners, n_cfgs):
    K = gas.capi
    cfgs = K.default_spat3d_config(n_cfgs)
    for i in range(n_cfgs):
        cfgs["attenuation_model"][i] = i % 4
        cfgs["speaker_mode"][i] = (i // 4) % 4
        cfgs["max_distance"][i] = [0.0, 60.0, 25.0][i % 3]
        cfgs["emission_angle_enabled"][i] = (i // 2) % 2
        cfgs["emission_angle"][i] = 30.0 + 10.0 * (i % 5)
        cfgs["doppler_tracking"][i] = (i // 3) % 2
        cfgs["panning_strength"][i] = [1.0, 0.5, 2.0][i % 3]
        cfgs["unit_size"][i] = [10.0, 4.0][i % 2]
        cfgs["attenuation_filter_db"][i] = [-24.0, -12.0][(i // 2) % 2]
    cfgs["hrtf_n_az"] = 32
    cfgs["hrtf_n_el"] = 9
    poses = np.zeros(n, K.POSE_DTYPE)
    d = np.exp(rng.uniform(np.log(0.5), np.log(120.0), n))
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    poses["position"] = (u * d[:, None]).astype(np.float32)
    poses["velocity"] = rng.uniform(-30, 30, (n, 3))
    poses["velocity"][::5] = 0
    fw = rng.standard_normal((n, 3))
    poses["forward"] = fw / np.linalg.norm(fw, axis=1, keepdims=True)
    # (32 of the sources get an emission cone exactly on listener 0's axis below: the dot product can land 1 ulp outside
    # [-1, 1] there; [ENGINE] Math::acos clamps, audio_spatializer_3d.cpp:378-385)
    poses["volume_db"] = rng.uniform(-12, 6, n)
    poses["max_db"] = 3.0
    poses["pitch_scale"] = rng.uniform(0.5, 2.0, n)
    listeners = np.zeros(n_listeners, K.LISTENER_DTYPE)
    for i in range(n_listeners):
        listeners["basis"][i] = random_rotation(rng)
        listeners["origin"][i] = rng.uniform(-5, 5, 3)
        listeners["velocity"][i] = rng.uniform(-3, 3, 3)
    for k, i in enumerate(range(0, min(n, 64), 2)):  # now exactly on listener 0's axis
        rel = poses["position"][i] - listeners["origin"][0]
        poses["forward"][i] = (rel / max(np.linalg.norm(rel), 1e-12) * (1.0 if k % 2 else -1.0)).astype(np.float32)
    cfg_index = rng.integers(0, n_cfgs, n).astype(np.uint32)
    return cfgs, poses, listeners, cfg_index


@pytest.mark.parametrize("n_listeners", [1, 3])
def test_calc_spatialization_matches_oracle(gas, ob, n_listeners):
    rng = np.random.default_rng(21)
    n, n_cfgs = 4000, 24
    cfgs, poses, listeners, cfg_index = scene(gas, rng, n, n_listeners, n_cfgs)
    with gas.SpatializerContext(max_sources=n, frames=512, channel_count=4) as ctx:
        slots = ctx.source_alloc_many(n, gas.capi.KIND_3D_MIX)
        was_further = np.zeros(n, np.int32)
        for tick in range(3):  # the update_parameters latch needs history (audio_spatializer_3d.cpp:472-479)
            if tick == 1:
                poses["position"] *= 3.0  # many sources leave max_distance
            got = ctx.calc_spatialization(cfgs, poses, listeners, slots, cfg_index=cfg_index)
            want = np.zeros(n, ob.PARAMS_DTYPE)
            ob.calc_spatialization(cfgs, cfg_index, poses, listeners, was_further, want)
            ok = np.isfinite(want["mix_volumes"]).all(axis=(1, 2))  # SPCAP with an un-normalised direction can go NaN (reference quirk)
            assert ok.mean() > 0.6
            np.testing.assert_array_equal(np.isfinite(got["mix_volumes"]).all(axis=(1, 2)), ok)
            np.testing.assert_allclose(got["mix_volumes"][ok], want["mix_volumes"][ok], rtol=3e-5, atol=1e-7)
            np.testing.assert_allclose(got["pitch_scale"], want["pitch_scale"], rtol=3e-5)
            np.testing.assert_allclose(got["linear_attenuation"], want["linear_attenuation"], rtol=3e-5, atol=1e-8)
            np.testing.assert_array_equal(got["attenuation_filter_cutoff_hz"], want["attenuation_filter_cutoff_hz"])
            np.testing.assert_array_equal(got["update_parameters"], want["update_parameters"])
            np.testing.assert_allclose(got["hrtf_gain"], want["hrtf_gain"], rtol=3e-5, atol=1e-8)
            differ = got["hrtf_dir"] != want["hrtf_dir"]
            assert differ.mean() < 1e-3  # grid-cell boundaries may round differently ...
            # ... and nowhere else: the float64 reference puts every such row within 1e-4 grid units of a rounding border
            margins = calc_spat_ref.calc(cfgs, cfg_index, poses, listeners, np.zeros(n, np.int32))["margins"]  # (the direction does not depend on the latch)
            assert calc_spat_ref.on_grid_border(margins)[differ].all()
            assert got["hrtf_dir"].max() < 32 * 9


@pytest.mark.parametrize("n_listeners", [1, 3])
def test_calc_spatialization_area_branches_match_oracle(gas, ob, n_listeners):
    """sources inside Area3Ds with a reverb send.  The closest area point per listener widens or
    vetoes the max-distance test (audio_spatializer_3d.cpp:364-370) and calc_reverb_vol (:154-197) yields the
    reverb-bus volumes, max-combined over the listeners (:399-402); every speaker mode, uniformity 0 and > 0."""
    K = gas.capi
    rng = np.random.default_rng(77)
    n, n_cfgs = 3000, 24
    cfgs, poses, listeners, cfg_index = scene(gas, rng, n, n_listeners, n_cfgs)
    cfgs["panning_strength"] = 1.0  # keeps SPCAP finite for most directions
    areas = np.zeros(n, K.AREA_SEND_DTYPE)
    areas["present"] = rng.random(n) < 0.8
    areas["using_reverb_bus"] = rng.random(n) < 0.7
    areas["reverb_uniformity"] = np.where(rng.random(n) < 0.4, 0.0, rng.uniform(0.05, 1.0, n))
    areas["reverb_amount"] = rng.uniform(0.0, 1.0, n)
    lap = (rng.standard_normal((n, n_listeners, 3)) * np.exp(rng.uniform(np.log(0.2), np.log(90.0), (n, n_listeners, 1)))).astype(np.float32)
    lap[::11] = 0.0  # the listener stands inside the area
    with gas.SpatializerContext(max_sources=n, frames=512, channel_count=4) as ctx:
        slots = ctx.source_alloc_many(n, K.KIND_3D_MIX)
        was_further = np.zeros(n, np.int32)
        for tick in range(2):
            if tick == 1:
                poses["position"] *= 2.0
            got, rev = ctx.calc_spatialization_areas(cfgs, poses, listeners, slots, areas, lap, cfg_index=cfg_index)
            want = np.zeros(n, ob.PARAMS_DTYPE)
            in_range, wrev = ob.calc_spatialization_areas(cfgs, cfg_index, poses, listeners, was_further, areas, lap, want)
            ok = np.isfinite(want["mix_volumes"]).all(axis=(1, 2)) & np.isfinite(wrev).all(axis=(1, 2))
            assert ok.mean() > 0.6
            np.testing.assert_array_equal(np.isfinite(got["mix_volumes"]).all(axis=(1, 2)) & np.isfinite(rev).all(axis=(1, 2)), ok)
            np.testing.assert_allclose(got["mix_volumes"][ok], want["mix_volumes"][ok], rtol=3e-5, atol=1e-7)
            np.testing.assert_allclose(rev[ok], wrev[ok], rtol=5e-5, atol=1e-7)
            np.testing.assert_array_equal(got["update_parameters"], want["update_parameters"])
            np.testing.assert_allclose(got["linear_attenuation"], want["linear_attenuation"], rtol=3e-5, atol=1e-8)
            # the branches are all taken: areas that veto a listener, areas that send, sources without an area
            sending = (areas["present"] != 0) & (areas["using_reverb_bus"] != 0)
            assert (np.abs(wrev[sending & ok]).max(axis=(1, 2)) > 0).mean() > 0.2
            assert not np.abs(wrev[~sending]).any() and not np.abs(rev[~sending]).any()
        # without areas the new entry is the old one
        plain = ctx.calc_spatialization(cfgs, poses, listeners, slots, cfg_index=cfg_index)
        same, zero = ctx.calc_spatialization_areas(cfgs, poses, listeners, slots, np.zeros(n, K.AREA_SEND_DTYPE), None, cfg_index=cfg_index)
        assert plain.tobytes() == same.tobytes() and not zero.any()


def test_generated_parameters_drive_the_mix(gas, ob):
    """The parameters the device generated are the ones the next callback mixes with (no host publish)."""
    from godot_audio_spatializer_amd import synth
    from helpers import TOL, rel_rms

    rng = np.random.default_rng(5)
    n = 200
    cfgs, poses, listeners, _ = scene(gas, rng, n, 1, 1)
    cfgs["speaker_mode"] = 0
    cfgs["attenuation_model"] = 0
    with gas.SpatializerContext(max_sources=n, frames=512) as ctx:
        slots = ctx.source_alloc_many(n, gas.capi.KIND_3D_MIX)
        p = ctx.calc_spatialization(cfgs, poses, listeners, slots)
        src = synth.draw_sources(rng, n, 512)
        mix, _ = ctx.process_block(src, slots)
        ora = ob.BatchOracle(ob.KIND_3D_MIX, n, 512)
        _, _, r64 = ora.block(p.astype(ob.PARAMS_DTYPE), src, want64=True)
        assert rel_rms(mix[0], r64[0]) <= TOL


def test_calc_spatialization_argument_checks(gas):
    K = gas.capi
    with gas.SpatializerContext(max_sources=4, frames=512) as ctx:
        slots = ctx.source_alloc_many(2, K.KIND_3D_MIX)
        cfg = K.default_spat3d_config(1)
        poses = np.zeros(2, K.POSE_DTYPE)
        lis = np.zeros(1, K.LISTENER_DTYPE)
        bad = cfg.copy()
        bad["speaker_mode"] = 9
        with pytest.raises(gas.GasError):
            ctx.calc_spatialization(bad, poses, lis, slots)
        with pytest.raises(gas.GasError):
            ctx.calc_spatialization(cfg, poses, lis, np.array([0, 3], np.uint32))  # slot 3 not allocated
        with pytest.raises(gas.GasError):
            ctx.calc_spatialization(cfg, poses, lis, slots, cfg_index=np.array([0, 1], np.uint32))
