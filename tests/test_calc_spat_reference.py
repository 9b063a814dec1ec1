"""tests/calc_spat_ref.py pinned to rows worked by hand, and the oracle's gaso_calc_spatialization[_area] pinned to it on
every scene of test_gpu_calc_spat_edges.py: several listeners, rotated bases, Doppler, hrtf_gain / hrtf_dir and
cfg_index included.  This is also where the GPU bounds come from: the oracle's worst deviation from float64 per field
is measured here, printed (pytest -s), and must stay within the figures calc_spat_ref's docstring records; the GPU
bound is four times the recorded figure and never above what the project already grants the kernel.  CPU only."""
import numpy as np
import pytest

import calc_spat_ref as ref
import calc_spat_scenes as sc
from oracle import binding as ob

FIELDS = ("mix_volumes", "reverb", "pitch_scale", "linear_attenuation", "hrtf_gain")


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    ob.build()


def run_oracle(scene, areas=True):
    n = len(scene["poses"])
    was = np.zeros(n, np.int32)
    out = []
    for t in range(len(scene["tick_scale"])):
        p = np.zeros(n, ob.PARAMS_DTYPE)
        if areas:
            in_range, rev = ob.calc_spatialization_areas(scene["cfgs"], scene["cfg_index"], sc.tick_poses(scene, t), scene["listeners"], was, scene["areas"], scene["lap"], p)
        else:
            in_range, rev = ob.calc_spatialization(scene["cfgs"], scene["cfg_index"], sc.tick_poses(scene, t), scene["listeners"], was, p), None
        out.append((p, rev, in_range, was.copy()))
    return out


def test_hand_worked_rows():
    """Four rows written out from the reference's formulas.

    1. Stereo, one identity listener at the origin, source (3, 0, -4): dist 5.  Inverse distance, unit_size 4, volume 0:
       multiplier = 1 / (5/4 + 1e-5) = 0.7999936.  pan_strength = 0.5 * 1: g = 0.25, f = 0.75 / 1.25 = 0.6,
       cos x = 3/5, f cos x = 0.36: (sqrt(0.32), sqrt(0.68)) * multiplier = (0.4525447, 0.6596916).
       db_att = (1 - 0.7999936) * -24 = -4.800154 dB: linear_attenuation 0.5754298.  az = atan2(3, 4) = 36.87 deg:
       36.87 / 360 * 32 = 3.277 -> 3; el = 0 -> row 4 of 9: hrtf_dir = 4 * 32 + 3 = 131, hrtf_gain the multiplier.
    2. 5.1, tightness 2 * 0.5 * 1 = 1, attenuation disabled, source (0, 0, -0.5).  1 + dot = 1.353553 (front pair), 1.5
       (centre), 0.646447 (rear pair).  Effective speakers: front 1 + .5 + .853553 + .5 + 0 = 2.853553, centre
       2 * .853553 + 1 + 2 * .146447 = 3, rear 2.146447.  Gains .5 * base / eff = .237170, .25, .150585; over their
       root sum of squares: 0.5052450, 0.5325772, 0.3207932; LFE 1.
    3. Doppler, attenuation disabled (both weights sqrt(1/2)), source (0, 0, -10) moving at (0, 0, 34.3), listeners at rest
       at the origin (approaching = -1: 343 / 308.7 = 1.111111) and at (0, 0, -20) (approaching = +1: 343 / 377.3 =
       0.909091): pitch = sqrt(1.111111 * 0.909091) = 1.0050378.  With the first listener alone, 1.111111.
    4. The seam behind the listener, 7 x 9 grid: (0, 0, 5) has az = pi, 3.5 cells, rounds away from zero to 4;
       (-0.01, 0, 5) has -3.4978 cells, rounds to -3, and -3 mod 7 = 4 as well; (+0.01, 0, 5) rounds to 3.  el = 0 is
       row 4: hrtf_dir 32, 32, 31.  On a 32 x 9 grid the three are 16.0, -15.99 and 15.99 cells: column 16, 144 all."""
    c = sc.cfg(1, attenuation_model=0, unit_size=4.0)
    r = ref.calc(c, None, sc.poses_at([(3, 0, -4)]), sc.ONE, [0])
    np.testing.assert_allclose(r["mix_volumes"][0, 0], (0.4525447, 0.6596916), rtol=2e-7)
    assert not r["mix_volumes"][0, 1:].any()
    np.testing.assert_allclose([r["linear_attenuation"][0], r["hrtf_gain"][0], r["pitch_scale"][0]], (0.5754298, 0.7999936, 1.0), rtol=2e-7)
    assert r["hrtf_dir"][0] == 131 and r["update_parameters"][0] == 1 and r["attenuation_filter_cutoff_hz"][0] == 5000.0 and r["in_range"][0]

    c = sc.cfg(1, attenuation_model=3, speaker_mode=2)
    r = ref.calc(c, None, sc.poses_at([(0, 0, -0.5)]), sc.ONE, [0])
    np.testing.assert_allclose(r["mix_volumes"][0], [(0.5052450, 0.5052450), (0.5325772, 1.0), (0.3207932, 0.3207932), (0, 0)], rtol=3e-7)
    np.testing.assert_allclose(r["margins"]["spcap"][0], 0.646447, rtol=1e-6)

    c = sc.cfg(1, attenuation_model=3, doppler_tracking=1)
    two = sc.listeners_at((sc.EYE, (0, 0, 0), (0, 0, 0)), (sc.EYE, (0, 0, -20), (0, 0, 0)))
    p = sc.poses_at([(0, 0, -10)], velocity=(0, 0, 34.3))
    np.testing.assert_allclose(ref.calc(c, None, p, two, [0])["pitch_scale"][0], 1.0050378, rtol=2e-7)
    np.testing.assert_allclose(ref.calc(c, None, p, two[:1], [0])["pitch_scale"][0], 1.1111111, rtol=2e-7)

    c = sc.cfg(2, attenuation_model=3)
    c["hrtf_n_az"][0] = 7
    r = ref.calc(c, [0, 0, 0, 1, 1, 1], sc.poses_at([(0, 0, 5), (-0.01, 0, 5), (0.01, 0, 5)] * 2), sc.ONE, np.zeros(6))
    assert r["hrtf_dir"].tolist() == [32, 32, 31, 144, 144, 144]
    assert r["margins"]["az_border"][0] == 0.0 and r["margins"]["az_border"][1] < 3e-3 and r["margins"]["az_border"][4] > 0.48


def test_reference_at_the_hand_placed_edges():
    """What the float64 reference says at the edges test_gpu_calc_spat_edges.py places by hand (the kernel and the oracle
    are compared with it there and below)."""
    e = sc.edge_cases()
    r = sc.run_ref(e["doppler_clamps"])[0]
    np.testing.assert_allclose(r["pitch_scale"], [8.0, 0.125, 343.0 / 743.0, 1.0, 1.0] + [1.5] * 5, rtol=1e-15)
    r = sc.run_ref(e["pan_limits"])[0]
    hard = np.sqrt([0.2, 0.8])  # f = 0.6: sqrt((1 -+ 0.6) / 2)
    m = r["mix_volumes"][:7, 0] / r["hrtf_gain"][:7, None]
    np.testing.assert_allclose(m, [np.sqrt([0.5, 0.5]), hard, hard[::-1], np.sqrt([0.5, 0.5]), np.sqrt([0.5, 0.5]), np.sqrt([0.5 - 0.3 * np.sqrt(0.5), 0.5 + 0.3 * np.sqrt(0.5)]), np.sqrt([0.5 + 0.3 * np.sqrt(0.5), 0.5 - 0.3 * np.sqrt(0.5)])], rtol=1e-12)
    assert np.isfinite(r["mix_volumes"]).all() and (r["mix_volumes"][7:9] < 1e-15).all()  # 3e19: silent, not NaN
    t0, t1 = sc.run_ref(e["max_distance_border"])
    assert t0["in_range"].tolist() == [True, False, True, False, True] and t0["update_parameters"].tolist() == [1] * 5 and t1["update_parameters"].tolist() == [1, 0, 1, 0, 1]
    assert not t0["mix_volumes"][:4].any() and t0["hrtf_gain"][0] == 0.0 and t0["margins"]["dist"][0] == 0.0
    assert sc.run_ref(e["area_veto"])[0]["in_range"].tolist() == [False, True, False]
    r = sc.run_ref(e["cone_border"])[0]
    cut = 10.0 ** (-12.0 / 20.0)
    np.testing.assert_allclose(r["linear_attenuation"], [1.0, cut, 1.0, 1.0, cut], rtol=1e-12)
    assert r["margins"]["cone"][0] == 0.0
    r = sc.run_ref(e["reverb_attenuation_one"])[0]
    assert (r["margins"]["rev_att"][:4] == 0.0).all() and (r["margins"]["rev_att"][4:8] < 0).all() and (r["margins"]["rev_att"][8:] > 0).all()
    r = sc.run_ref(e["equal_multipliers"])[0]
    assert (r["margins"]["mult_gap"] == 0.0).all() and (r["hrtf_dir"] == 131).all()  # the first listener's direction (row 1 above)
    r = sc.run_ref(e["doppler_co_moving"])[0]
    assert not np.allclose(r["pitch_scale"], 1.5)  # the listener at rest hears a shift; the co-moving one adds nothing
    t0, t1 = sc.run_ref(e["no_listeners"])
    for t, upd in ((t0, 1), (t1, 0)):
        assert not t["mix_volumes"].any() and not t["linear_attenuation"].any() and (t["attenuation_filter_cutoff_hz"] == 5000.0).all()
        assert (t["pitch_scale"] == 1.25).all() and not t["hrtf_gain"].any() and t["hrtf_dir"].tolist() == [128, 128, 0] and (t["update_parameters"] == upd).all()


MEASURED = {}


@pytest.mark.parametrize("n_listeners", sc.DENSE_LISTENERS)
@pytest.mark.parametrize("kind", sc.SCENES)
def test_oracle_against_float64_on_every_scene(kind, n_listeners):
    """The oracle against calc_spat_ref on the dense scenes, both ticks, no row left out: NaN patterns equal, integers,
    cutoff, latch and in_range equal, hrtf_dir equal but on a proven rounding border (at most 0.1 % of a scene), and
    every finite value within the figure calc_spat_ref records (a quarter of the GPU bound)."""
    worst = dict.fromkeys(FIELDS, 0.0)
    for n in sc.DENSE_N:
        scene = sc.dense(kind, n, n_listeners)
        assert scene["left"] == 0
        differ = 0
        for t, (want, (got, rev, in_range, was)) in enumerate(zip(sc.run_ref(scene), run_oracle(scene))):
            what = f"{kind} n={n} listeners={n_listeners} tick={t}"
            if kind != "quirk":
                assert np.isfinite(want["mix_volumes"]).all() and np.isfinite(want["reverb"]).all(), what
            if kind == "near":
                assert want["margins"]["spcap"].min() >= ref.GUARD_SPCAP, what
            differ += sc.check(got, rev, want, ref.MEASURED, what)
            np.testing.assert_array_equal(in_range != 0, want["in_range"], err_msg=what)
            np.testing.assert_array_equal(was, want["was_further"], err_msg=what)
            for f, d in sc.deviation(got, rev, want).items():
                worst[f] = max(worst[f], d)
        assert differ <= 1e-3 * n * len(scene["tick_scale"]), (kind, n, n_listeners, differ)
    print(f"\noracle vs float64, {kind}, {n_listeners} listeners: " + ", ".join(f"{f} {worst[f]:.2e}" for f in FIELDS))
    for f in FIELDS:
        MEASURED[f] = max(MEASURED.get(f, 0.0), worst[f])


def test_gpu_bounds_are_four_times_the_measured_figures():
    """Runs after the scenes above (same module, file order): the bound of each field is 4 x the worst figure measured,
    which calc_spat_ref records rounded up (by less than a quarter), and within the project's rtol for this kernel."""
    if len(MEASURED) != len(FIELDS):
        return  # run on its own there is nothing measured; the per-scene tests hold the figures either way
    print("\nmeasured over all scenes: " + ", ".join(f"{f} {MEASURED[f]:.2e}" for f in FIELDS))
    for f in FIELDS:
        assert 0.8 * ref.MEASURED[f] <= MEASURED[f] <= ref.MEASURED[f], (f, MEASURED[f], ref.MEASURED[f])
        assert ref.GPU_RTOL[f] == 4 * ref.MEASURED[f] <= ref.RTOL_CAP[f]


def test_oracle_against_float64_at_the_edges_and_without_areas():
    """The hand-placed edges, and the plain entry (no areas) on one dense scene of each kind."""
    rtol = ref.MEASURED
    for name, scene in sc.edge_cases().items():
        for t, (want, (got, rev, _, was)) in enumerate(zip(sc.run_ref(scene), run_oracle(scene))):
            assert sc.check(got, rev, want, rtol, f"{name} tick={t}") == 0
            np.testing.assert_array_equal(was, want["was_further"], err_msg=name)
    for kind in sc.SCENES:
        scene = sc.dense(kind, 257, 3, with_areas=False)
        assert scene["left"] == 0
        for t, (want, (got, _, _, was)) in enumerate(zip(sc.run_ref(scene, areas=False), run_oracle(scene, areas=False))):
            sc.check(got, None, want, rtol, f"{kind} plain tick={t}")
            np.testing.assert_array_equal(was, want["was_further"])
