"""Scenes for the parameter generator's tests, shared by test_calc_spat_reference.py (oracle against calc_spat_ref on
the CPU) and test_gpu_calc_spat_edges.py (kernel against both).  Dense scenes are drawn under a fixed seed; a row that
calc_spat_ref's margins put on a cancellation or within float32's reach of a branch border is redrawn under the same
generator until none is left (see calc_spat_ref.badly_placed)."""
import numpy as np

import calc_spat_ref as ref
from godot_audio_spatializer_amd import capi as K

DENSE_N = (1, 255, 256, 257, 1000)
DENSE_LISTENERS = (1, 3, 16)
N_CFGS = 64
SCENES = ("far", "near", "quirk")
PANNING = {"far": (1.0, 2.0), "near": (0.3, 0.5, 1.5), "quirk": (1.0, 0.5, 2.0)}
TICK_SCALE = {"far": (1.0, 3.0), "near": (1.0, 0.5), "quirk": (1.0, 3.0)}  # positions of tick 0, tick 1 (sources leave max_distance)


def random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float32)


def configs(kind):
    """64 configs: attenuation model x speaker mode in full, the other settings spread over them."""
    c = K.default_spat3d_config(N_CFGS)
    ps = PANNING[kind]
    for i in range(N_CFGS):
        c["attenuation_model"][i] = i & 3
        c["speaker_mode"][i] = (i >> 2) & 3
        c["max_distance"][i] = (0.0, 25.0, 60.0)[(i + (i >> 2) + (i >> 4)) % 3]
        c["emission_angle_enabled"][i] = (i >> 4) & 1
        c["emission_angle"][i] = 30.0 + 10.0 * (i % 5)
        c["doppler_tracking"][i] = (i >> 5) & 1
        c["unit_size"][i] = (4.0, 10.0)[(i ^ (i >> 3)) & 1]
        c["attenuation_filter_db"][i] = (-24.0, -12.0)[((i >> 1) ^ (i >> 4)) & 1]
        c["panning_strength"][i] = ps[(i + (i >> 2)) % len(ps)]
    c["hrtf_n_az"] = 32
    c["hrtf_n_el"] = 9
    return c


def _draw_rows(kind, rng, n, listeners, with_areas=True):
    nl = len(listeners)
    poses = np.zeros(n, K.POSE_DTYPE)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if kind == "near":  # within 0.9 of every listener (they stand within 0.05 of the origin): 1 + dot >= 0.1 for every speaker
        d = np.exp(rng.uniform(np.log(0.02), np.log(0.85), n))
    else:
        d = np.exp(rng.uniform(np.log(0.5), np.log(120.0), n))
    poses["position"] = (u * d[:, None]).astype(np.float32)
    poses["velocity"] = rng.uniform(-30, 30, (n, 3))
    poses["velocity"][rng.random(n) < 0.2] = 0
    fw = rng.standard_normal((n, 3))
    poses["forward"] = fw / np.linalg.norm(fw, axis=1, keepdims=True)
    on_axis = rng.random(n) < 0.03  # the cone's axis through listener 0: the dot lands within an ulp of +-1
    rel = poses["position"] - listeners["origin"][0]
    sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    poses["forward"][on_axis] = (rel / np.maximum(np.linalg.norm(rel, axis=1, keepdims=True), 1e-12) * sign[:, None]).astype(np.float32)[on_axis]
    poses["volume_db"] = rng.uniform(-12, 6, n)
    poses["max_db"] = 3.0
    poses["pitch_scale"] = rng.uniform(0.5, 2.0, n)
    areas = np.zeros(n, K.AREA_SEND_DTYPE)
    areas["present"] = (rng.random(n) < 0.6) & with_areas
    areas["using_reverb_bus"] = rng.random(n) < 0.7
    areas["reverb_uniformity"] = np.where(rng.random(n) < 0.4, 0.0, rng.uniform(0.05, 1.0, n))
    areas["reverb_amount"] = rng.uniform(0.0, 1.0, n)
    lap = (rng.standard_normal((n, nl, 3)) * np.exp(rng.uniform(np.log(0.2), np.log(90.0), (n, nl, 1)))).astype(np.float32)
    lap[rng.random(n) < 0.1] = 0.0  # the listener stands inside the area
    return poses, areas, lap


def tick_poses(scene, tick):
    p = scene["poses"].copy()
    p["position"] *= np.float32(scene["tick_scale"][tick])
    return p


def run_ref(scene, areas=True):
    """calc_spat_ref over the scene's ticks: a list of result dicts (the latch carried from tick to tick)."""
    was = np.zeros(len(scene["poses"]), np.int32)
    out = []
    for t in range(len(scene["tick_scale"])):
        r = ref.calc(scene["cfgs"], scene["cfg_index"], tick_poses(scene, t), scene["listeners"], was, scene["areas"] if areas else None, scene["lap"] if areas else None)
        was = r["was_further"]
        out.append(r)
    return out


def dense(kind, n, n_listeners, seed=0, with_areas=True):
    """The scene dict: cfgs, cfg_index, poses, listeners, areas, lap, tick_scale; `redrawn` counts rows drawn again and
    `left` those still badly placed (the tests assert 0).  with_areas=False: no source sits in an area (the plain entry)."""
    rng = np.random.default_rng([SCENES.index(kind), n, n_listeners, seed])
    listeners = np.zeros(n_listeners, K.LISTENER_DTYPE)
    for i in range(n_listeners):
        listeners["basis"][i] = random_rotation(rng)
        # near: at the origin but for a jitter that keeps their distances to a source, and so their multipliers, apart --
        # from exactly one point every listener is equally loud up to rounding, and which one is "the loudest" is noise
        listeners["origin"][i] = rng.uniform(-0.028, 0.028, 3) if kind == "near" else rng.uniform(-5, 5, 3)
        listeners["velocity"][i] = rng.uniform(-3, 3, 3)
    scene = {"kind": kind, "cfgs": configs(kind), "cfg_index": rng.integers(0, N_CFGS, n).astype(np.uint32), "listeners": listeners, "tick_scale": TICK_SCALE[kind]}
    scene["poses"], scene["areas"], scene["lap"] = _draw_rows(kind, rng, n, listeners, with_areas)
    def bad_rows(poses, areas, lap, cfg_index):
        sub = dict(scene, poses=poses, areas=areas, lap=lap, cfg_index=cfg_index)
        bad = np.zeros(len(poses), bool)
        for r in run_ref(sub):
            bad |= ref.badly_placed(r["margins"])
        return bad

    todo = np.flatnonzero(bad_rows(scene["poses"], scene["areas"], scene["lap"], scene["cfg_index"]))  # a row's margins depend on no other row
    redrawn = 0
    for _ in range(100):
        if not len(todo):
            break
        redrawn += len(todo)
        tries = 16  # candidates per row and round; the first well-placed one is taken
        p, a, l = _draw_rows(kind, rng, len(todo) * tries, listeners, with_areas)
        good = ~bad_rows(p, a, l, np.repeat(scene["cfg_index"][todo], tries)).reshape(len(todo), tries)
        pick = np.arange(len(todo)) * tries + good.argmax(axis=1)
        found = good.any(axis=1)
        scene["poses"][todo[found]], scene["areas"][todo[found]], scene["lap"][todo[found]] = p[pick[found]], a[pick[found]], l[pick[found]]
        todo = todo[~found]
    scene["redrawn"], scene["left"] = redrawn, len(todo)
    return scene


# ---- hand-placed edges: every value exact in float32, so float32 and float64 take the same branch by construction ----

EYE = np.eye(3, dtype=np.float32)
TURN_Y_90 = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)  # a signed axis permutation
TURN_Y_180 = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float32)


def cfg(n=1, **kw):
    c = K.default_spat3d_config(n, hrtf_n_az=32, hrtf_n_el=9)
    for k, v in kw.items():
        c[k] = v
    return c


def poses_at(positions, **kw):
    p = np.zeros(len(positions), K.POSE_DTYPE)
    p["position"] = np.asarray(positions, np.float32)
    p["forward"] = (0, 0, 1)
    p["max_db"] = 3.0
    p["pitch_scale"] = 1.0
    for k, v in kw.items():
        p[k] = v
    return p


def listeners_at(*specs):
    """specs: (basis, origin, velocity) per listener."""
    lis = np.zeros(len(specs), K.LISTENER_DTYPE)
    for i, (b, o, v) in enumerate(specs):
        lis["basis"][i], lis["origin"][i], lis["velocity"][i] = b, o, v
    return lis


def _case(cfgs, poses, listeners, cfg_index=None, areas=None, lap=None, ticks=1):
    n = len(poses)
    return {
        "kind": "edge",
        "cfgs": cfgs,
        "cfg_index": np.zeros(n, np.uint32) if cfg_index is None else np.asarray(cfg_index, np.uint32),
        "poses": poses,
        "listeners": listeners,
        "areas": np.zeros(n, K.AREA_SEND_DTYPE) if areas is None else areas,
        "lap": np.zeros((n, len(listeners), 3), np.float32) if lap is None else np.asarray(lap, np.float32),
        "tick_scale": (1.0,) * ticks,
    }


def area_rows(n, uniformity, amount=0.75):
    a = np.zeros(n, K.AREA_SEND_DTYPE)
    a["present"], a["using_reverb_bus"], a["reverb_uniformity"], a["reverb_amount"] = 1, 1, uniformity, amount
    return a


ONE = listeners_at((EYE, (0, 0, 0), (0, 0, 0)))
TINY = np.float32(1e-20)  # its square is a float32 denormal
STEP = float(np.nextafter(np.float32(25.0), np.float32(30.0)))


def edge_cases():
    """name -> scene dict (see dense); what each row is for stands in test_gpu_calc_spat_edges.py."""
    e = {}
    # stereo (SPCAP of 3e19 overflows float32), every attenuation model, one with max_distance
    pan_cfgs = cfg(5, speaker_mode=0)
    pan_cfgs["attenuation_model"] = (0, 1, 2, 3, 0)
    pan_cfgs["max_distance"][4] = 25.0
    pan_pos = [(0, 0, 0), (TINY, 0, 0), (-TINY, 0, 0), (0, 0, TINY), (0, 0, -TINY), (TINY, TINY, TINY), (-TINY, TINY, -TINY), (3e19, 0, 0), (0, 3e19, 0)]
    pan_idx = np.repeat(np.arange(5), len(pan_pos))
    # (with attenuation disabled the 3e19 row is not silent, and float32's x * x = inf pans it to the centre: left out)
    keep = ~((pan_idx == 3) & (np.tile(np.arange(len(pan_pos)), 5) == 7))
    e["pan_limits"] = _case(pan_cfgs, poses_at(pan_pos * 5)[keep], ONE, cfg_index=pan_idx[keep])
    # grid corners: n_el in {1, 2, 9} x n_az in {1, 7, 32}; straight up, down, behind (+0.0 on x), ahead
    grid = cfg(9, attenuation_model=3)
    grid["hrtf_n_el"] = np.repeat((1, 2, 9), 3)
    grid["hrtf_n_az"] = np.tile((1, 7, 32), 3)
    corner = [(0, 2, 0), (0, -2, 0), (0.0, 0, 2), (0, 0, -2), (2, 0, 0), (-2, 0, 0)]
    e["grid_corners"] = _case(grid, poses_at(corner * 9), ONE, cfg_index=np.repeat(np.arange(9), len(corner)))
    # the same seen by a listener turned half round: (+0.0, -0.0, -2) is straight behind it with x = -0.0 in its space
    turned = listeners_at((TURN_Y_180, (0, 0, 0), (0, 0, 0)))
    e["grid_behind_negative_zero"] = _case(grid, poses_at([(0.0, -0.0, -2.0)] * 9), turned, cfg_index=np.arange(9))
    # dist == max_distance (in range, taper 0), one float32 step beyond (out), twice: the latch
    e["max_distance_border"] = _case(cfg(1, max_distance=25.0), poses_at([(0, 0, -25.0), (0, 0, -STEP), (25.0, 0, 0), (0, -STEP, 0), (0, 0, -5.0)]), ONE, ticks=2)
    # an area point that widens total_max vetoes the listener (:369); one at max_distance exactly does not
    e["area_veto"] = _case(cfg(1, max_distance=25.0), poses_at([(0, 0, -5.0)] * 3), ONE, areas=area_rows(3, 0.5), lap=[[(0, 0, -30.0)], [(0, 0, -25.0)], [(0, -STEP, 0)]], ticks=2)
    # angle == emission_angle exactly (forward along x, listener->source along -z: the cosine is 0, the angle 90),
    # and a little to either side; a zero forward (normalized() leaves it zero: 90 degrees against a 45 degree cone)
    cone = cfg(2, emission_angle_enabled=1, emission_angle=90.0, attenuation_model=3)
    cone["emission_angle"][1] = 45.0
    tilt = 2.0**-18
    cone_poses = poses_at([(0, 0, -5.0)] * 5)
    cone_poses["forward"] = [(1, 0, 0), (1, 0, tilt), (1, 0, -tilt), (0, 0, 0), (0, 0, 0)]
    e["cone_border"] = _case(cone, cone_poses, ONE, cfg_index=[0, 0, 0, 0, 1])
    # att + volume_db == max_db (attenuation disabled: att is volume_db) and one step above it
    e["max_db_border"] = _case(cfg(1, attenuation_model=3), poses_at([(3, 0, -4.0)] * 3, volume_db=[3.0, float(np.nextafter(np.float32(3), np.float32(4))), 2.5]), ONE)
    # attenuation == 1 in calc_reverb_vol (0 dB: the centre branch), below it (panned) and above
    e["reverb_attenuation_one"] = _case(cfg(4, attenuation_model=3, speaker_mode=[0, 1, 2, 3]), poses_at([(3, 0, -4.0)] * 12, volume_db=np.repeat((0.0, -1.0, 2.0), 4)), ONE, cfg_index=np.tile(np.arange(4), 3), areas=area_rows(12, 0.5), lap=[[(3.0, 1.0, -4.0)]] * 12)
    # Doppler: approach at exactly the speed of sound (c + v.a == 0 -> +inf -> 8), supersonic approach (negative -> 0.125),
    # supersonic recession (343 / 743), at rest, and tracking disabled with the same velocities
    dop = cfg(2, doppler_tracking=1, attenuation_model=3)
    dop["doppler_tracking"][1] = 0
    vel = [(0, 0, 343.0), (0, 0, 400.0), (0, 0, -400.0), (0, 0, 0), (7.0, 0, 0)]
    e["doppler_clamps"] = _case(dop, poses_at([(0, 0, -10.0)] * 10, velocity=vel * 2, pitch_scale=[1.0] * 5 + [1.5] * 5), ONE, cfg_index=np.repeat((0, 1), 5))
    # a listener co-moving with the source (skipped, :416) next to one that is not
    two = listeners_at((EYE, (0, 0, 0), (5.0, 0, 0)), (EYE, (0, 0, 6.0), (0, 0, 0)))
    e["doppler_co_moving"] = _case(cfg(1, doppler_tracking=1), poses_at([(0, 0, -4.0), (3.0, 0, 2.0)], velocity=[(5.0, 0, 0)] * 2, pitch_scale=1.5), two)
    # equal multipliers: the same origin, bases that are signed axis permutations; 9 + 0 + 16 sums to 25 in any order
    tie = listeners_at((EYE, (0, 0, 0), (0, 0, 0)), (TURN_Y_90, (0, 0, 0), (0, 0, 0)), (TURN_Y_180, (0, 0, 0), (0, 0, 0)))
    e["equal_multipliers"] = _case(cfg(4, speaker_mode=[0, 1, 2, 3]), poses_at([(3.0, 0, -4.0)] * 4), tie, cfg_index=np.arange(4))
    # the last listener in range sets linear_attenuation although the first is louder; one out of range between them
    three = listeners_at((EYE, (0, 0, 0), (0, 0, 0)), (EYE, (100.0, 0, 0), (0, 0, 0)), (TURN_Y_90, (0, 0, 10.0), (0, 0, 0)))
    e["last_in_range_wins"] = _case(cfg(2, max_distance=[25.0, 0.0]), poses_at([(0, 0, -5.0), (0, 0, -5.0), (0, 2.0, 1.0)]), three, cfg_index=[0, 1, 0])
    # no listeners at all, two ticks
    none = cfg(3, max_distance=[0.0, 25.0, 25.0])
    none["hrtf_n_az"][2] = 0
    e["no_listeners"] = _case(none, poses_at([(1, 2, 3)] * 3, pitch_scale=1.25, velocity=(9, 9, 9)), np.zeros(0, K.LISTENER_DTYPE), cfg_index=[0, 1, 2], ticks=2)
    # the most listeners the entry takes
    rng = np.random.default_rng(16)
    many = listeners_at(*[((EYE, TURN_Y_90, TURN_Y_180)[i % 3], rng.integers(-8, 9, 3), rng.integers(-2, 3, 3)) for i in range(16)])
    e["sixteen_listeners"] = _case(cfg(4, speaker_mode=[0, 1, 2, 3], doppler_tracking=1, max_distance=[0.0, 25.0, 60.0, 25.0], panning_strength=[1.0, 1.0, 2.0, 2.0]), poses_at(rng.integers(-20, 21, (64, 3)) + 0.5, velocity=rng.integers(-30, 31, (64, 3))), many, cfg_index=np.arange(64) % 4)
    return e


def check(got, got_reverb, want, rtol, what):
    """Field by field against a calc_spat_ref result: NaN patterns equal, every finite element within rtol (and the
    project's atol), the cutoff, the latch equal, hrtf_dir equal except on a rounding border of the grid.  Returns the
    number of hrtf_dir that differ.  got_reverb may be None."""
    for f in ("mix_volumes", "pitch_scale", "linear_attenuation", "hrtf_gain", "reverb"):
        g = got_reverb if f == "reverb" else got[f]
        if g is None:
            continue
        w = want[f]
        if f == "hrtf_gain":
            g, w = g[want["hrtf_written"]], w[want["hrtf_written"]]
        nan = np.isnan(w)
        np.testing.assert_array_equal(np.isnan(g), nan, err_msg=f"{what}: NaN pattern of {f}")
        np.testing.assert_allclose(g[~nan], w[~nan], rtol=rtol[f], atol=ref.ATOL[f], err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(got["attenuation_filter_cutoff_hz"], want["attenuation_filter_cutoff_hz"], err_msg=what)
    np.testing.assert_array_equal(got["update_parameters"], want["update_parameters"], err_msg=f"{what}: latch")
    differ = want["hrtf_written"] & (got["hrtf_dir"] != want["hrtf_dir"])
    assert ref.on_grid_border(want["margins"])[differ].all(), f"{what}: hrtf_dir differs away from a rounding border at rows {np.flatnonzero(differ & ~ref.on_grid_border(want['margins']))}"
    return int(differ.sum())


def deviation(got, got_reverb, want):
    """Worst |got - want| / (atol + |want|) per field over the finite elements."""
    out = {}
    for f in ("mix_volumes", "pitch_scale", "linear_attenuation", "hrtf_gain", "reverb"):
        g, w = (got_reverb if f == "reverb" else got[f]), want[f]
        fin = np.isfinite(w) & np.isfinite(g)
        out[f] = float((np.abs(g - w)[fin] / (ref.ATOL[f] + np.abs(w[fin]))).max()) if fin.any() else 0.0
    return out
