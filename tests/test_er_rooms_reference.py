"""tests/er_rooms_ref.py, the float64 statement of gas_calc_early_reflections' rule, against cases worked out by hand,
and the shares of its scenes that a float32 implementation may legitimately answer differently.  No GPU.

The 1-D case.  Identity basis, origin 0, half_extent (5, 5, 5), source s = (1, 0, 0), listener l = (-2, 0, 0): d0 = 3.
Reflectances -x 0.5, +x 0.8, the y and z walls 0 (every image that meets one of them has R = 0), level 1,
c = 480 m/s at 48 kHz = 100 frames per metre, ring 4096, 512 frames: M = 3584.
    candidate  0, m = (-1,0,0): img_x = -10 - 1 = -11, dist =  9, R = 0.5       g = 0.5 * 3 /  9 = 1/6     fr =  600
    candidate  5, m = ( 1,0,0): img_x =  10 - 1 =   9, dist = 11, R = 0.8       g = 0.8 * 3 / 11 = 12/55   fr =  800
    candidate  6, m = (-2,0,0): img_x = -20 + 1 = -19, dist = 17, R = 0.8 * 0.5 g = 0.4 * 3 / 17 = 6/85    fr = 1400
    candidate 23, m = ( 2,0,0): img_x =  20 + 1 =  21, dist = 23, R = 0.8 * 0.5 g = 0.4 * 3 / 23 = 6/115   fr = 2000
By gain: 5, 0, 6, 23; the other four taps are (0, 1) and belong to the lowest-numbered candidates left: 1, 2, 3, 4."""
import numpy as np
import pytest

import er_rooms_ref as R

RATE, F, RING = 48000.0, 512, 4096


def test_candidate_numbering():
    assert R.TRIPLES[:8] == [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0), (-2, 0, 0), (-1, -1, 0)]
    assert R.TRIPLES[8:] == [(-1, 0, -1), (-1, 0, 1), (-1, 1, 0), (0, -2, 0), (0, -1, -1), (0, -1, 1), (0, 0, -2), (0, 0, 2), (0, 1, -1), (0, 1, 1), (0, 2, 0), (1, -1, 0), (1, 0, -1), (1, 0, 1), (1, 1, 0), (2, 0, 0)]
    assert len(set(R.TRIPLES)) == 24 and all(1 <= sum(abs(a) for a in m) <= 2 for m in R.TRIPLES)


def test_the_one_dimensional_case_of_the_docstring():
    room = R.unit_room(half_extent=(5, 5, 5), c=480.0)
    room["reflectance"] = [[0.5, 0.8, 0, 0, 0, 0]]
    t = R.taps(room, [[1, 0, 0]], [-2, 0, 0], RATE, F, RING)
    assert t.d0[0] == 3.0
    assert list(t.cand[0]) == [5, 0, 6, 23, 1, 2, 3, 4]
    # the reflectances are float32 values: 0.5 is exact, 0.8 is not
    r8 = float(np.float32(0.8))
    np.testing.assert_allclose(t.gain[0], [r8 * 3 / 11, 0.5 * 3 / 9, r8 * 0.5 * 3 / 17, r8 * 0.5 * 3 / 23, 0, 0, 0, 0], rtol=1e-15)
    assert list(t.delay[0]) == [800, 600, 1400, 2000, 1, 1, 1, 1]
    np.testing.assert_allclose(t.dist_all[0, [0, 5, 6, 23]], [9, 11, 17, 23], rtol=1e-15)
    # the same room rotated and moved: the taps depend on the room frame only
    b = R.random_basis(np.random.default_rng(3))
    room2 = room.copy()
    room2["basis"], room2["origin"] = b, [[3.0, -7.0, 11.0]]
    o = room2["origin"][0].astype(np.float64)
    b32 = room2["basis"][0].astype(np.float64)
    t2 = R.taps(room2, [b32 @ [1, 0, 0] + o], b32 @ [-2, 0, 0] + o, RATE, F, RING)
    assert list(t2.cand[0]) == list(t.cand[0])
    np.testing.assert_allclose(t2.gain[0], t.gain[0], rtol=1e-5)
    assert np.all(np.abs(t2.delay[0] - t.delay[0]) <= 1)


def test_cube_with_the_source_at_its_centre():
    a = 4.0
    lis = np.array([1.5, -0.5, 2.0])
    room = R.unit_room(half_extent=(a, a, a), reflectance=0.75, level=0.5)
    t = R.taps(room, [[0, 0, 0]], lis, RATE, F, RING)
    d0 = np.sqrt((lis**2).sum())
    assert t.d0[0] == pytest.approx(d0, rel=1e-15)
    for cnum in range(6):  # first order: the image lies at 2 a m
        img = 2 * a * np.array(R.TRIPLES[cnum], np.float64)
        dist = np.sqrt(((img - lis) ** 2).sum())
        assert t.dist_all[0, cnum] == pytest.approx(dist, rel=1e-15)
        assert t.g_all[0, cnum] == pytest.approx(0.5 * 0.75 * d0 / dist, rel=1e-15)
        assert t.delay_all[0, cnum] == int(np.rint((dist - d0) / 343.0 * RATE))
    # second order through one wall pair comes back to the source's mirror twice removed: 4 a m; through two walls: 2 a m
    for cnum in range(6, 24):
        img = 2 * a * np.array(R.TRIPLES[cnum], np.float64)
        assert t.dist_all[0, cnum] == pytest.approx(np.sqrt(((img - lis) ** 2).sum()), rel=1e-15)
        assert t.g_all[0, cnum] == pytest.approx(0.5 * 0.75**2 * d0 / t.dist_all[0, cnum], rel=1e-15)
    assert np.all(t.gain[0] <= 0.5) and np.all(np.diff(t.gain[0]) <= 0)


def test_every_image_is_at_least_as_far_as_the_source():
    rooms, ri, pos, lis = R.scene(np.random.default_rng(11), 2000)
    t = R.taps(rooms, pos, lis, RATE, F, RING, ri)
    assert not t.outside.any()
    assert np.all(t.dist_all >= t.d0[:, None])
    assert np.all(t.g_all <= rooms["level"][ri].astype(np.float64)[:, None])
    assert np.all(t.delay >= 1) and np.all(t.delay <= RING - F)
    assert np.all(np.diff(t.gain, axis=1) <= 0)


def test_first_order_rooms_have_six_taps():
    rooms, ri, pos, lis = R.scene(np.random.default_rng(12), 500, n_rooms=2, max_order=1)
    rooms["half_extent"] = np.minimum(rooms["half_extent"], 6.0)  # every first-order image within reach of the ring
    t = R.taps(rooms, pos, lis, RATE, F, RING, ri)
    inside = ~t.outside
    assert inside.sum() > 100
    assert np.all(t.gain[inside][:, :6] > 0) and np.all(t.cand[inside][:, :6] < 6)
    assert np.all(t.gain[:, 6:] == 0) and np.all(t.delay[:, 6:] == 1)


def test_rule_two_and_the_far_images():
    room = R.unit_room()
    for pos, lis in ([[4.1, 0, 0], [0, 0, 0]], [[0, 0, 0], [0, -2.6, 0]]):
        t = R.taps(room, [pos], lis, RATE, F, RING)
        assert t.outside[0] and np.all(t.gain == 0) and np.all(t.delay == 1)
    t = R.taps(room, [[1, 1, 1]], [0, 0, 0], RATE, F, RING, room_index=[R.ROOM_NONE])
    assert np.all(t.gain == 0) and np.all(t.delay == 1)
    big = R.unit_room(half_extent=(200, 200, 200))  # the nearest image is 400 m - 2 m away: 55 000 frames
    t = R.taps(big, [[1, 0, 0]], [-1, 0, 0], RATE, F, RING)
    assert not t.outside[0] and np.all(t.gain == 0) and np.all(t.delay == 1)
    t = R.taps(room, [[1, 1, 1]], [1, 1, 1], RATE, F, RING)  # d0 = 0
    assert np.all(t.gain == 0) and np.all(t.delay == 1)


def test_border_shares_of_the_scene_generator():
    """What a float32 implementation may answer differently stays a small share of a scene: selected taps next to a
    rounding border at most 3 %, sources with a near tie among their nine largest gains at most 1 % (a float32 numpy
    restatement gave 1.9 % and 0.33 % on 4000 sources), sources with a candidate at the ring's reach at most 0.5 %."""
    rooms, ri, pos, lis = R.scene(np.random.default_rng(2024), 4000)
    t = R.taps(rooms, pos, lis, RATE, F, RING, ri)
    live = t.gain > 0
    share_border = t.border.sum() / live.sum()
    share_tie = (t.gap < R.NEAR_TIE).any(axis=1).mean()
    share_edge = t.drop_edge.mean()
    print(f"border taps {share_border:.4f}, near-tie sources {share_tie:.4f}, ring-reach sources {share_edge:.4f}")
    assert live.sum() > 0.9 * live.size
    assert share_border <= 0.03
    assert share_tie <= 0.01
    assert share_edge <= 0.005


def test_binding_matches_the_header_and_the_reference(gas):
    """No GPU: the PODs of the binding are the header's, the symbol is exported, and synth's room scenes are inside their
    rooms by the reference's own test."""
    import os
    import re

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    assert K.ROOM_DTYPE == R.ROOM_DTYPE and K.ROOM_DTYPE.itemsize == 96 and K.ROOM_NONE == R.ROOM_NONE
    assert [K.ROOM_DTYPE.fields[f][1] for f in ("basis", "origin", "half_extent", "reflectance", "speed_of_sound", "level", "max_order")] == [0, 36, 48, 60, 84, 88, 92]
    assert K.ER_TAPS_DTYPE.itemsize == 64 and K.ER_TAPS_DTYPE.fields["delay"][1] == 32
    # a gas_er_taps is bytes 64 .. 127 of a gas_params
    assert K.PARAMS_DTYPE.fields["er_gain"][1] == 64 and K.PARAMS_DTYPE.fields["er_delay"][1] == 64 + K.ER_TAPS_DTYPE.fields["delay"][1]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gas_amd.h")).read()
    assert int(re.search(r"#define GAS_MAX_ROOMS (\d+)", header).group(1)) == K.MAX_ROOMS
    assert int(re.search(r"#define GAS_ROOM_NONE (0x[0-9a-f]+)u", header).group(1), 16) == K.ROOM_NONE
    assert "gas_calc_early_reflections" in K.EXPORTS and hasattr(gas.load_library(), "gas_calc_early_reflections")
    rooms, ri, poses, listener = synth.draw_room_scene(np.random.default_rng(1), 300)
    t = R.taps(rooms, poses["position"], listener["origin"][0], RATE, F, RING, ri)
    assert not t.outside.any() and (t.gain[:, 0] > 0).all()
