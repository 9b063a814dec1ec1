"""tests/room_brir_ref.py, the float64 statement of gas_conv_ir_from_room_hrtf's rule, against what the header promises
of it (the delta-set identity, additivity over orders), against a convolution, against a case written out by hand and
against a turn of the listener; and the condition under which tests/test_gpu_room_brir.py may compare the device with
it: no image of any of its cases lies near a cell's edge.  No GPU.

The hand case is test_room_ir_reference.py's 1-D room: half_extent (5, 5, 5), source (1, 0, 0), listener (-2, 0, 0),
d0 = 3, c = 480 m/s at 48 kHz = 100 frames per metre; the image m = (1, 0, 0) lies at x = 9: dist 11, pos exactly 800."""
import numpy as np
import pytest

import er_rooms_ref as E
import room_brir_cases as CS
import room_brir_ref as BR
import room_ir_ref as R
from helpers import TOL, rel_rms

RATE = CS.RATE


@pytest.mark.parametrize("grid", [(12, 5), (1, 1), (64, 16)])
@pytest.mark.parametrize("orders", [None, (3, None)])
def test_delta_set_is_the_one_channel_rule_exactly(grid, orders):
    n_az, n_el = grid
    d = CS.describe()
    out = BR.brir(d, BR.delta_set(n_az * n_el), n_az, n_el, 2048, RATE, orders=orders)
    mono = R.ir(d, 1, 2048, RATE, orders=orders)
    assert mono.acc.any()
    assert np.array_equal(out.acc[0], mono.acc[0]) and np.array_equal(out.acc[1], mono.acc[0])
    assert out.h[0].tobytes() == out.h[1].tobytes() == mono.h[0].tobytes()


def test_delta_set_ignores_the_later_taps_of_a_longer_set():
    d = CS.describe()
    a = BR.brir(d, BR.delta_set(60, taps=1), 12, 5, 1000, RATE)
    b = BR.brir(d, BR.delta_set(60, taps=9), 12, 5, 1000, RATE)
    assert np.array_equal(a.acc, b.acc)


def test_orders_add_up_exactly():
    d, hrir = CS.describe(), CS.noise_set(21, 60, 32)
    whole = BR.brir(d, hrir, 12, 5, 2048, RATE)
    early = BR.brir(d, hrir, 12, 5, 2048, RATE, orders=(0, 2))
    tail = BR.brir(d, hrir, 12, 5, 2048, RATE, orders=(3, None))
    assert early.acc.any() and tail.acc.any()
    assert np.array_equal(early.acc + tail.acc, whole.acc)
    assert early.mono.candidates + tail.mono.candidates == whole.mono.candidates


def test_one_row_everywhere_is_a_convolution():
    """The same pair of rows in every cell: each ear is the one-channel response convolved with its row."""
    taps = 2048
    d = CS.describe()
    rng = np.random.default_rng(22)
    row = (rng.standard_normal((2, 40)) * 0.5).astype(np.float32)
    out = BR.brir(d, np.broadcast_to(row, (60, 2, 40)).copy(), 12, 5, taps, RATE)
    mono = R.ir(d, 1, taps, RATE).acc[0].astype(np.float64) / BR.ONE
    for e in range(2):
        want = np.convolve(mono, row[e].astype(np.float64))[:taps]
        err = rel_rms(out.h[e], want)
        print(f"ear {e}: rel rms {err:.3g}")
        assert err <= TOL


def test_one_image_by_hand():
    """Direct sound off (orders 1 .. 1) and every wall dead but +x: the image at x = 9, R = 0.5, dist 11, v = 0.5 * 3 / 11,
    pos = 800 exactly.  Move the source by a quarter frame (0.0025 m towards -x is not float32-exact, so the fraction is
    taken from the reference's own pos) and write the four taps of a two-tap HRIR out."""
    room = E.unit_room(half_extent=(5.0, 5.0, 5.0), c=480.0)
    room["reflectance"] = [[0.0, 0.5, 0.0, 0.0, 0.0, 0.0]]
    hrir = np.zeros((4, 2, 2), np.float32)
    hrir[:, 0] = (0.5, -0.25)
    hrir[:, 1] = (1.0, 2.0)
    d = R.describe(room, (1.0, 0.0, 0.0), (-2.0, 0.0, 0.0), min_order=1, max_order=1)
    out = BR.brir(d, hrir, 4, 1, 1000, RATE)
    v = 0.5 * 3.0 / 11.0
    assert out.mono.pos[0][out.mono.v[0] > 0].tolist() == [800.0]
    q = lambda x: int(np.rint(x * BR.ONE))
    assert out.acc[0, 800:803].tolist() == [q(v * 0.5), q(v * -0.25), 0]
    assert out.acc[1, 800:803].tolist() == [q(v * 1.0), q(v * 2.0), 0]
    assert np.count_nonzero(out.acc) == 4
    # a fractional delay: source at x = 0.875 (exact in float32): img = 9.125, d0 = 2.875, dist - d0 = 8.25 m = 825 frames;
    # at c = 512 m/s the same path is 8.25 / 512 * 48000 = 773.4375 frames: k = 773, f = 0.4375
    room["speed_of_sound"] = 512.0
    d = R.describe(room, (0.875, 0.0, 0.0), (-2.0, 0.0, 0.0), min_order=1, max_order=1)
    out = BR.brir(d, hrir, 4, 1, 1000, RATE)
    v = 0.5 * 2.875 / 11.125
    a0, a1 = v * (1.0 - 0.4375), v * 0.4375
    assert out.acc[0, 773:777].tolist() == [q(a0 * 0.5), q(a0 * -0.25 + a1 * 0.5), q(a1 * -0.25), 0]
    assert out.acc[1, 773:777].tolist() == [q(a0 * 1.0), q(a0 * 2.0 + a1 * 1.0), q(a1 * 2.0), 0]
    assert np.count_nonzero(out.acc) == 6


def test_the_cell_follows_the_convention_of_hrtf_dir():
    """Identity listener: straight ahead (-z) is azimuth 0, +x is a quarter turn, +y is up (the higher rows)."""
    n_az, n_el = 8, 5
    p = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]]).T
    dirs, near = BR.cells(p, n_az, n_el)
    assert dirs.tolist()[:6] == [2 * n_az + 0, 2 * n_az + 2, 2 * n_az + 4, 2 * n_az + 6, 3 * n_az + 2, 1 * n_az + 2]
    assert dirs[6] // n_az == 4 and near.tolist() == [False] * 6 + [True]  # straight up: the top row, azimuth ill-defined


def test_a_quarter_turn_of_the_listener_moves_the_direct_sound_by_a_quarter_of_the_azimuths():
    """Turning the listener by 90 degrees about +y to its left (its -z axis goes to -x) moves a source 90 degrees to the
    right in its frame: ai grows by n_az / 4, the elevation row stays."""
    n_az, n_el = 12, 5
    hrir = BR.delta_set(n_az * n_el)
    d0 = CS.describe(listener_basis=CS.rotation(0.2, 0.0, 0.0))
    d1 = CS.describe(listener_basis=CS.rotation(0.2 + np.pi / 2, 0.0, 0.0))
    a = BR.brir(d0, hrir, n_az, n_el, 256, RATE, orders=(0, 0))
    b = BR.brir(d1, hrir, n_az, n_el, 256, RATE, orders=(0, 0))
    assert a.near_edge == 0 and b.near_edge == 0 and len(a.dirs) == 1
    ai0, ai1 = int(a.dirs[0]) % n_az, int(b.dirs[0]) % n_az
    assert int(a.dirs[0]) // n_az == int(b.dirs[0]) // n_az
    assert (ai0 + n_az // 4) % n_az == ai1


@pytest.mark.parametrize("name", list(CS.CASES))
def test_no_image_of_a_gpu_case_lies_near_an_edge(name):
    """The condition under which two libraries' atan2 cannot pick different cells."""
    _, hrir, n_az, n_el, taps, ref = CS.reference(name)
    print(f"{name}: {ref.mono.candidates} candidates, {ref.in_range} reach a tap, near_edge {ref.near_edge}")
    assert ref.in_range >= 10 and ref.h[0].any() and ref.h[1].any()
    assert ref.near_edge == 0
    assert len(set(ref.dirs.tolist())) >= min(n_az * n_el, 5)  # the images do come from many directions


@pytest.mark.parametrize("angles", CS.ORIENTATIONS)
def test_direct_sound_cases_are_clear_of_edges_in_both_formulations(angles):
    n_az, n_el = CS.DIRECT_GRID
    basis = CS.rotation(*angles)
    d = CS.describe(listener_basis=basis)
    ref = BR.brir(d, BR.delta_set(n_az * n_el), n_az, n_el, 64, RATE, orders=(0, 0))
    cell, near = CS.calc_spatialization_cell(CS.SRC, CS.LIS, d["listener"]["basis"][0], n_az, n_el)
    assert ref.near_edge == 0 and not near
    assert int(ref.dirs[0]) == cell


def test_orientations_reach_different_cells():
    n_az, n_el = CS.DIRECT_GRID
    got = {CS.calc_spatialization_cell(CS.SRC, CS.LIS, CS.rotation(*a).astype(np.float32), n_az, n_el)[0] for a in CS.ORIENTATIONS}
    assert len(got) >= 4
