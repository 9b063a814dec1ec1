"""tests/room_planes_ref.py against what is known without a GPU: a box given as its six planes is the lattice of
tests/room_ir_ref.py, a lone ground plane is one image whose tap and shares are worked out by hand, a corner and two
parallel planes have the images theory says, source and receiver may be swapped, and the candidates are counted as the
header counts them."""
import numpy as np
import pytest

import er_rooms_ref as E
import room_ir_ref as R
import room_planes_ref as P
from helpers import TOL, rel_rms

RATE = 48000.0
ORIGIN = np.array([3.0, -7.0, 11.0])
HALF = (2.5, 2.0, 1.5)
REFL = (0.9, 0.85, 0.8, 0.75, 0.7, 0.95)
SRC, LIS = ORIGIN + (1.0, 0.5, 0.25), ORIGIN + (-1.0, 0.25, -0.5)
ATTIC_SRC, ATTIC_LIS = (1.1, 1.2, 0.5), (-0.9, 1.45, -0.8)


@pytest.mark.parametrize("channels,max_order", [(1, 3), (2, 4)])
def test_a_box_as_six_planes_is_the_box(channels, max_order):
    room = E.unit_room(half_extent=HALF)
    room["reflectance"] = [list(REFL)]
    room["origin"] = ORIGIN
    taps = 2000
    box = R.ir(R.describe(room, SRC, LIS, ear_spacing=0.18, max_order=max_order), channels, taps, RATE)
    got = P.ir(P.describe(P.box_planes(ORIGIN, HALF, REFL), SRC, LIS, ear_spacing=0.18, max_order=max_order), channels, taps, RATE)
    assert box.h.any()
    print(f"{channels} channel(s), max_order {max_order}: int64 sums bitwise equal {np.array_equal(got.acc, box.acc)}, largest difference {np.abs(got.acc - box.acc).max()} / 2^32")
    for e in range(channels):
        mx = np.abs(got.h[e].astype(np.float64) - box.h[e]).max() / np.abs(box.h[e]).max()
        assert rel_rms(got.h[e], box.h[e]) <= TOL and mx <= TOL
    assert got.candidates == sum(6 * 5 ** (k - 1) for k in range(1, max_order + 1))


def test_one_ground_plane_is_one_image_by_hand():
    """Source (0, 3, 0) and listener (8, 3, 0) over the plane y = 0: d0 = 8, the image is (0, -3, 0), dist = 10 exactly.
    pos = (10 - 8) / 343 * 48000 = 279.88...; v = 0.5 * 8 / 10 = 0.4."""
    d = P.describe([((0, 1, 0), 0.0, 0.5)], (0.0, 3.0, 0.0), (8.0, 3.0, 0.0), max_order=1, level=0.5)
    out = P.ir(d, 1, 400, RATE)
    assert (out.candidates, out.void, out.valid) == (1, 0, [1])
    pos = 2.0 / 343.0 * 48000.0
    k = 279
    assert k < pos < k + 1
    f = pos - k
    want = np.zeros(400, np.int64)
    want[0] = 1 << 32  # the direct sound: v = 1, pos = 0
    v = 0.5 * 8.0 / 10.0
    want[k] = round(v * (1.0 - f) * 2.0**32)
    want[k + 1] = round(v * f * 2.0**32)
    assert np.array_equal(out.acc[0], want)
    assert out.h[0, 0] == np.float32(0.5) and out.h[0, k] == np.float32(0.5 * want[k] / 2.0**32)
    assert out.v_min == v and out.margin == np.inf  # no other plane to test a hit against
    no_direct = P.ir(P.describe([((0, 1, 0), 0.0, 0.5)], (0.0, 3.0, 0.0), (8.0, 3.0, 0.0), min_order=1, max_order=1), 1, 400, RATE)
    assert no_direct.acc[0, 0] == 0 and np.array_equal(no_direct.acc[0, 1:], want[1:])


def test_a_corner_of_three_planes_has_seven_images():
    d = P.describe([((1, 0, 0), 0.0, 0.9), ((0, 1, 0), 0.0, 0.8), ((0, 0, 1), 0.0, 0.7)], (1.0, 1.5, 2.0), (2.0, 0.7, 1.1), max_order=3)
    out = P.ir(d, 1, 4000, RATE)
    assert out.candidates == 3 + 6 + 12 and out.valid == [7]
    # the images are the source with every non-empty set of coordinates negated; each arrives once
    s, l = np.array([1.0, 1.5, 2.0]), np.array([2.0, 0.7, 1.1])
    d0 = np.linalg.norm(s - l)
    ks = sorted(int(np.floor((np.linalg.norm(s * sg - l) - d0) / 343.0 * RATE)) for sg in np.array(np.meshgrid([1, -1], [1, -1], [1, -1])).reshape(3, -1).T[1:])
    assert len(set(ks)) == 7 and all(out.acc[0, k] > 0 for k in ks)
    assert np.count_nonzero(out.acc[0]) == 1 + 2 * 7  # the direct sound on tap 0 alone, two taps per image


def test_two_parallel_planes_give_an_arithmetic_progression():
    """Planes x = -2 and x = 2.5 (4.5 m apart), source and listener on one line across them.  Two sequences per order, one
    starting at either wall, none void, all valid: 16 images.  On the line the images are known by hand -- every value
    is a short binary fraction, so the arithmetic is exact: among the images that start at one wall, those of odd order
    and those of even order each recede by 9 m per step, an arithmetic progression of delays (the flutter echo)."""
    d = P.describe([((1, 0, 0), -2.0, 0.9), ((-1, 0, 0), -2.5, 0.8)], (0.5, 0.0, 0.0), (-0.75, 0.0, 0.0), max_order=8)
    taps, d0 = 6000, 1.25
    out = P.ir(d, 1, taps, RATE)
    assert out.per_order == {k: 2 for k in range(1, 9)} and out.candidates == 16 and out.void == 0 and out.valid == [16]
    walls, refl = (-2.0, 2.5), (float(np.float32(0.9)), float(np.float32(0.8)))
    want = np.zeros(taps, np.int64)
    want[0] = 1 << 32  # the direct sound
    for first in (0, 1):
        x, Rr, dists = 0.5, 1.0, []
        for i in range(8):
            w = (i + first) % 2
            x = 2.0 * walls[w] - x
            Rr = Rr * refl[w]
            dist = abs(x + 0.75)
            dists.append(dist)
            pos = (dist - d0) / 343.0 * RATE
            k = int(np.floor(pos))
            f = pos - k
            v = Rr * d0 / max(dist, d0)
            assert k + 1 < taps
            want[k] += int(np.rint(v * (1.0 - f) * 2.0**32))
            want[k + 1] += int(np.rint(v * f * 2.0**32))
        assert (np.diff(dists[0::2]) == 9.0).all() and (np.diff(dists[1::2]) == 9.0).all()
    assert np.array_equal(out.acc[0], want)


def test_reciprocity():
    for planes, a, b, order in ((P.attic(), ATTIC_SRC, ATTIC_LIS, 4), (P.box_planes(ORIGIN, HALF, REFL), SRC, LIS, 3)):
        fwd = P.ir(P.describe(planes, a, b, max_order=order), 1, 4000, RATE)
        back = P.ir(P.describe(planes, b, a, max_order=order), 1, 4000, RATE)
        assert fwd.valid == back.valid and fwd.h.any()
        print(f"reciprocity, {len(planes)} planes: int64 sums bitwise equal {np.array_equal(fwd.acc, back.acc)}")
        assert rel_rms(back.h[0], fwd.h[0]) <= TOL and np.abs(back.h[0].astype(np.float64) - fwd.h[0]).max() <= TOL * np.abs(fwd.h[0]).max()


def test_candidate_counts():
    assert P.count(1, 0, 8) == {1: 1, 2: 0, 3: 0, 4: 0, 5: 0, 6: 0, 7: 0, 8: 0}
    assert P.count(7, 0, 3) == {1: 7, 2: 42, 3: 252} and sum(P.count(7, 0, 4).values()) == 1813
    assert P.count(7, 3, 4) == {3: 252, 4: 1512}
    assert sum(P.count(16, 0, 2).values()) == 256 and sum(P.count(16, 0, 3).values()) == 3856
    for Pn, K in ((1, 1), (2, 8), (3, 3), (7, 4), (16, 2)):
        seq = P.sequences(Pn, K)
        assert seq.shape == (Pn * (Pn - 1) ** (K - 1), K) and len({tuple(r) for r in seq}) == len(seq)
        assert (seq[:, 1:] != seq[:, :-1]).all() and seq.min() == 0 and seq.max() == Pn - 1
    one = P.ir(P.describe([((0, 1, 0), 0.0, 0.6)], (0.0, 3.0, 0.0), (8.0, 3.0, 0.0), max_order=8), 1, 400, RATE)
    assert one.candidates == 1 and one.valid == [1]
    sixteen = P.ir(P.describe(sixteen_planes(), ATTIC_SRC, ATTIC_LIS, max_order=2), 1, 4000, RATE)
    assert sixteen.candidates == 256 and sixteen.void + sixteen.valid[0] <= 256


def sixteen_planes():
    """A floor, a ceiling at 3.2 m and fourteen walls at uneven angles and distances of 3.5 to 4.5 m."""
    rng = np.random.default_rng(0)
    rows = [((0, 1, 0), 0.0, 0.8), ((0, -1, 0), -3.2, 0.8)]
    for i in range(14):
        th = 2 * np.pi * (i + rng.uniform(-0.2, 0.2)) / 14
        ap = rng.uniform(3.5, 4.5)
        rows.append(((-np.cos(th), 0.0, -np.sin(th)), -ap, 0.7 + 0.02 * (i % 10)))
    return rows
