"""gas_calc_early_reflections on the GPU: k_calc_er against tests/er_rooms_ref.py (float64), its edges, what it writes and
what it refuses.

Parity.  A source outside the reference's near-tie set must come out tap for tap: gains within GAIN_RTOL = 3e-5 (zeros
exactly), delays equal, except that a tap whose reference fr lies within 0.01 frames of k + 0.5 may be one off.  A
near-tie source (two of its nine largest gains closer than 1e-4 relative, or a candidate at the ring's reach) may order
or select differently: its eight gains, sorted, must still agree within GAIN_RTOL, and each of its taps must be one of the
reference's 24 candidates.  Both bands come from er_rooms_ref's docstring, not from this kernel.

The tie-break of rule 7 cannot be seen in the values of exactly tied candidates (the same gain, the same delay): what the
tie case pins is that the ranks stay a permutation -- all eight taps written, none twice, none left as published."""
import ctypes as C

import numpy as np
import pytest

import er_ref
import er_rooms_ref as R
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

ER, HRTF = 2, 3
RATE, F, RING = 48000.0, 512, 4096
N_MAX = 4000
SMALL = [1, 2, 3, 7, 8, 9, 63, 64, 65, 257]  # source-group (1), wave (2) and workgroup (8) edges, several workgroups
PEAK_TOL = dict(rtol=2e-5, atol=1e-7)  # test_gpu_er_edges.py's


@pytest.fixture(scope="module")
def ctx(gas):
    with gas.SpatializerContext(max_sources=N_MAX + 8, frames=F, er_ring_frames=RING) as c:
        c.test_slots = c.source_alloc_many(N_MAX, gas.capi.KIND_EFFECT, (ER,))
        yield c


def poses_of(K, pos):
    """Only `position` is read: every other field is NaN."""
    p = np.zeros(len(pos), K.POSE_DTYPE)
    for f in ("volume_db", "velocity", "max_db", "forward", "pitch_scale"):
        p[f] = np.nan
    p["position"] = pos
    return p


def listener_of(K, origin):
    """Only `origin` is read."""
    l = np.zeros(1, K.LISTENER_DTYPE)
    l["basis"], l["velocity"], l["pad"] = np.nan, np.nan, np.nan
    l["origin"] = origin
    return l


def read_rows(K, c, slots):
    """The slots' whole rows, through gas_calc_spatialization's out_params (a config without a grid: it leaves hrtf_*, the
    shelf and the early-reflection fields as they are)."""
    poses = np.zeros(len(slots), K.POSE_DTYPE)
    poses["pitch_scale"] = 1.0
    lis = np.zeros(1, K.LISTENER_DTYPE)
    lis["basis"] = np.eye(3)
    return c.calc_spatialization(K.default_spat3d_config(), poses, lis, slots)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw(ctx, rooms, n_rooms, ri, poses, lis, slots, n, out, mem=0):
    return ctx.lib.gas_calc_early_reflections(ctx.h, _ptr(rooms), n_rooms, _ptr(ri), _ptr(poses), _ptr(lis), _ptr(slots), n, _ptr(out), mem)


def generate(gas, ctx, rooms, ri, pos, lis, slots, mem="host"):
    K = gas.capi
    rooms = np.ascontiguousarray(rooms, dtype=K.ROOM_DTYPE)
    poses, listener = poses_of(K, pos), listener_of(K, lis)
    if mem == "host":
        return ctx.calc_early_reflections(rooms, poses, listener, slots=slots, room_index=ri)
    import torch

    n = len(poses)
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    d_out = torch.full((n * K.ER_TAPS_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sl = None if slots is None else np.ascontiguousarray(slots, dtype=np.uint32)
    rix = None if ri is None else np.ascontiguousarray(ri, dtype=np.uint32)
    rc = ctx.lib.gas_calc_early_reflections(ctx.h, _ptr(rooms), len(rooms), _ptr(rix), C.c_void_p(d_poses.data_ptr()), _ptr(listener), _ptr(sl), n, C.c_void_p(d_out.data_ptr()), K.MEM_DEVICE)
    assert rc == 0, rc
    return d_out.cpu().numpy().view(K.ER_TAPS_DTYPE).copy()


def tap_is_a_candidate(t, i, gain, delay):
    if gain == 0:
        return delay == 1
    close = np.abs(t.g_all[i] - gain) <= R.GAIN_RTOL * t.g_all[i]
    slack = np.where(R.frac_border(t.fr_all[i]), 1, 0)
    return bool(np.any(close & (t.g_all[i] > 0) & (np.abs(t.delay_all[i] - delay) <= slack)))


def check_parity(got, t, what, firm_all=False):
    """got: ER_TAPS_DTYPE [n]; t: er_rooms_ref.Taps.  firm_all: near ties are exact ties here, compare them tap for tap too."""
    gain, delay = got["gain"].astype(np.float64), got["delay"].astype(np.int64)
    assert np.all(np.isfinite(gain)) and np.all(delay >= 1) and np.all(delay <= RING - F), what
    firm = np.ones(len(gain), bool) if firm_all else ~t.near_tie
    live = t.gain[firm] > 0
    rel = np.abs(gain[firm][live] - t.gain[firm][live]) / t.gain[firm][live]
    diff = delay[firm] - t.delay[firm]
    off = diff != 0
    print(f"{what}: {firm.sum()} firm of {len(gain)} sources, max rel gain error {rel.max() if rel.size else 0.0:.3e}, {off.sum()} delays one off of {t.border[firm].sum()} border taps")
    np.testing.assert_allclose(gain[firm], t.gain[firm], rtol=R.GAIN_RTOL, atol=0, err_msg=what)
    assert np.all(np.abs(diff[off]) == 1) and np.all(t.border[firm][off]), what
    for i in np.flatnonzero(~firm):
        np.testing.assert_allclose(np.sort(gain[i]), np.sort(t.gain[i]), rtol=R.GAIN_RTOL, atol=0, err_msg=f"{what} near-tie source {i}")
        assert all(tap_is_a_candidate(t, i, gain[i, k], delay[i, k]) for k in range(8)), f"{what} near-tie source {i}"


_SCENES = {}


def scene(n, mode):
    """(rooms, room_index or None, positions, listener origin, reference taps), computed once per (n, mode)."""
    if (n, mode) not in _SCENES:
        rng = np.random.default_rng(1000 * n + len(mode))
        if mode == "null":  # room_index NULL: room 0 for everybody
            rooms, ri, pos, lis = R.scene(rng, n, n_rooms=1)
            ri = None
        else:
            rooms, ri, pos, lis = R.scene(rng, n, n_rooms=8, with_none=0.25 if mode == "none" else 0.0)
            if mode == "none":
                ri[0] = R.ROOM_NONE
        _SCENES[(n, mode)] = (rooms, ri, pos, lis, R.taps(rooms, pos, lis, RATE, F, RING, ri))
    return _SCENES[(n, mode)]


CASES = [(N_MAX, m) for m in ("null", "mixed", "none")] + [(n, ("null", "mixed", "none")[i % 3]) for i, n in enumerate(SMALL)] + [(1, "mixed"), (9, "none"), (65, "null")]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("n,mode", CASES, ids=[f"n{n}_{m}" for n, m in CASES])
def test_parity_with_the_float64_reference(gas, ctx, n, mode, mem):
    rooms, ri, pos, lis, t = scene(n, mode)
    if n == N_MAX:  # the scene must be worth comparing
        assert (~t.near_tie).mean() > 0.98 and t.border.sum() > 100
        assert (t.gain[:, 7] > 0).mean() > 0.5 if mode != "none" else (t.outside.sum() > 500 and (~t.outside).sum() > 2000)
    got = generate(gas, ctx, rooms, ri, pos, lis, ctx.test_slots[:n], mem)
    check_parity(got, t, f"n {n} {mode} {mem}")


def _edge_cases():
    a, b = [1.3, -0.4, 0.9], [-0.7, 0.6, -1.1]
    two_dead = R.unit_room()
    two_dead["reflectance"] = [[0.0, 0.8, 0.8, 0.0, 0.8, 0.8]]
    cube = R.unit_room(half_extent=(3, 3, 3), reflectance=0.7)
    return {
        # name: (room, source, listener, what the reference must say about it)
        "source_outside": (R.unit_room(), [4.5, 0, 0], b, lambda t: t.outside[0] and not t.gain.any()),
        "listener_outside": (R.unit_room(), a, [0, 0, -3.25], lambda t: t.outside[0] and not t.gain.any()),
        "source_on_a_wall": (R.unit_room(), [4.0, 0.3, -0.7], b, lambda t: not t.outside[0] and t.delay_all[0, 5] == 1 and t.fr_all[0, 5] == 0 and t.g_all[0, 5] > 0.79),
        "source_at_the_listener": (R.unit_room(), a, a, lambda t: t.d0[0] == 0 and not t.gain.any()),
        "room_5cm": (R.unit_room(half_extent=(0.025, 0.02, 0.015)), [0.01, -0.004, 0.006], [-0.012, 0.007, -0.003], lambda t: np.all(t.gain > 0) and t.delay.max() <= 20 and not t.border.any()),
        "room_1mm": (R.unit_room(half_extent=(0.0005, 0.0004, 0.0003)), [0.00021, -0.00013, 0.00008], [-0.00033, 0.00017, -0.00011], lambda t: np.all(t.gain > 0) and np.all(t.delay == 1) and t.fr.max() < 0.49),
        "room_400m": (R.unit_room(half_extent=(200, 200, 200)), a, b, lambda t: not t.outside[0] and not t.gain.any() and np.all(np.rint(t.fr_all) > RING - F)),
        "two_dead_walls": (two_dead, a, b, lambda t: (t.g_all[0] == 0).sum() == 13 and np.all(t.gain > 0)),
        "level_0": (R.unit_room(level=0.0), a, b, lambda t: not t.outside[0] and not t.gain.any()),
        "max_order_1": (R.unit_room(max_order=1), a, b, lambda t: np.all(t.gain[0, :6] > 0) and not t.gain[0, 6:].any() and sorted(t.cand[0, :6]) == list(range(6))),
        # identity basis, cube, source at the centre, listener on the x axis, equal walls: the +-y and +-z images tie bit
        # for bit (candidates 1, 2, 3, 4), and so do the second-order ones in fours and pairs: taps 6 and 7 are the first two
        # of the four tied candidates 19 .. 22
        "exact_ties": (cube, [0, 0, 0], [1.25, 0, 0], lambda t: len(set(t.g_all[0, 1:5])) == 1 and list(t.cand[0]) == [5, 1, 2, 3, 4, 0, 19, 20] and len(set(t.g_all[0, 19:23])) == 1),
    }


@pytest.mark.parametrize("name", list(_edge_cases()))
def test_edges(gas, ctx, name):
    K = gas.capi
    room, pos, lis, expect = _edge_cases()[name]
    t = R.taps(room, [pos], lis, RATE, F, RING)
    assert expect(t), name  # the case is what it says
    assert name == "exact_ties" or not (t.gap < R.NEAR_TIE).any()
    slot = ctx.test_slots[:1]
    row = np.zeros(1, K.PARAMS_DTYPE)  # what the launch must replace, all of it
    row["er_gain"], row["er_delay"] = -77.0, 4242
    ctx.params_publish_batch(slot, row)
    got = generate(gas, ctx, room, None, [pos], lis, slot)
    assert not np.any(got["gain"] == -77.0) and not np.any(got["delay"] == 4242)
    check_parity(got, t, name, firm_all=True)
    assert not t.border.any()  # so every delay is the reference's
    np.testing.assert_array_equal(got["delay"], t.delay)
    # the row holds what out_taps holds
    back = read_rows(K, ctx, slot)
    np.testing.assert_array_equal(back["er_gain"], got["gain"])
    np.testing.assert_array_equal(back["er_delay"], got["delay"])


def _sentinel_rows(K, n):
    row = np.zeros(n, K.PARAMS_DTYPE)
    row["mix_volumes"] = 0.125
    row["pitch_scale"], row["linear_attenuation"], row["attenuation_filter_cutoff_hz"] = 1.5, 0.375, 1234.0
    row["hrtf_gain"], row["hrtf_dir"] = 0.625, 11
    row["fx_shelf_gain"], row["fx_shelf_cutoff_hz"] = 0.4375, 4321.0
    row["er_gain"] = -0.0625 * np.arange(1, 9)
    row["er_delay"] = 100 + np.arange(8)
    return row


def test_only_the_two_fields_are_written(gas):
    """Rows published with sentinels; the generator's launch; then gas_calc_spatialization (a config without a grid, so
    it leaves hrtf_* alone) hands the whole rows back: er_* are the generated taps, the shelf and hrtf sentinels are
    intact.  A later publish replaces the generated fields.  A slot that only ever got taps has no parameters."""
    K = gas.capi
    n = 9
    rooms, ri, pos, lis, t = scene(n, "mixed")
    with gas.SpatializerContext(max_sources=n + 1, frames=F, er_ring_frames=RING) as c:
        slots = c.source_alloc_many(n, K.KIND_EFFECT, (ER,))[::-1].copy()  # not the identity
        rows = _sentinel_rows(K, n)
        c.params_publish_batch(slots, rows)
        taps = generate(gas, c, rooms, ri, pos, lis, slots)
        check_parity(taps, t, "rows")
        assert (taps["gain"] > 0).any()
        back = read_rows(K, c, slots)
        np.testing.assert_array_equal(back["er_gain"], taps["gain"])
        np.testing.assert_array_equal(back["er_delay"], taps["delay"])
        for f in ("hrtf_gain", "hrtf_dir", "fx_shelf_gain", "fx_shelf_cutoff_hz"):
            np.testing.assert_array_equal(back[f], rows[f], err_msg=f)
        c.params_publish_batch(slots, rows)
        back = read_rows(K, c, slots)
        np.testing.assert_array_equal(back["er_gain"], rows["er_gain"])
        np.testing.assert_array_equal(back["er_delay"], rows["er_delay"])
        fresh = c.source_alloc_many(1, K.KIND_EFFECT, (ER,))
        generate(gas, c, rooms[:1], None, pos[:1], lis, fresh)
        with pytest.raises(gas.GasError) as ei:
            c.process_block(np.zeros((1, F, 2), np.float32), fresh)
        assert ei.value.status == -12  # GAS_ERR_NO_PARAMS


def test_without_slots_it_is_a_pure_generator(gas):
    K = gas.capi
    n = 65
    rooms, ri, pos, lis, t = scene(n, "none")
    with gas.SpatializerContext(max_sources=n, frames=F, er_ring_frames=RING) as c:
        slots = c.source_alloc_many(n, K.KIND_EFFECT, (ER,))
        rows = _sentinel_rows(K, n)
        c.params_publish_batch(slots, rows)
        for mem in ("host", "device"):
            free = generate(gas, c, rooms, ri, pos, lis, None, mem)
            check_parity(free, t, f"slot-less {mem}")
            back = read_rows(K, c, slots)
            np.testing.assert_array_equal(back["er_gain"], rows["er_gain"])
            np.testing.assert_array_equal(back["er_delay"], rows["er_delay"])
        bound = generate(gas, c, rooms, ri, pos, lis, slots)
        assert bound.tobytes() == free.tobytes()


@pytest.mark.parametrize("chain", [(ER,), (ER, HRTF)], ids=["er", "er_hrtf"])
def test_generated_taps_drive_the_effect(gas, chain):
    """F = 256, ring 1024: three sources move through a room over four callbacks, taps generated into their rows before
    each.  The output is er_ref.ErBank's fed the returned taps; through [ER, HRTF] with a unit-impulse HRIR and hrtf_gain 1
    both ears carry (yl + yr) / 2 times the HRTF stage's ramp (0 -> 1 over the first callback), as in test_gpu_er_edges.py."""
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    f, ring, n, T = 256, 1024, 3, 4
    rng = np.random.default_rng(5)
    room = R.unit_room(half_extent=(2.0, 1.5, 1.8))
    lis = [0.4, -0.3, 0.2]
    start = np.array([[-1.6, 1.0, -1.2], [1.5, -1.1, 0.3], [0.2, 0.9, 1.4]])
    step = np.array([[0.35, -0.2, 0.3], [-0.4, 0.25, -0.1], [0.1, -0.3, -0.35]])
    with gas.SpatializerContext(max_sources=n, frames=f, er_ring_frames=ring) as c:
        if HRTF in chain:
            h = np.zeros((16, 2, 256), np.float32)
            h[:, :, 0] = 1.0
            c.hrtf_load(h)
        slots = c.source_alloc_many(n, K.KIND_EFFECT, chain)
        p = synth.draw_params(rng, n, dirs=16, ring_frames=ring, frames=f)
        p["hrtf_gain"] = 1.0
        c.params_publish_batch(slots, p)
        bank = er_ref.ErBank(n, f, ring)
        seen = set()
        for b in range(T):
            pos = start + b * step
            taps = generate(gas, c, room, None, pos, lis, slots)
            t = R.taps(room, pos, lis, RATE, f, ring)
            check_parity(taps, t, f"callback {b}")
            assert (taps["gain"] > 0).sum() >= 12 and taps["delay"].max() <= ring - f
            seen.add(taps.tobytes())
            x = synth.draw_sources(rng, n, f)
            mix, pk = c.process_block(x, slots)
            q = np.zeros(n, K.PARAMS_DTYPE)
            q["er_gain"], q["er_delay"] = taps["gain"], taps["delay"]
            rows = bank.block(q, x)
            if HRTF in chain:
                mono = rows.mean(axis=2)
                if b == 0:
                    mono = mono * (np.arange(f, dtype=np.float64) / f)[None, :]
                rows = np.stack([mono, mono], axis=2)
            e = rel_rms(mix[0], rows.sum(axis=0))
            assert e <= TOL, f"callback {b}: mix rel rms {e:.3e}"
            np.testing.assert_allclose(pk, np.abs(rows).max(axis=1), err_msg=f"callback {b}", **PEAK_TOL)
        assert len(seen) == T  # the taps moved with the sources


def test_argument_checks(gas, ctx):
    """Every refusal leaves out_taps and the rows as they were, and the valid call after it gives what it gave before."""
    K = gas.capi
    n = 7
    rooms, ri, pos, lis, t = scene(n, "mixed")
    rooms = np.ascontiguousarray(rooms, dtype=K.ROOM_DTYPE)
    poses, listener = poses_of(K, pos), listener_of(K, lis)
    slots = np.ascontiguousarray(ctx.test_slots[:n], dtype=np.uint32)
    good = generate(gas, ctx, rooms, ri, pos, lis, slots)
    check_parity(good, t, "before the refusals")
    INVALID, BAD_SLOT = -1, -3

    def refused(want, rooms_=rooms, n_rooms=None, ri_=ri, poses_=poses, lis_=listener, slots_=slots, n_=n, out=True, mem=0, handle=None):
        buf = np.full(n, 0x5A, np.uint8).repeat(64).view(K.ER_TAPS_DTYPE) if out else None
        keep = None if buf is None else buf.copy()
        h = ctx.h if handle is None else handle
        rc = ctx.lib.gas_calc_early_reflections(h, _ptr(rooms_), len(rooms) if n_rooms is None else n_rooms, _ptr(ri_), _ptr(poses_), _ptr(lis_), _ptr(slots_), n_, _ptr(buf), mem)
        assert rc == want, (rc, want)
        assert buf is None or buf.tobytes() == keep.tobytes()
        again = generate(gas, ctx, rooms, ri, pos, lis, None)  # (the rows are read back at the end)
        assert again.tobytes() == good.tobytes()

    refused(INVALID, handle=C.c_void_p(None))
    refused(INVALID, rooms_=None)
    refused(INVALID, poses_=None)
    refused(INVALID, lis_=None)
    refused(INVALID, slots_=None, out=False)
    refused(INVALID, mem=2)
    refused(INVALID, n_rooms=0)
    refused(INVALID, rooms_=np.resize(rooms, K.MAX_ROOMS + 1), n_rooms=K.MAX_ROOMS + 1)
    refused(INVALID, n_=ctx.max_sources + 1)
    for bad in (len(rooms), 0xFFFFFFFE):
        r2 = ri.copy()
        r2[n - 1] = bad
        refused(INVALID, ri_=r2)
    twice = slots.copy()
    twice[n - 1] = twice[0]
    refused(INVALID, slots_=twice)
    for field, idx, values in (("half_extent", 1, (0.0, -1.0, np.nan, np.inf)), ("speed_of_sound", None, (0.0, -343.0, np.nan, np.inf)), ("level", None, (-0.5, np.nan, np.inf)), ("reflectance", 4, (-0.01, 1.01, np.nan)), ("max_order", None, (0, 3))):
        for v in values:
            r2 = rooms.copy()
            if idx is None:
                r2[field][len(rooms) - 1] = v
            else:
                r2[field][len(rooms) - 1, idx] = v
            refused(INVALID, rooms_=r2)
    unused = slots.copy()
    unused[2] = N_MAX + 3  # never allocated
    refused(BAD_SLOT, slots_=unused)
    unused[2] = ctx.max_sources
    refused(BAD_SLOT, slots_=unused)
    assert raw(ctx, rooms, len(rooms), ri, poses, listener, slots, 0, None) == 0  # n == 0, and nothing to write to
    back = read_rows(K, ctx, slots)
    np.testing.assert_array_equal(back["er_gain"], good["gain"])
    np.testing.assert_array_equal(back["er_delay"], good["delay"])
    with gas.SpatializerContext(max_sources=n, frames=F, er_ring_frames=0) as c0:  # no ring: no effect to feed
        s0 = c0.source_alloc_many(n, K.KIND_3D_MIX)
        out = np.zeros(n, K.ER_TAPS_DTYPE)
        assert raw(c0, rooms, len(rooms), ri, poses, listener, s0, n, out) == INVALID
        assert raw(c0, rooms, len(rooms), ri, poses, listener, None, n, out) == INVALID
        assert not out.view(np.uint8).any()
