"""gas_conv_ir_from_room_hrtf on the GPU: k_room_ir_hrtf against tests/room_brir_ref.py (float64, int64 sums), what is
bitwise, the direct sound's cell against gas_calc_spatialization's hrtf_dir, the generated IR in the convolver calls,
and the refusals.

Tolerance: helpers.TOL (1e-5), as relative RMS per channel and as max-abs relative to max|h|.  Device and reference
quantise the same float64 products to integers and choose the cell of every image by the same rule, so the expected
error is nothing at all wherever the two atan2 agree on the cell; tests/test_room_brir_reference.py requires of every
case used here that no image lies near a cell's edge (near_edge == 0).  Every comparison prints its figures (and
whether the taps are equal to the bit) before it asserts.  Measured on an MI355X: 0 and 0 on every shape, every
channel equal to the bit (profiles/room_brir_notes.md).  Each reference is computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest

import er_rooms_ref as E
import room_brir_cases as CS
import room_brir_ref as BR
import room_ir_ref as R
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

RATE = CS.RATE
F = 128
WORST = [0.0, 0.0]
SENTINEL = 0xDEADBEEF


def context(gas):
    return gas.SpatializerContext(max_sources=4, frames=F)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw(ctx, desc, hrir, n_az, n_el, hrir_taps, taps, out_taps, want_ir):
    """The call itself -> (status, *out_ir): out_ir keeps the sentinel where the library does not write it."""
    out = C.c_uint32(SENTINEL)
    d = None if desc is None else np.ascontiguousarray(desc)
    rc = ctx.lib.gas_conv_ir_from_room_hrtf(ctx.h, ptr(d), ptr(hrir), n_az, n_el, hrir_taps, taps, ptr(out_taps), C.byref(out) if want_ir else None)
    return rc, out.value


@pytest.mark.parametrize("name", list(CS.CASES))
def test_parity(gas, name):
    d, hrir, n_az, n_el, taps, ref = CS.reference(name)
    assert ref.near_edge == 0
    with context(gas) as ctx:
        h = ctx.conv_ir_from_room_hrtf(d, hrir, n_az, n_el, taps, want_taps=True, load=False)
    assert h.shape == (2, taps) and h.dtype == np.float32 and ref.h[0].any() and ref.h[1].any()
    for e in range(2):
        rms = rel_rms(h[e], ref.h[e])
        mx = np.abs(h[e].astype(np.float64) - ref.h[e]).max() / np.abs(ref.h[e]).max()
        WORST[0], WORST[1] = max(WORST[0], rms), max(WORST[1], mx)
        print(f"{name} ear {e}: rel rms {rms:.3g}, max abs / max|h| {mx:.3g}, bitwise {np.array_equal(h[e], ref.h[e])} (worst so far {WORST[0]:.3g}, {WORST[1]:.3g})")
        assert rms <= TOL and mx <= TOL, (name, e, rms, mx)


@pytest.mark.parametrize("grid,hrir_taps,min_order", [((12, 5), 1, 0), ((64, 16), 9, 0), ((1, 1), 256, 0), ((12, 5), 1, 3)])
def test_delta_set_is_the_one_channel_call_bitwise(gas, grid, hrir_taps, min_order):
    n_az, n_el = grid
    taps = 2048
    d = CS.describe(min_order=min_order)
    with context(gas) as ctx:
        mono = ctx.conv_ir_from_room(d, 1, taps, want_taps=True, load=False)
        h = ctx.conv_ir_from_room_hrtf(d, BR.delta_set(n_az * n_el, hrir_taps), n_az, n_el, taps, want_taps=True, load=False)
    assert mono.any()
    print(f"delta set {grid}, {hrir_taps} hrir taps, min_order {min_order}: left bitwise {h[0].tobytes() == mono[0].tobytes()}, right bitwise {h[1].tobytes() == mono[0].tobytes()}")
    assert h[0].tobytes() == mono[0].tobytes() and h[1].tobytes() == mono[0].tobytes()


def test_orders_add_up(gas):
    """Orders [0, 2] plus [3, inf) against [0, inf): exact in the integer sums, so with level 1 the float32 taps differ by
    their own final rounding at the most; the reference's integers say where they must be equal to the bit (taps that only
    one of the two parts reaches)."""
    d, hrir, n_az, n_el, taps, ref = CS.reference("2048 taps, 12x5, 32 hrir taps")
    early_ref = BR.brir(CS.describe(max_order=2), hrir, n_az, n_el, taps, RATE)
    tail_ref = BR.brir(CS.describe(min_order=3), hrir, n_az, n_el, taps, RATE)
    assert np.array_equal(early_ref.acc + tail_ref.acc, ref.acc)
    with context(gas) as ctx:
        whole = ctx.conv_ir_from_room_hrtf(d, hrir, n_az, n_el, taps, want_taps=True, load=False)
        early = ctx.conv_ir_from_room_hrtf(CS.describe(max_order=2), hrir, n_az, n_el, taps, want_taps=True, load=False)
        tail = ctx.conv_ir_from_room_hrtf(CS.describe(min_order=3), hrir, n_az, n_el, taps, want_taps=True, load=False)
    for got, want in ((whole, ref), (early, early_ref), (tail, tail_ref)):
        assert rel_rms(got, want.h) <= TOL
    only_early, only_tail = tail_ref.acc == 0, early_ref.acc == 0
    assert only_early.any() and only_tail.any()
    assert np.array_equal(whole[only_early], early[only_early]) and np.array_equal(whole[only_tail], tail[only_tail])
    # three float32 roundings of one exact sum: half an ulp of each
    slack = 2.0**-24 * (np.abs(early).astype(np.float64) + np.abs(tail) + np.abs(whole))
    assert (np.abs(early.astype(np.float64) + tail - whole) <= slack).all()


def test_two_calls_give_the_same_bits(gas):
    d, hrir, n_az, n_el, taps, _ = CS.reference("4096 taps, rotated, 16x7, 256 hrir taps")
    with context(gas) as ctx:
        a = ctx.conv_ir_from_room_hrtf(d, hrir, n_az, n_el, taps, want_taps=True, load=False)
        b = ctx.conv_ir_from_room_hrtf(d, hrir, n_az, n_el, taps, want_taps=True, load=False)
        d2 = d.copy()
        d2["ear_spacing"] = np.nan  # neither read nor validated
        d2["room"]["max_order"] = 77  # not read here either
        c = ctx.conv_ir_from_room_hrtf(d2, hrir, n_az, n_el, taps, want_taps=True, load=False)
    assert a.any() and a.tobytes() == b.tobytes() == c.tobytes()


def test_a_loading_call_leaves_the_generators_taps(gas):
    d, hrir, n_az, n_el, taps, ref = CS.reference("2048 taps, 12x5, 32 hrir taps")
    with context(gas) as ctx:
        pure = ctx.conv_ir_from_room_hrtf(d, hrir, n_az, n_el, taps, want_taps=True, load=False)
        buf = np.full((2, taps), np.nan, np.float32)
        assert raw(ctx, d, hrir, n_az, n_el, hrir.shape[2], taps, buf, True) == (-6, SENTINEL)  # GAS_ERR_UNSUPPORTED_CHAIN
        assert raw(ctx, d, hrir, n_az, n_el, hrir.shape[2], taps, None, True) == (-6, SENTINEL)
        assert np.isnan(buf).all()
        ctx.reserve_conv(1, taps)
        ir, loaded = ctx.conv_ir_from_room_hrtf(d, hrir, n_az, n_el, taps, want_taps=True)
        assert ir == 0 and ctx.conv_ir_get_info(ir) == (2, taps)
    assert pure.any() and pure.tobytes() == loaded.tobytes()
    assert rel_rms(pure, ref.h) <= TOL


@pytest.mark.parametrize("angles", CS.ORIENTATIONS)
def test_direct_sound_arrives_from_the_cell_of_hrtf_dir(gas, angles):
    """Every wall dead: only m = 0 is left, at tap 0 with a0 = 1 exactly.  The set holds (cell + 1) / 64 in tap 0 of both
    ears, so h[e][0] names the cell the call chose; gas_calc_spatialization names its own in the read-back parameters."""
    K = gas.capi
    n_az, n_el = CS.DIRECT_GRID
    basis = CS.rotation(*angles)
    d = CS.describe(CS.small_room(refl=(0,) * 6), listener_basis=basis)
    codes = np.zeros((n_az * n_el, 2, 4), np.float32)
    codes[:, :, 0] = ((np.arange(n_az * n_el) + 1) / 64.0)[:, None]
    want, near = CS.calc_spatialization_cell(CS.SRC, CS.LIS, d["listener"]["basis"][0], n_az, n_el)
    ref = BR.brir(d, codes, n_az, n_el, 64, RATE, orders=(0, 0))
    assert not near and ref.near_edge == 0 and int(ref.dirs[0]) == want
    cfgs = K.default_spat3d_config(1, hrtf_n_az=n_az, hrtf_n_el=n_el)
    poses = np.zeros(1, K.POSE_DTYPE)
    poses["position"][0] = CS.SRC
    poses["forward"][:, 2] = 1.0
    poses["pitch_scale"] = 1.0
    poses["max_db"] = 3.0
    listeners = np.zeros(1, K.LISTENER_DTYPE)
    listeners["basis"][0] = d["listener"]["basis"][0]
    listeners["origin"][0] = CS.LIS
    with context(gas) as ctx:
        ctx.hrtf_load(CS.noise_set(50, n_az * n_el, 256))
        slots = ctx.source_alloc_many(1, K.KIND_EFFECT, (K.FX_HRTF,))
        params = ctx.calc_spatialization(cfgs, poses, listeners, slots)
        h = ctx.conv_ir_from_room_hrtf(d, codes, n_az, n_el, 64, want_taps=True, load=False)
    got = [int(np.rint(float(h[e, 0]) * 64.0)) - 1 for e in range(2)]
    print(f"listener {angles}: hrtf_dir {int(params['hrtf_dir'][0])}, direct sound's cell {got}, reference {want}")
    assert h[0, 0] == codes[want, 0, 0] and h[1, 0] == codes[want, 1, 0] and not h[:, 1:].any()
    assert got[0] == got[1] == int(params["hrtf_dir"][0]) == want


def test_registered_ir_is_the_loaded_one_bitwise(gas):
    """3 F + 40 taps: four partitions, the last a partial one; four blocks of noise reach every partition."""
    taps = 3 * F + 40
    d, hrir = CS.describe(), CS.noise_set(31, 60, 256)
    rng = np.random.default_rng(11)
    with context(gas) as ctx:
        ctx.reserve_conv(2, 4 * F)
        made, h = ctx.conv_ir_from_room_hrtf(d, hrir, 12, 5, taps, want_taps=True)
        assert ctx.conv_ir_get_info(made) == (2, taps)
        loaded = ctx.conv_ir_load(h)
        assert (made, loaded) == (0, 1)
        convs = [ctx.conv_create(made), ctx.conv_create(loaded)]
        for _ in range(4):
            x = rng.uniform(-1, 1, (1, F, 2)).astype(np.float32)
            y = ctx.conv_process(convs, np.concatenate([x, x]))
            assert y[0].any() and y[0].tobytes() == y[1].tobytes()
        with pytest.raises(gas.capi.GasError):
            ctx.conv_ir_free(made)  # in use, as any IR
        for k in convs:
            ctx.conv_destroy(k)
        ctx.conv_ir_free(made)
        with pytest.raises(gas.capi.GasError) as ei:
            ctx.conv_ir_get_info(made)
        assert ei.value.status == -3
        assert ctx.conv_ir_from_room_hrtf(d, hrir, 12, 5, taps) == 0  # the lowest free id, as gas_conv_ir_load gives


def test_generated_ir_as_the_target_of_a_fade(gas):
    """State B of gas_conv_fade_to from a loaded two-channel IR; once the fade has ended the instance is bitwise a twin
    that was switched hard."""
    taps = 3 * F + 17
    rng = np.random.default_rng(12)
    dry_room = (rng.standard_normal((2, 50)) * 0.1).astype(np.float32)
    d, hrir = CS.describe(), CS.noise_set(32, 60, 64)
    with context(gas) as ctx:
        ctx.reserve_conv(2, 4 * F)
        a = ctx.conv_ir_load(dry_room)
        b = ctx.conv_ir_from_room_hrtf(d, hrir, 12, 5, taps)
        assert ctx.conv_ir_get_info(b) == (2, taps)
        fading, twin = ctx.conv_create(a), ctx.conv_create(a)
        ctx.conv_fade_to(fading, b, 0.0, 1.0, 2)
        for block in range(6):
            if block == 2:
                assert ctx.conv_fade_remaining(fading) == 0
                ctx.conv_set_ir(twin, b)
            x = rng.uniform(-1, 1, (1, F, 2)).astype(np.float32)
            y = ctx.conv_process([fading, twin], np.concatenate([x, x]))
            if block == 1:
                assert y[0].tobytes() != y[1].tobytes()  # half way: A and B mixed against A alone
            if block >= 2:
                assert y[0][:, 0].any() and y[0][:, 1].any() and y[0].tobytes() == y[1].tobytes()


def refusals():
    """(what, descriptor, hrir, n_az, n_el, hrir_taps, taps, with out_taps, with out_ir) under a reserve of 4096 taps."""
    ok = CS.describe()
    hrir = CS.noise_set(41, 60, 32)
    good = (hrir, 12, 5, 32)

    def room(**kw):
        d = ok.copy()
        for k, v in kw.items():
            d["room"][k] = v
        return d

    def desc(**kw):
        d = ok.copy()
        for k, v in kw.items():
            d[k] = v
        return d

    def listener(**kw):
        d = ok.copy()
        for k, v in kw.items():
            d["listener"][k] = v
        return d

    def bad_value(v, at):
        h = hrir.copy()
        h[at] = v
        return h

    nan_basis = np.eye(3, dtype=np.float32)
    nan_basis[1, 2] = np.nan
    cube = R.describe(E.unit_room(half_extent=(0.5, 0.5, 0.5)), (0.25, 0.0, 0.0), (-0.25, 0.0, 0.0))
    cube323 = cube.copy()
    cube323["max_order"] = 323
    yield ("NULL descriptor", None) + good + (256, True, True)
    yield ("neither output", ok) + good + (256, False, False)
    yield ("no taps", ok) + good + (0, True, True)
    yield ("more taps than the reserve", ok) + good + (4097, True, True)
    yield ("more taps than 2^20 for the pure generator", ok) + good + ((1 << 20) + 1, True, False)
    yield ("half extent 0", room(half_extent=(2.5, 0.0, 1.5))) + good + (256, True, True)
    yield ("half extent inf", room(half_extent=(2.5, np.inf, 1.5))) + good + (256, True, True)
    yield ("speed of sound 0", room(speed_of_sound=0.0)) + good + (256, True, True)
    yield ("level < 0", room(level=-0.5)) + good + (256, True, True)
    yield ("level inf", room(level=np.inf)) + good + (256, True, True)
    yield ("reflectance > 1", room(reflectance=(0.9, 1.5, 0.8, 0.8, 0.8, 0.8))) + good + (256, True, True)
    yield ("reflectance nan", room(reflectance=(0.9, np.nan, 0.8, 0.8, 0.8, 0.8))) + good + (256, True, True)
    yield ("min_order > max_order", desc(min_order=4, max_order=3)) + good + (256, True, True)
    yield ("source nan", desc(source=(1.0, np.nan, 0.25))) + good + (256, True, True)
    yield ("listener origin inf", listener(origin=(np.inf, 0.0, 0.0))) + good + (256, True, True)
    yield ("listener basis nan", listener(basis=nan_basis)) + good + (256, True, True)
    yield ("room basis nan", room(basis=nan_basis)) + good + (256, True, True)
    yield ("room origin nan", room(origin=(0.0, 0.0, np.nan))) + good + (256, True, True)
    yield ("source outside", desc(source=(2.6, 0.5, 0.25))) + good + (256, True, True)
    yield ("listener outside", listener(origin=(-1.0, 0.25, -1.6))) + good + (256, True, True)
    yield ("source at the listener", desc(source=CS.LIS)) + good + (256, True, True)
    yield ("d0 below a millimetre", desc(source=(CS.LIS[0] + 5e-4, CS.LIS[1], CS.LIS[2]))) + good + (256, True, True)
    yield ("box over the cap", cube) + good + (1 << 20, True, False)
    yield ("box over the cap with a max_order", cube323) + good + (1 << 20, True, False)
    yield ("NULL hrir", ok, None, 12, 5, 32, 256, True, True)
    yield ("n_az 0", ok, hrir, 0, 5, 32, 256, True, True)
    yield ("n_el 0", ok, hrir, 12, 0, 32, 256, True, True)
    yield ("more than 65 536 directions", ok, hrir, 257, 256, 32, 256, True, True)  # refused before the set is read
    yield ("n_az n_el wraps in 32 bits", ok, hrir, 1 << 16, 1 << 16, 32, 256, True, True)
    yield ("hrir_taps 0", ok, hrir, 12, 5, 0, 256, True, True)
    yield ("hrir_taps 257", ok, hrir, 12, 5, 257, 256, True, True)
    yield ("hrir nan", ok, bad_value(np.nan, (59, 1, 31)), 12, 5, 32, 256, True, True)
    yield ("hrir inf", ok, bad_value(-np.inf, (0, 0, 0)), 12, 5, 32, 256, True, True)
    yield ("hrir above 4", ok, bad_value(4.5, (17, 1, 3)), 12, 5, 32, 256, True, True)
    yield ("hrir below -4", ok, bad_value(-4.000001, (17, 0, 3)), 12, 5, 32, 256, True, True)


def test_refusals_change_nothing(gas):
    ok = CS.describe()
    hrir = CS.noise_set(41, 60, 32)
    with context(gas) as ctx:
        ctx.reserve_conv(2, 4096)
        first = ctx.conv_ir_from_room_hrtf(ok, hrir, 12, 5, 256)
        assert first == 0
        for what, d, h, n_az, n_el, hrir_taps, taps, with_taps, with_ir in refusals():
            buf = np.full((2, max(taps, 1)), np.nan, np.float32) if with_taps else None
            rc, ir = raw(ctx, d, h, n_az, n_el, hrir_taps, taps, buf, with_ir)
            assert rc == -1, (what, rc)
            assert ir == SENTINEL, what
            assert buf is None or np.isnan(buf).all(), what
        edge = hrir.copy()
        edge[5, 1, 7], edge[6, 0, 0] = 4.0, -4.0  # the bound itself is allowed
        assert ctx.conv_ir_from_room_hrtf(ok, edge, 12, 5, 256) == 1
        ctx.conv_ir_free(1)
        assert ctx.lib.gas_conv_ir_from_room_hrtf(None, ptr(np.ascontiguousarray(ok)), ptr(hrir), 12, 5, 32, 256, None, C.byref(C.c_uint32())) == -1
        assert ctx.conv_ir_load(np.ones((1, 4), np.float32)) == 1  # the id it would have had: the table is as it was
        assert ctx.conv_ir_get_info(first) == (2, 256)
        with pytest.raises(gas.capi.GasError) as ei:
            ctx.conv_ir_get_info(2)
        assert ei.value.status == -3
