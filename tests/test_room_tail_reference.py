"""gas_conv_ir_from_room_diffuse and gas_conv_ir_from_room_hrtf_diffuse without a GPU: tests/room_tail_ref.py against the
rule's check vectors, its marks and weights, what the rule makes bitwise, the statistics of the diffuse part, the cases
tests/test_gpu_room_tail.py compares (tests/room_tail_cases.py), gas_room_tail's C layout and the two exports.

The two statistical bounds are derived, not fitted.  Pure diffuse taps are h / (level s0) = xi[k] (1 - f[k]) +
xi[k - 1] f[k - 1] with xi of unit variance and f uniform on (0, 1): variance E[(1 - f)^2] + E[f^2] = 2/3.  The
estimate over a window of 4096 taps scatters by about sqrt(2 / 4096) (1 + the neighbours' correlation), 2 - 3 %; the bound
of 15 % is five of those.  Measured with the seeds below, both ears, 16 windows each: 5.8 % at the worst.  With rho < 1
the energy falls as exp(-(mu r_k)), r_k = d0 + c k / rate, so the logarithm of a window's variance falls by mu c per
second; a least-squares line through 16 windows that each scatter by 3 % over a fall of several nepers is off by well
under 1 %, measured 0.1 % at the worst; the bound is 10 %."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import room_bands_cases as BC
import room_bands_ref as BD
import room_tail_cases as TC
import room_tail_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = TC.RATE
SEEDS = (0, 1, 7, 0xFFFFFFFF)
WINDOW, WINDOWS = 4096, 16


# ------------------------------------------------------------------------------------------------------ steps 1 and 4
@pytest.mark.parametrize("seed,e,k,z,num", [(1, 0, 0, 0xC42C5A1AA3820138, -66133), (1, 0, 1, 0x204391A6FD59956F, 84191), (0, 1, 5, 0x554B78B0C52407ED, -29819), (0xFFFFFFFF, 1, (1 << 20) - 1, 0x5E823BEAA35DC300, 17553)])
def test_check_vectors(seed, e, k, z, num):
    assert T.hash_scalar(seed, e, k) == z
    zs = T.hash_taps(seed, e, k + 1)
    assert int(zs[k]) == z  # the vectorised uint64 form wraps as the integers do
    assert int(T.numerator(zs)[k]) == num and num % 2 != 0
    xi, f = T.noise(seed, e, k + 1)
    assert xi[k] == num / np.sqrt(65536.0**2 - 1.0) and f[k] == ((z >> 48) + 0.5) / 65536.0 and 0.0 < f[k] < 1.0


def test_noise_has_unit_variance_by_construction():
    """u uniform on 0 .. 65535 has variance (65536^2 - 1) / 12; the numerator is 2 (sum of three) - 3 * 65535."""
    u = np.arange(65536, dtype=np.float64)
    var_u = float(np.mean((u - 32767.5) ** 2))
    assert var_u == (65536.0**2 - 1.0) / 12.0
    assert 4.0 * 3.0 * var_u / T.XI_DEN**2 == pytest.approx(1.0, abs=1e-15)


def test_weights_are_power_complementary():
    for k0, k1, taps in ((0, 0, 10), (3, 3, 10), (0, 777, 1000), (250, 330, 4096), (100, 200, 200)):
        ws, wd = T.weights(k0, k1, taps)
        assert np.abs(ws * ws + wd * wd - 1.0).max() <= np.finfo(np.float64).eps, (k0, k1)
        assert (ws[:k0] == 1.0).all() and (wd[:k0] == 0.0).all() and (ws[k1:] == 0.0).all() and (wd[k1:] == 1.0).all()
        if k1 > k0:
            assert ws[k0] == 1.0 and wd[k0] == 0.0 and 0.0 < wd[k1 - 1] < 1.0
            assert (np.diff(wd[k0:k1]) > 0).all()


def test_marks():
    assert T.marks(TC.tail(100, 0), 1000, RATE) == (100, 100)  # fade 0: a hard switch
    assert T.marks(TC.tail(1000, 10), 1000, RATE) == (1000, 1000)  # K0 == taps
    assert T.marks(TC.tail(5000, 10), 1000, RATE) == (1000, 1000)
    assert T.marks(TC.tail(900, 500), 1000, RATE) == (900, 1000)
    assert T.marks(T.describe(0, 3.0e38, 3.0e38), 1 << 20, RATE) == (1 << 20, 1 << 20)  # the clamp to 2^31 comes first
    # a .5 tie goes to the even mark, as llrint does: 0.5 and 1.5 taps at a rate of 1, 2.5 taps at a rate of 2
    assert T.marks(T.describe(0, 0.5, 0.0), 10, 1.0) == (0, 0)
    assert T.marks(T.describe(0, 1.5, 0.0), 10, 1.0) == (2, 2)
    assert T.marks(T.describe(0, 1.25, 1.25), 10, 2.0) == (2, 4)
    assert T.marks(T.describe(0, 0.0, 1.75), 10, 2.0) == (0, 4)


# ------------------------------------------------------------------------------------------------------ what is bitwise
def test_case_marks_are_what_the_names_say():
    for name, (make, want) in TC.CASES.items():
        d, bands, t, channels, taps = make()
        assert T.marks(t, taps, RATE) == want, name
    assert T.marks(TC.hrtf_reference()[2], TC.HRTF_TAPS, RATE) == TC.HRTF_MARKS


@pytest.mark.parametrize("name", list(TC.CASES))
def test_cases_are_not_silent(name):
    d, bands, t, channels, taps, ref = TC.reference(name)
    assert ref.h.shape == (channels, taps) and np.isfinite(ref.h).all()
    for e in range(channels):
        assert ref.h[e].any(), (name, e)
    if ref.K1 < taps and channels == 2:
        assert not np.array_equal(ref.h[0, ref.K1 :], ref.h[1, ref.K1 :])  # the ears' diffuse parts differ
    assert np.abs(ref.acc).max() < 1 << 62


def test_hrtf_cases():
    for delta in (False, True):
        d, bands, t, hrir, n_az, n_el, taps, ref = TC.hrtf_reference(delta)
        assert ref.near_edge == 0 and ref.h[0].any() and ref.h[1].any()
        assert (ref.K0, ref.K1) == TC.HRTF_MARKS
    # through unit-impulse HRIRs the specular part is the one-channel sums in both ears
    mono = T.ir(d, bands, t, 1, taps, RATE)
    assert np.array_equal(ref.spec[:, 0], mono.spec[:, 0]) and np.array_equal(ref.spec[:, 1], mono.spec[:, 0])
    assert not np.array_equal(ref.h[0, ref.K1 :], ref.h[1, ref.K1 :])


def test_specular_sums_of_a_k1_tap_lattice_are_the_full_lattice_below_k1():
    """Step 2's claim: the lattice passes run as for an IR of K1 taps."""
    d, bands, t, channels, taps, ref = TC.reference("B 3, L 255, 4096 taps, marks across a tile's and two waves' ends, air on one band")
    full = BD.ir(d, bands, channels, taps, RATE)
    assert ref.K1 == 330 and np.array_equal(ref.spec, full.acc[:, :, : ref.K1])


def test_k0_at_taps_is_the_bands_call_bitwise():
    d, bands, t, channels, taps, ref = TC.reference("B 3, L 255, 200 taps, K0 == taps")
    want = BD.ir(d, bands, channels, taps, RATE)
    assert np.array_equal(ref.acc, want.acc) and ref.h.tobytes() == want.h.tobytes()


def test_gain_0_is_silent_from_k1_plus_d():
    d, bands, _, channels, taps, _ = TC.reference("B 3, L 255, 4096 taps, marks across a tile's and two waves' ends, air on one band")
    ref = T.ir(d, bands, TC.tail(250, 80, gain=0.0), channels, taps, RATE)
    assert ref.D == 127 and ref.h[:, : ref.K1].any()
    assert not ref.acc[:, :, ref.K1 :].any() and not ref.h[:, ref.K1 + ref.D :].any()


def test_taps_below_k0_minus_d_are_the_bands_call_bitwise():
    d, bands, t, channels, taps, ref = TC.reference("B 3, L 255, 6001 taps, fade 0, min_order 3")
    want = BD.ir(d, bands, channels, taps, RATE)
    edge = ref.K0 - ref.D
    assert np.array_equal(ref.acc[:, :, : ref.K0], want.acc[:, :, : ref.K0])
    assert edge > 0 and ref.h[:, :edge].any() and ref.h[:, :edge].tobytes() == want.h[:, :edge].tobytes()
    other = T.ir(d, bands, TC.tail(1500, 0, seed=12345), channels, taps, RATE)
    assert other.h[:, :edge].tobytes() == ref.h[:, :edge].tobytes()
    for e in range(channels):  # another seed: other taps from K0 on
        assert np.count_nonzero(other.h[e, ref.K0 :] != ref.h[e, ref.K0 :]) > 0.99 * (taps - ref.K0)


def test_a_dead_band_has_no_diffuse_part():
    d, bands, t, channels, taps, ref = TC.reference("B 3, L 255, 4096 taps, pure diffuse, a dead band")
    assert ref.rho[2] == 0.0 and not ref.d[2].any() and not ref.acc[2].any() and ref.acc[0].any() and ref.acc[1].any()


# ---------------------------------------------------------------------------------------------------------- statistics
def pure_diffuse(seed, reflectance):
    taps = WINDOW * WINDOWS
    d = BC.plain(ear_spacing=0.18)
    ref = T.ir(d, BD.describe([(reflectance,) * 6]), T.describe(seed), 2, taps, RATE)
    level = float(d["room"]["level"][0])
    return ref, ref.h.astype(np.float64) / (level * ref.s0)


@pytest.mark.parametrize("seed", SEEDS)
def test_pure_diffuse_variance_is_two_thirds(seed):
    ref, x = pure_diffuse(seed, 1.0)
    assert ref.rho[0] == 1.0 and ref.mu[0] == 0.0 and (ref.K0, ref.K1) == (0, 0)
    var = (x.reshape(2, WINDOWS, WINDOW) ** 2).mean(axis=2)
    worst = np.abs(var / (2.0 / 3.0) - 1.0).max()
    print(f"seed {seed:#x}: window variance / (2/3) in [{var.min() * 1.5:.4f}, {var.max() * 1.5:.4f}], worst {worst:.4f}")
    assert worst <= 0.15


@pytest.mark.parametrize("seed", SEEDS)
def test_decay_follows_eyring(seed):
    ref, x = pure_diffuse(seed, 0.9)
    want = ref.mu[0] * float(BC.plain()["room"]["speed_of_sound"][0])  # nepers of energy per second
    assert ref.rho[0] == pytest.approx(0.81, rel=1e-6) and want * WINDOW * WINDOWS / RATE > 20.0  # a fall of many nepers
    t = (np.arange(WINDOWS) + 0.5) * WINDOW / RATE
    for e in range(2):
        log_e = np.log((x[e].reshape(WINDOWS, WINDOW) ** 2).mean(axis=1))
        slope = -np.polyfit(t, log_e, 1)[0]
        print(f"seed {seed:#x} ear {e}: slope {slope:.4f} /s against mu c = {want:.4f} /s, off by {abs(slope / want - 1.0):.4f}")
        assert abs(slope / want - 1.0) <= 0.10


# ------------------------------------------------------------------------------------------------------ layout, exports
def test_struct_layout_matches_the_c_header(gas, tmp_path):
    dt = gas.capi.ROOM_TAIL_DTYPE
    fields = list(dt.names)
    src = tmp_path / "l.c"
    body = " ".join(f'printf("%zu ", offsetof(gas_room_tail, {f}));' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gas_amd.h"\n' f'int main(void) {{ printf("%zu %zu %zu %d ", sizeof(gas_room_tail), sizeof(gas_room_bands), sizeof(gas_room_ir), GAS_ABI_VERSION); {body} return 0; }}\n')
    exe = tmp_path / "l"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == dt.itemsize == 32
    assert got[1:4] == [264, 184, 2]  # the structs it stands next to keep their sizes; the ABI version stays
    assert fields == ["seed", "mix_time_s", "fade_s", "gain", "reserved"]
    assert got[4:] == [dt.fields[f][1] for f in fields] == [0, 4, 8, 12, 16]
    assert dt.fields["reserved"][0].shape == (4,)
    assert T.ROOM_TAIL_DTYPE == dt  # the reference states the layout on its own


def test_library_exports_and_capi_binds(gas):
    lib = gas.load_library()
    for name, n in (("gas_conv_ir_from_room_diffuse", 8), ("gas_conv_ir_from_room_hrtf_diffuse", 11)):
        assert hasattr(lib, name) and name in gas.capi.EXPORTS
        assert len(getattr(lib, name).argtypes) == n
    assert callable(gas.SpatializerContext.conv_ir_from_room_diffuse) and callable(gas.SpatializerContext.conv_ir_from_room_hrtf_diffuse)
    t = gas.capi.default_room_tail(seed=9)
    assert t.dtype == gas.capi.ROOM_TAIL_DTYPE and t.shape == (1,)
    assert (int(t["seed"][0]), float(t["gain"][0])) == (9, 1.0) and not t["reserved"].any()
    assert T.marks(t, 48000, RATE) == (3840, 4800)
    assert lib.gas_abi_version() == 2


@pytest.mark.parametrize("missing", ["ctx", "desc", "bands", "tail"])
def test_a_null_pointer_is_refused_before_the_device(gas, missing):
    """No context can exist without a device, so the context is NULL throughout; a NULL descriptor, bands or tail next
    to it must be refused in that same first check and never be read.  (With a live context: test_gpu_room_tail.py.)"""
    lib = gas.load_library()
    d, b, t = gas.capi.default_room_ir(), gas.capi.default_room_bands(), gas.capi.default_room_tail()
    hrir = np.zeros((4, 2, 8), np.float32)
    hrir[:, :, 0] = 1.0
    out = np.full((2, 8), np.nan, np.float32)
    ir = C.c_uint32(0xDEADBEEF)
    dp = None if missing == "desc" else d.ctypes.data
    bp = None if missing == "bands" else b.ctypes.data
    tp = None if missing == "tail" else t.ctypes.data
    assert lib.gas_conv_ir_from_room_diffuse(None, dp, bp, tp, 2, 8, out.ctypes.data, C.byref(ir)) == -1
    assert lib.gas_conv_ir_from_room_hrtf_diffuse(None, dp, bp, tp, hrir.ctypes.data, 4, 1, 8, 8, out.ctypes.data, C.byref(ir)) == -1
    assert np.isnan(out).all() and ir.value == 0xDEADBEEF
