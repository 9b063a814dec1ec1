"""CPU checks of the GAS_FX_FILTER restatement (tests/fx_filter_ref.py) against the oracle's coefficient preparation,
closed forms and an f64 loop, and of gas_fx_filter_settings' C layout, the shared check and the new exports.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fx_filter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RATES = (44100.0, 48000.0, 96000.0)
# the oracle's kind numbers (GAS_FX_*) of the five modes gaso_filter_coeffs has
ORACLE_KIND = {ref.LOWPASS: 4, ref.HIGHPASS: 5, ref.BANDPASS: 6, ref.NOTCH: 7, ref.LOWSHELF: 8}


def _capi():
    from godot_audio_spatializer_amd import capi

    return capi


def _one(ftype, db, cutoff, resonance, gain=1.0, n=1):
    s = _capi().fx_filter_settings_defaults(n)
    s["type"][:, 0], s["db"][:, 0], s["cutoff_hz"][:, 0], s["resonance"][:, 0], s["gain"][:, 0] = ftype, db, cutoff, resonance, gain
    return s


# --------------------------------------------------------------------------------------------------- layout, exports
def test_settings_layout_matches_the_c_header(gas, tmp_path):
    """gas_fx_filter_settings compiled from the C header with the system C compiler: size, offsets, constants."""
    capi = gas.capi
    dt = capi.FX_FILTER_SETTINGS_DTYPE
    fields = list(dt.names)
    consts = "GAS_MAX_EFFECTS, GAS_FX_FILTER, GAS_ABI_VERSION, GAS_FILTER_LOWPASS, GAS_FILTER_HIGHPASS, GAS_FILTER_BANDPASS, GAS_FILTER_NOTCH, GAS_FILTER_LOWSHELF, GAS_FILTER_HIGHSHELF, GAS_FILTER_BANDLIMIT, GAS_FILTER_6DB, GAS_FILTER_12DB, GAS_FILTER_18DB, GAS_FILTER_24DB"
    body = " ".join(f'printf("%zu ", offsetof(gas_fx_filter_settings, {f}));' for f in fields)
    src = tmp_path / "l.c"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "gas_amd.h"\n'
        f'int main(void) {{ printf("%zu " {" ".join(chr(34) + "%d " + chr(34) for _ in range(14))}, sizeof(gas_fx_filter_settings), {consts}); {body} return 0; }}\n'
    )
    exe = tmp_path / "l"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == dt.itemsize == 128 == C.sizeof(capi.FxFilterSettings)
    assert got[1:4] == [4, capi.FX_FILTER, 2] and capi.FX_FILTER == 24
    assert got[4:11] == [capi.FILTER_LOWPASS, capi.FILTER_HIGHPASS, capi.FILTER_BANDPASS, capi.FILTER_NOTCH, capi.FILTER_LOWSHELF, capi.FILTER_HIGHSHELF, capi.FILTER_BANDLIMIT]
    assert got[4:11] == list(ref.TYPES)
    assert got[11:15] == [0, 1, 2, 3] == [capi.FILTER_6DB, capi.FILTER_12DB, capi.FILTER_18DB, capi.FILTER_24DB]
    assert got[15:] == [dt.fields[f][1] for f in fields] == [0, 16, 32, 48, 64, 80]
    assert fields == ["type", "db", "cutoff_hz", "resonance", "gain", "reserved"]
    assert [getattr(capi.FxFilterSettings, f).offset for f in fields] == got[15:]
    assert dt.fields["type"][0].base == np.int32 and dt.fields["db"][0].base == np.int32
    assert all(dt.fields[f][0].base == np.float32 and dt.fields[f][0].shape == (4,) for f in ("cutoff_hz", "resonance", "gain"))


def test_defaults_are_the_engine_resource():
    d = _capi().fx_filter_settings_defaults(3)
    assert d.dtype == _capi().FX_FILTER_SETTINGS_DTYPE and d.shape == (3,)
    assert (d["type"] == ref.LOWPASS).all() and (d["db"] == 0).all() and (d["reserved"] == 0).all()
    assert (d["cutoff_hz"] == f32(2000.0)).all() and (d["resonance"] == f32(0.5)).all() and (d["gain"] == f32(1.0)).all()


def test_new_symbols_are_exported(gas):
    lib = gas.load_library()
    for name in ("gas_fx_filter_settings_publish", "gas_ctx_reserve_fx_filter", "gas_host_set_effect_settings_filter"):
        assert hasattr(lib, name), name
    assert "gas_fx_filter_settings_publish" in gas.capi.EXPORTS and "gas_ctx_reserve_fx_filter" in gas.capi.EXPORTS


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """csrc/gas_fx_filter_check.h (plain C++) built for the CPU: valid(settings) and the defaults it hands out."""
    d = tmp_path_factory.mktemp("flt_check")
    src = d / "c.cpp"
    hdr = os.path.join(ROOT, "godot-audio-spatializer_amd", "csrc", "gas_fx_filter_check.h")
    src.write_text(
        f'#include "{hdr}"\n'
        'extern "C" int valid(const gas_fx_filter_settings *s) { return gas_fx_filter_settings_valid(*s) ? 1 : 0; }\n'
        'extern "C" void defaults(gas_fx_filter_settings *s) { *s = gas_fx_filter_settings_defaults(); }\n'
    )
    so = d / "c.so"
    subprocess.run(["c++", "-std=c++17", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.valid.argtypes = [C.c_void_p]
    lib.defaults.argtypes = [C.c_void_p]
    return lib


def test_the_shared_check_refuses_what_the_header_says(check):
    capi = _capi()

    def valid(s):
        return bool(check.valid(s.ctypes.data))

    d = capi.fx_filter_settings_defaults(1)
    got = capi.fx_filter_settings_defaults(1)
    got["cutoff_hz"] = 0
    check.defaults(got.ctypes.data)
    assert got.tobytes() == d.tobytes()  # the C defaults are the Python ones
    assert valid(d)
    for j in (0, 3):  # a position is checked whether a chain uses it or not
        for field, values in (
            ("type", (-1, 7, 100)),
            ("db", (-1, 4)),
            ("cutoff_hz", (0.5, 20500.5, np.nan, np.inf, -np.inf)),
            ("resonance", (-0.01, 1.01, np.nan, np.inf)),
            ("gain", (-0.01, 4.01, np.nan, np.inf)),
        ):
            for v in values:
                s = d.copy()
                s[field][0, j] = v
                assert not valid(s), (field, v, j)
        for t in ref.TYPES:
            for db in range(4):
                for cutoff, res, gain in ((1.0, 1.0, 0.0), (20500.0, 1e-6, 4.0)):
                    s = d.copy()
                    s["type"][0, j], s["db"][0, j], s["cutoff_hz"][0, j], s["resonance"][0, j], s["gain"][0, j] = t, db, cutoff, res, gain
                    assert valid(s), (t, db, cutoff)
        s = d.copy()
        s["resonance"][0, j] = 0.0
        assert valid(s)  # every other type takes resonance 0 (the engine's Q floor)
        s["type"][0, j] = ref.BANDLIMIT
        assert not valid(s)  # the documented deviation: log(0) in the engine
        s["resonance"][0, j] = -0.0
        assert not valid(s)


# ------------------------------------------------------------------------------------------------------ coefficients
GRID = [(c, r, g) for c in (1.0, 20.0, 90.0, 2000.0, 5000.0, 20500.0) for r in (0.0, 0.05, 0.5, 0.7, 1.0) for g in (0.0, 0.25, 1.0, 4.0)]


def _oracle_filter(ob, kind, sr, c, r, g):
    L = ob.lib()
    L.gaso_filter_coeffs.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(ob.Coeffs)]
    L.gaso_filter_coeffs.restype = None
    out = ob.Coeffs()
    L.gaso_filter_coeffs(kind, sr, c, r, g, C.byref(out))
    return tuple(f32(getattr(out, k)) for k in ("b0", "b1", "b2", "a1", "a2"))


def _oracle_highshelf(ob, sr, c, r, g, stages):
    out = ob.Coeffs()
    ob.lib().gaso_highshelf_coeffs(sr, c, r, g, stages, C.byref(out))
    return tuple(f32(getattr(out, k)) for k in ("b0", "b1", "b2", "a1", "a2"))


def _bits(co):
    return np.asarray(co, f32).tobytes()


@pytest.mark.parametrize("sr", RATES)
def test_one_stage_equals_the_oracles_filter_coeffs(ob, sr):
    for t, kind in ORACLE_KIND.items():
        for c, r, g in GRID:
            args = (float(f32(c)), float(f32(r)), float(f32(g)))
            assert _bits(ref.coefficients(t, sr, c, r, g, 1)) == _bits(_oracle_filter(ob, kind, sr, *args)), (t, c, r, g)


@pytest.mark.parametrize("sr", RATES)
@pytest.mark.parametrize("stages", [1, 2, 3, 4])
def test_highshelf_equals_the_oracles_at_every_slope(ob, sr, stages):
    for c, r, g in GRID:
        args = (float(f32(c)), float(f32(r)), float(f32(g)))
        assert _bits(ref.coefficients(ref.HIGHSHELF, sr, c, r, g, stages)) == _bits(_oracle_highshelf(ob, sr, *args, stages)), (c, r, g)


def test_stage_correction_leaves_unity_gain_low_q_filters_alone():
    """resonance <= 1 and gain 1: Q stays, pow(1, .) = 1, so LOWPASS / HIGHPASS / NOTCH do not depend on the slope."""
    for t in (ref.LOWPASS, ref.HIGHPASS, ref.NOTCH):
        for c, r, _ in GRID:
            one = _bits(ref.coefficients(t, 48000.0, c, r, 1.0, 1))
            for stages in (2, 3, 4):
                assert _bits(ref.coefficients(t, 48000.0, c, r, 1.0, stages)) == one, (t, c, r, stages)


def test_bandpass_reaches_the_q_above_one_branch():
    """BANDPASS doubles Q first, so resonance in (0.5, 1] takes pow(Q, 1 / stages); up to 0.5 it does not."""
    for r in (0.6, 0.75, 1.0):
        one = ref.coefficients(ref.BANDPASS, 48000.0, 1000.0, r, 1.0, 1)
        for stages in (2, 3, 4):
            got = ref.coefficients(ref.BANDPASS, 48000.0, 1000.0, r, 1.0, stages)
            assert _bits(got) != _bits(one)
            # alpha = sin / (2 Q'), Q' = (2 r)^(1 / stages): a2 = -(1 - alpha) / (1 + alpha)
            q = (2.0 * float(f32(r))) ** (1.0 / stages)
            alpha = np.sin(2 * np.pi * 1000.0 / 48000.0) / (2 * q)
            assert abs(float(got[4]) + (1 - alpha) / (1 + alpha)) < 1e-6
    for r in (0.1, 0.5):
        one = ref.coefficients(ref.BANDPASS, 48000.0, 1000.0, r, 1.0, 1)
        assert all(_bits(ref.coefficients(ref.BANDPASS, 48000.0, 1000.0, r, 1.0, s)) == _bits(one) for s in (2, 3, 4))


@pytest.mark.parametrize("sr", RATES)
def test_bandlimit_is_a_unity_peak_bandpass_and_finite_over_the_range(sr):
    tiny = float(np.nextafter(f32(0), f32(1)))
    for cutoff in (1.0, 20.0, 2000.0, 8000.0, 20500.0):
        for res in (tiny, 1e-30, 1e-6, 0.01, 0.5, 1.0):
            co = ref.coefficients(ref.BANDLIMIT, sr, cutoff, res, 1.0, 1)
            assert np.isfinite(np.asarray(co, np.float64)).all(), (cutoff, res, co)
            assert co[1] == 0 and co[0] == -co[2]  # b0 + b1 + b2 = 0: a zero at DC
            if 1.0 - float(co[3]) - float(co[4]) != 0.0:  # (the widest bands round a2 to 1: a pole on the zero)
                assert abs(ref.response(co, 0.0)) == 0.0
            for stages in (2, 3, 4):  # nothing of it depends on the slope
                assert _bits(ref.coefficients(ref.BANDLIMIT, sr, cutoff, res, 1.0, stages)) == _bits(co)
            if res >= 1e-6 and cutoff >= 20.0:  # (narrower bands: f32 coefficients no longer resolve the peak)
                w0 = 2 * np.pi * ((float(f32(cutoff)) + float(f32(res))) / 2.0) / float(f32(sr))
                assert abs(abs(ref.response(co, w0)) - 1.0) < 2e-4, (cutoff, res, abs(ref.response(co, w0)))


# ----------------------------------------------------------------------------------------------------------- cascade
def test_stage_is_the_direct_form_of_its_coefficients():
    """One stage from rest equals y = b0 x + b1 x1 + b2 x2 + a1 y1 + a2 y2 written out."""
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (2, 64, 2)).astype(f32)
    s = _one(ref.LOWSHELF, 0, 700.0, 0.4, 2.5, n=2)
    y = ref.FilterStage(0, 2).block(x, s)
    b0, b1, b2, a1, a2 = ref.coefficients(ref.LOWSHELF, 48000.0, 700.0, 0.4, 2.5, 1)
    want = np.zeros_like(x)
    for t in range(64):
        x1 = x[:, t - 1] if t >= 1 else 0 * x[:, 0]
        x2 = x[:, t - 2] if t >= 2 else 0 * x[:, 0]
        y1 = want[:, t - 1] if t >= 1 else 0 * x[:, 0]
        y2 = want[:, t - 2] if t >= 2 else 0 * x[:, 0]
        want[:, t] = x[:, t] * b0 + x1 * b1 + x2 * b2 + y1 * a1 + y2 * a2
    np.testing.assert_array_equal(y, want)


def test_four_stages_are_four_one_stage_filters_in_a_row():
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (3, 256, 2)).astype(f32)
    y = ref.FilterStage(0, 3).block(x, _one(ref.LOWPASS, 3, 1500.0, 0.8, n=3))
    v = x
    for _ in range(4):
        v = ref.FilterStage(0, 3).block(v, _one(ref.LOWPASS, 0, 1500.0, 0.8, n=3))
    np.testing.assert_array_equal(y, v)


def test_db_switch_leaves_the_upper_stages_history_alone():
    """24 dB, then 6 dB, then 24 dB again: during the 6 dB block stages 1 .. 3 keep exactly what they held."""
    rng = np.random.default_rng(3)
    st = ref.FilterStage(0, 2)
    blocks = [rng.uniform(-1, 1, (2, 128, 2)).astype(f32) for _ in range(3)]
    st.block(blocks[0], _one(ref.HIGHPASS, 3, 300.0, 0.6, n=2))
    held = st.h.copy()
    assert (held[:, 1:] != 0).any()
    y6 = st.block(blocks[1], _one(ref.HIGHPASS, 0, 300.0, 0.6, n=2))
    np.testing.assert_array_equal(st.h[:, 1:], held[:, 1:])
    assert (st.h[:, 0] != held[:, 0]).any()
    alone = ref.FilterStage(0, 2)
    alone.h[:, 0] = held[:, 0]
    np.testing.assert_array_equal(y6, alone.block(blocks[1], _one(ref.HIGHPASS, 0, 300.0, 0.6, n=2)))
    y24 = st.block(blocks[2], _one(ref.HIGHPASS, 3, 300.0, 0.6, n=2))
    fresh = ref.FilterStage(0, 2)
    fresh.h[:] = held
    fresh.h[:, 0] = alone.h[:, 0]
    np.testing.assert_array_equal(y24, fresh.block(blocks[2], _one(ref.HIGHPASS, 3, 300.0, 0.6, n=2)))


def test_one_block_of_512_is_two_of_256():
    rng = np.random.default_rng(4)
    s = ref.draw_settings(rng, 6, _capi())
    x = rng.uniform(-1, 1, (6, 512, 2)).astype(f32)
    whole = ref.FilterStage(0, 6).block(x, s)
    st = ref.FilterStage(0, 6)
    halves = np.concatenate([st.block(x[:, :256], s), st.block(x[:, 256:], s)], axis=1)
    np.testing.assert_array_equal(whole, halves)


def test_mixed_slopes_in_one_batch_equal_each_alone():
    rng = np.random.default_rng(5)
    s = ref.draw_settings(rng, 8, _capi())
    x = rng.uniform(-1, 1, (8, 128, 2)).astype(f32)
    y = ref.FilterStage(0, 8).block(x, s)
    for i in range(8):
        np.testing.assert_array_equal(y[i], ref.FilterStage(0, 1).block(x[i : i + 1], s[i : i + 1])[0])


F64_CASES = [
    (ref.LOWPASS, 2000.0, 0.5),
    (ref.LOWPASS, 500.0, 1.0),
    (ref.LOWPASS, 200.0, 0.1),
    (ref.HIGHPASS, 90.0, 0.3),
    (ref.HIGHPASS, 90.0, 0.05),
    (ref.BANDPASS, 1000.0, 0.7),
    (ref.BANDLIMIT, 2000.0, 0.5),
    (ref.BANDLIMIT, 8000.0, 0.01),
]
F64_BOUND = 1.3e-4


@pytest.mark.parametrize("ftype,cutoff,resonance", F64_CASES)
def test_float32_cascade_stays_near_an_f64_loop(ftype, cutoff, resonance):
    """4096 frames of uniform noise (seed 0) at 48 kHz, 1 .. 4 stages, the same f32 coefficients in both loops: the
    float32 cascade's largest deviation from the all-f64 loop, relative to the f64 loop's peak.

    Measured with this restatement over all eight settings and four slopes: worst 6.4e-5 (HIGHPASS 90 Hz, resonance
    0.3, one stage; next 4.3e-5 the same at two and four stages).  Bound: twice that, 1.3e-4."""
    x = np.random.default_rng(0).uniform(-1, 1, (1, 4096, 2)).astype(f32)
    for stages in (1, 2, 3, 4):
        y = ref.FilterStage(0, 1).block(x, _one(ftype, stages - 1, cutoff, resonance))[0]
        y64 = ref.cascade_f64(x[0], ref.coefficients(ftype, 48000.0, cutoff, resonance, 1.0, stages), stages)
        err = np.abs(y - y64).max() / np.abs(y64).max()
        print(f"type {ftype} cutoff {cutoff} resonance {resonance} stages {stages}: {err:.3e}")
        assert err <= F64_BOUND, (stages, err)
