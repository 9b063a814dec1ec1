"""GAS_FX_DISTORTION / GAS_FX_COMPRESSOR without a GPU: the numpy restatement the GPU tests compare against
(tests/fx_dyn_ref.py) checked against closed forms, and the gas_fx_dyn_settings layout of the Python binding against
what a C compiler makes of include/gas_amd.h."""
import os
import subprocess

import numpy as np
import pytest

import fx_dyn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings(gas, n, **kw):
    s = gas.capi.fx_dyn_settings_defaults(n)
    for name, v in kw.items():
        s[name] = v
    return s


def test_waveshape_at_drive_zero_with_unit_gains_is_the_identity(gas):
    rng = np.random.default_rng(0)
    x = rng.uniform(-1.0, 1.0, (5, 256, 2)).astype(np.float32)
    s = _settings(gas, 5, distortion_mode=ref.WAVESHAPE, distortion_drive=0.0)
    s["distortion_keep_hf_hz"][:, 0] = [1.0, 100.0, 2000.0, 16000.0, 20000.0]
    h = np.zeros((5, 2), np.float32)
    for _ in range(3):  # and with state carried over
        y, lo = ref.distortion(x, s, 0, h)
        np.testing.assert_allclose(y, x, rtol=0, atol=2e-7)  # lo + (x - lo): one rounding of x - lo
        assert np.abs(lo).max() > 0


def test_distortion_modes_bound_and_quantise(gas):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1.0, 1.0, (4, 128, 2)).astype(np.float32)
    s = _settings(gas, 4, distortion_mode=ref.CLIP, distortion_pre_gain_db=30.0, distortion_keep_hf_hz=20000.0)
    s["distortion_drive"][:, 0] = [0.0, 0.3, 0.7, 1.0]
    k = ref.distortion_constants(s, 0, 48000.0)
    a = rng.uniform(-40.0, 40.0, (4, 128, 2)).astype(np.float32)
    clip = ref.shape(ref.CLIP, a, k, np.ones(4, bool))
    assert np.abs(clip).max() == 1.0 and (np.abs(clip) == 1.0).mean() > 0.5  # CLIP saturates at +-1
    s["distortion_mode"] = ref.LOFI
    k = ref.distortion_constants(s, 0, 48000.0)
    lofi = ref.shape(ref.LOFI, a / np.float32(40.0), k, np.ones(4, bool))
    steps = lofi[[0, 3]] * k["lofi_mult"][[0, 3], None, None]  # (powers of two at drive 0 and 1: exact products)
    np.testing.assert_array_equal(steps, np.round(steps))  # multiples of 1 / lofi_mult
    assert k["lofi_mult"][0] == 65536.0 and k["lofi_mult"][3] == 4.0  # 16 bits at drive 0, 2 at drive 1
    y, _ = ref.distortion(x, s, 0, np.zeros((4, 2), np.float32))
    assert np.isfinite(y).all()


def test_compressor_below_threshold_or_at_ratio_one_is_makeup_and_mix(gas):
    rng = np.random.default_rng(2)
    n, F = 6, 512
    x = rng.uniform(-0.5, 0.5, (n, F, 2)).astype(np.float32)
    s = _settings(gas, n, compressor_threshold_db=0.0)  # |x| < 1: never over
    s["compressor_gain_db"][:, 0] = rng.uniform(-20, 20, n)
    s["compressor_mix"][:, 0] = [0.0, 0.25, 0.5, 0.75, 1.0, 0.1]
    mk = np.exp(s["compressor_gain_db"][:, 0].astype(np.float64) * ref.DB2LIN).astype(np.float32)[:, None, None]
    mix = s["compressor_mix"][:, 0][:, None, None]
    want = ((x * mk) * mix + x * (np.float32(1) - mix)).astype(np.float32)
    rundb = np.zeros(n, np.float32)
    y, over, _ = ref.compressor(x, s, 0, rundb)
    assert (over == 0).all() and (rundb == 0).all()
    np.testing.assert_array_equal(y, want)
    s["compressor_threshold_db"] = -40.0  # well over the threshold, but ratio 1 takes nothing off
    s["compressor_ratio"] = 1.0
    y, over, runs = ref.compressor(x, s, 0, rundb)
    assert over.max() > 50 and runs.max() > 0
    np.testing.assert_array_equal(y, want)


def test_compressor_steady_tone_converges_to_over_over_ratio(gas):
    n, F = 4, 512
    amp = np.float32(0.8)
    x = np.empty((n, F, 2), np.float32)
    x[:, :, 0] = amp * np.where(np.arange(F) % 2 == 0, 1, -1)  # a tone of constant peak (a square wave)
    x[:, :, 1] = -x[:, :, 0]
    s = _settings(gas, n, compressor_threshold_db=-24.0, compressor_attack_us=500.0, compressor_release_ms=100.0)
    s["compressor_ratio"][:, 0] = [2.0, 4.0, 10.0, 48.0]
    rundb = np.zeros(n, np.float32)
    for _ in range(20):
        y, over, runs = ref.compressor(x, s, 0, rundb)
    over_db = 2.08136898 * 8.685889638065035 * np.log(0.8 / 10 ** (-24 / 20))
    np.testing.assert_allclose(over[:, -1], over_db, rtol=1e-6)
    np.testing.assert_allclose(runs[:, -1], over_db, rtol=1e-5)  # the detector has settled on the level
    g_db = 8.685889638065035 * np.log(np.abs(y[:, -1, 0]) / amp)
    ratio = s["compressor_ratio"][:, 0]
    np.testing.assert_allclose(over_db + g_db, over_db / ratio, rtol=1e-4)  # the level above threshold, divided by ratio


def test_compressor_attack_then_release_and_silence(gas):
    n, F = 1, 256
    s = _settings(gas, n, compressor_threshold_db=-20.0, compressor_attack_us=2000.0, compressor_release_ms=20.0)
    rundb = np.zeros(n, np.float32)
    loud = np.full((n, F, 2), 0.9, np.float32)
    _, _, up = ref.compressor(loud, s, 0, rundb)
    assert (np.diff(up[0]) > 0).all()  # attack branch: rising towards over
    quiet = np.zeros((n, F, 2), np.float32)  # silence: lin2db = -inf, clamped to 0
    y, over, down = ref.compressor(quiet, s, 0, rundb)
    assert (over == 0).all() and (np.diff(down[0]) < 0).all() and (y == 0).all()  # release branch: falling to 0


def test_undenormalize_flushes_below_two_to_minus_111():
    v = np.array([2.0**-111, 2.0**-112, -(2.0**-111), -(2.0**-120), 1e-30, 0.0, 3.0], np.float32)
    np.testing.assert_array_equal(ref.undenormalize(v), np.array([2.0**-111, 0.0, -(2.0**-111), 0.0, 1e-30, 0.0, 3.0], np.float32))


def test_dyn_settings_layout_matches_the_c_header(gas, tmp_path):
    dt = gas.capi.FX_DYN_SETTINGS_DTYPE
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gas_amd.h"', "int main(void) {", '\tprintf("size %u\\n", (unsigned)sizeof(gas_fx_dyn_settings));']
    for name in dt.names:
        lines.append(f'\tprintf("{name} %u %u\\n", (unsigned)offsetof(gas_fx_dyn_settings, {name}), (unsigned)sizeof(((gas_fx_dyn_settings *)0)->{name}));')
    consts = ["GAS_FX_DISTORTION", "GAS_FX_COMPRESSOR", "GAS_DISTORTION_CLIP", "GAS_DISTORTION_ATAN", "GAS_DISTORTION_LOFI", "GAS_DISTORTION_OVERDRIVE", "GAS_DISTORTION_WAVESHAPE"]
    for cst in consts:
        lines.append(f'\tprintf("{cst} %d\\n", (int){cst});')
    lines += ["\treturn 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["size"]) == dt.itemsize == 192
    for name in dt.names:
        off, size = map(int, out[name].split())
        assert (off, size) == (dt.fields[name][1], dt.fields[name][0].itemsize), name
    K = gas.capi
    want = [K.FX_DISTORTION, K.FX_COMPRESSOR, K.DISTORTION_CLIP, K.DISTORTION_ATAN, K.DISTORTION_LOFI, K.DISTORTION_OVERDRIVE, K.DISTORTION_WAVESHAPE]
    assert [int(out[c]) for c in consts] == want
    assert K.FX_COMPRESSOR <= 15  # fits the 4-bit chain signature
    d = K.fx_dyn_settings_defaults(1)
    assert d["distortion_keep_hf_hz"][0, 0] == 16000 and d["compressor_ratio"][0, 0] == 4 and d["compressor_attack_us"][0, 0] == 20
    assert d["compressor_release_ms"][0, 0] == 250 and d["compressor_mix"][0, 0] == 1 and d["distortion_mode"][0, 0] == K.DISTORTION_CLIP


@pytest.mark.parametrize("kind", ["host", "ctx"])
def test_new_symbols_are_exported(gas, kind):
    lib = gas.load_library()
    assert hasattr(lib, "gas_fx_dyn_settings_publish" if kind == "ctx" else "gas_host_set_effect_settings_dyn")
