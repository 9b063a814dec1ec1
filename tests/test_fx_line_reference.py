"""GAS_FX_DELAY / GAS_FX_REVERB without a GPU: the numpy restatement the GPU tests compare against
(tests/fx_line_ref.py) checked against closed forms and an independent float64 loop, and the gas_fx_line_settings
layout of the Python binding against what a C compiler makes of include/gas_amd.h."""
import os
import subprocess

import numpy as np
import pytest

import fx_line_ref as ref
from helpers import rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings(gas, n, **kw):
    s = gas.capi.fx_line_settings_defaults(n)
    for name, v in kw.items():
        s[name] = v
    return s


def test_delay_with_taps_and_feedback_off_is_dry(gas):
    rng = np.random.default_rng(0)
    n, F = 5, 256
    s = _settings(gas, n, delay_tap1_active=0, delay_tap2_active=0, delay_feedback_active=0)
    s["delay_dry"][:, 0] = [0.0, 0.25, 0.5, 0.9, 1.0]
    st = ref.DelayStage(0, n)
    for _ in range(4):
        x = rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)
        y = st.block(x, s)
        np.testing.assert_array_equal(y, x * s["delay_dry"][:, 0][:, None, None])


@pytest.mark.parametrize("tap_ms", [0.0, 1.0, 5.0, 250.0, 1500.0])
def test_one_tap_impulse_lands_at_d_with_the_pan_gains(gas, tap_ms):
    n, F = 3, 128
    s = _settings(gas, n, delay_dry=0.0, delay_tap2_active=0, delay_feedback_active=0, delay_tap1_ms=tap_ms, delay_tap1_level_db=-6.0)
    s["delay_tap1_pan"][:, 0] = [-1.0, 0.0, 0.6]
    D = int(tap_ms / 1000.0 * 48000.0)
    blocks = D // F + 2
    x = np.zeros((n, blocks * F, 2), np.float32)
    x[:, 0, :] = 1.0
    st = ref.DelayStage(0, n)
    y = np.concatenate([st.block(x[:, b * F : (b + 1) * F], s) for b in range(blocks)], axis=1)
    l1 = np.float32(np.exp(-6.0 * ref.DB2LIN))
    pan = s["delay_tap1_pan"][:, 0].astype(np.float64)
    want = np.zeros_like(y)
    want[:, D, 0] = (l1 * np.clip(1 - pan, 0, 1)).astype(np.float32)
    want[:, D, 1] = (l1 * np.clip(1 + pan, 0, 1)).astype(np.float32)
    np.testing.assert_array_equal(y, want)


def test_feedback_echo_repeats_every_dfb_frames_decaying(gas):
    n, F = 1, 512
    s = _settings(gas, n, delay_dry=1.0, delay_tap1_active=0, delay_tap2_active=0, delay_feedback_active=1, delay_feedback_ms=1.0, delay_feedback_level_db=-6.0, delay_feedback_lowpass_hz=16000.0)
    Dfb = int(1.0 / 1000.0 * 48000.0)
    x = np.zeros((n, F, 2), np.float32)
    x[:, 0, :] = 1.0
    y = ref.DelayStage(0, n).block(x, s)
    peaks = [np.abs(y[0, k * Dfb : (k + 1) * Dfb, 0]).max() for k in range(1, F // Dfb)]
    assert peaks[0] > 0.1 and all(b < a for a, b in zip(peaks, peaks[1:]))


def test_reverb_with_wet_zero_is_dry_exactly(gas):
    rng = np.random.default_rng(1)
    n, F = 4, 256
    s = ref.draw_settings(rng, n, gas.capi)
    s["reverb_wet"] = 0.0
    st = ref.ReverbStage(0, n)
    for _ in range(3):
        x = rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)
        y = st.block(x, s)
        np.testing.assert_array_equal(y, (x * s["reverb_dry"][:, 0][:, None, None]).astype(np.float32))


def test_reverb_lengths_at_44100_are_freeverbs_tunings():
    g = ref.reverb_geometry(44100.0)
    assert g["xs"] == [0, 23]  # Freeverb's stereo spread
    assert g["comb"][0] == [1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617]
    assert g["allpass"][0] == [225, 341, 441, 556]
    assert g["comb"][1] == [c + 23 for c in g["comb"][0]] and g["allpass"][1] == [a + 23 for a in g["allpass"][0]]
    g48 = ref.reverb_geometry(48000.0)
    assert g48["echo"] == 24001 and min(g48["comb"][0]) >= 512 and round(0.02 * 48000) >= 512


@pytest.mark.parametrize("hipass", [0.0, 0.3])
def test_reverb_impulse_response_matches_a_float64_loop(gas, hipass):
    F, blocks = 512, 6
    s = _settings(gas, 1, reverb_predelay_ms=30.0, reverb_predelay_feedback=0.5, reverb_room_size=0.9, reverb_damping=0.3, reverb_spread=1.0, reverb_hipass=hipass, reverb_dry=0.7, reverb_wet=0.8)
    x = np.zeros((1, F * blocks, 2), np.float32)
    x[0, 0, :] = 1.0
    x[0, 700, :] = -0.5
    st = ref.ReverbStage(0, 1)
    y = np.concatenate([st.block(x[:, b * F : (b + 1) * F], s) for b in range(blocks)], axis=1)
    k = ref.reverb_constants(s, 0, 48000.0, st.geo)
    g = st.geo
    hp = {} if hipass == 0 else {"a1": float(k["a1"][0]), "b1": float(k["b1"][0])}
    want = ref.reverb_impulse_f64(x[0, :, 0], float(k["fbk"][0]), float(k["damp"][0]), int(k["pd"][0]), 0.5, 0.8, float(np.float32(0.7)), g["comb"][0], g["allpass"][0], g["echo"], **hp)
    assert np.abs(want[2000:]).max() > 1e-3  # a tail, not only the dry impulse
    assert rel_rms(y[0, :, 0], want) <= 1e-5


def test_delay_q_edges(gas):
    """Dfb = 0 keeps q at 0 (one frame of lag); a shorter feedback delay leaves q >= Dfb, which wraps on the next frame."""
    n, F = 1, 128
    s = _settings(gas, n, delay_dry=1.0, delay_tap1_active=0, delay_tap2_active=0, delay_feedback_active=1, delay_feedback_ms=0.0, delay_feedback_level_db=0.0, delay_feedback_lowpass_hz=16000.0)
    st = ref.DelayStage(0, n)
    x = np.zeros((n, F, 2), np.float32)
    x[0, 0, 0] = 1.0
    y = st.block(x, s)
    assert (st.q == 0).all() and y[0, 1, 0] != 0 and y[0, 0, 0] == 1.0  # echo one frame later
    s["delay_feedback_ms"] = 10.0
    st2 = ref.DelayStage(0, n)
    st2.block(np.zeros((n, F, 2), np.float32), s)  # q runs up to 128 of 480
    s["delay_feedback_ms"] = 1.0  # Dfb 48 <= q
    st2.block(np.zeros((n, 1, 2), np.float32), s)
    assert st2.q[0] == 0


def test_line_settings_layout_matches_the_c_header(gas, tmp_path):
    dt = gas.capi.FX_LINE_SETTINGS_DTYPE
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gas_amd.h"', "int main(void) {", '\tprintf("size %u\\n", (unsigned)sizeof(gas_fx_line_settings));']
    for name in dt.names:
        lines.append(f'\tprintf("{name} %u %u\\n", (unsigned)offsetof(gas_fx_line_settings, {name}), (unsigned)sizeof(((gas_fx_line_settings *)0)->{name}));')
    consts = ["GAS_FX_DELAY", "GAS_FX_REVERB"]
    for cst in consts:
        lines.append(f'\tprintf("{cst} %d\\n", (int){cst});')
    lines += ["\treturn 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["size"]) == dt.itemsize == 336
    for name in dt.names:
        off, size = map(int, out[name].split())
        assert (off, size) == (dt.fields[name][1], dt.fields[name][0].itemsize), name
    K = gas.capi
    assert [int(out[c]) for c in consts] == [K.FX_DELAY, K.FX_REVERB] == [13, 14]
    d = K.fx_line_settings_defaults(1)
    assert d["delay_tap1_ms"][0, 0] == 250 and d["delay_tap2_level_db"][0, 0] == -12 and d["delay_feedback_active"][0, 0] == 0
    assert d["reverb_predelay_ms"][0, 0] == 150 and d["reverb_wet"][0, 0] == 0.5 and d["reverb_spread"][0, 0] == 1


@pytest.mark.parametrize("name", ["gas_fx_line_settings_publish", "gas_ctx_reserve_fx_lines", "gas_host_set_effect_settings_line"])
def test_new_symbols_are_exported(gas, name):
    assert hasattr(gas.load_library(), name)
