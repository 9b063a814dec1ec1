"""CPU checks of the GAS_FX_PANNER / GAS_FX_STEREO_ENHANCE / GAS_FX_LIMITER restatement (tests/fx_stereo_ref.py)
against closed forms, integer arithmetic and an f64 loop, and of gas_fx_stereo_settings' C layout and the new exports.
No GPU."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fx_stereo_ref as ref
from helpers import TOL, rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _capi():
    from godot_audio_spatializer_amd import capi

    return capi


def _settings(n=1):
    return _capi().fx_stereo_settings_defaults(n)


def _noise(rng, n, F):
    return rng.uniform(-1, 1, (n, F, 2)).astype(f32)


# --------------------------------------------------------------------------------------------------- layout, exports
def test_settings_layout_matches_the_c_header(gas, tmp_path):
    """gas_fx_stereo_settings compiled from the C header with the system C compiler: size and offsets of the numpy dtype."""
    capi = gas.capi
    dt = capi.FX_STEREO_SETTINGS_DTYPE
    fields = list(dt.names)
    src = tmp_path / "l.c"
    body = " ".join(f'printf("%zu ", offsetof(gas_fx_stereo_settings, {f}));' for f in fields)
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "gas_amd.h"\n'
        f'int main(void) {{ printf("%zu %d %d %d %d %d ", sizeof(gas_fx_stereo_settings), GAS_MAX_EFFECTS, GAS_FX_PANNER, GAS_FX_STEREO_ENHANCE, GAS_FX_LIMITER, GAS_ABI_VERSION); {body} return 0; }}\n'
    )
    exe = tmp_path / "l"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == dt.itemsize == 128
    assert got[1:6] == [4, capi.FX_PANNER, capi.FX_STEREO_ENHANCE, capi.FX_LIMITER, 2]
    assert (capi.FX_PANNER, capi.FX_STEREO_ENHANCE, capi.FX_LIMITER) == (21, 22, 23)
    assert got[6:] == [dt.fields[f][1] for f in fields]
    assert len(fields) == 8 and all(dt.fields[f][0].shape == (4,) and dt.fields[f][0].base == np.float32 for f in fields)


def test_defaults_are_the_engine_resources():
    d = _capi().fx_stereo_settings_defaults(3)
    assert d.dtype == _capi().FX_STEREO_SETTINGS_DTYPE and d.shape == (3,)
    want = {
        "panner_pan": 0.0,
        "enhance_pan_pullout": 1.0,
        "enhance_time_pullout_ms": 0.0,
        "enhance_surround": 0.0,
        "limiter_ceiling_db": -0.1,
        "limiter_threshold_db": 0.0,
        "limiter_soft_clip_db": 2.0,
        "limiter_soft_clip_ratio": 10.0,
    }
    for name, v in want.items():
        assert (d[name] == f32(v)).all(), name


def test_new_symbols_are_exported(gas):
    lib = gas.load_library()
    for name in ("gas_fx_stereo_settings_publish", "gas_ctx_reserve_fx_stereo", "gas_host_set_effect_settings_stereo"):
        assert hasattr(lib, name), name
    assert "gas_fx_stereo_settings_publish" in gas.capi.EXPORTS and "gas_ctx_reserve_fx_stereo" in gas.capi.EXPORTS


# ------------------------------------------------------------------------------------------------------------ panner
def test_panner_centre_is_the_identity():
    x = _noise(np.random.default_rng(1), 3, 256)
    x[0, :4] = [[0.0, -0.0], [-0.0, 0.0], [-0.0, -0.0], [1.0, -0.0]]
    y = ref.PannerStage(2, 3).block(x, _settings(3))
    assert (y == x).all()  # as values: -0 may come out +0


def test_panner_hard_left_and_right_closed_form():
    x = _noise(np.random.default_rng(2), 2, 128)
    s = _settings(2)
    s["panner_pan"][:, 1] = (1.0, -1.0)
    y = ref.PannerStage(1, 2).block(x, s)
    both = x[..., 0] + x[..., 1]  # one f32 sum
    assert (y[0, :, 0] == 0).all() and (y[0, :, 1] == both[0]).all()  # pan 1: left 0, right R + L
    assert (y[1, :, 1] == 0).all() and (y[1, :, 0] == both[1]).all()  # pan -1: right 0, left L + R
    s["panner_pan"][:, 1] = (0.5, -0.25)
    y = ref.PannerStage(1, 2).block(x, s)
    assert (y[0, :, 0] == x[0, :, 0] * f32(0.5)).all() and (y[0, :, 1] == x[0, :, 1] + x[0, :, 0] * f32(0.5)).all()
    assert (y[1, :, 1] == x[1, :, 1] * f32(0.75)).all() and (y[1, :, 0] == x[1, :, 0] + x[1, :, 1] * f32(0.25)).all()


# --------------------------------------------------------------------------------------------------- stereo enhance
@pytest.mark.parametrize("sr,R", [(8000.0, 512), (44100.0, 4096), (48000.0, 4096), (96000.0, 8192)])
def test_ring_size(sr, R):
    assert ref.ring_frames(sr) == R
    assert ref.EnhanceStage(0, 1, sr).ring.shape == (1, R)
    assert R > int(0.05 * sr)  # the longest delay fits


def test_enhance_defaults_return_the_input_to_a_rounding():
    """pullout 1, delay 0, no surround: the right ear passes through the ring, both ears are c + (x - c), three f32
    roundings (c, x - c, the sum), each at most 2^-24 of max(|L|, |R|); exact where L = R (x - c = 0)."""
    x = _noise(np.random.default_rng(3), 4, 512)
    x[1, :, 1] = x[1, :, 0]
    st = ref.EnhanceStage(0, 4)
    for _ in range(3):
        y = st.block(x, _settings(4))
        m = np.abs(x).max(axis=-1, keepdims=True).astype(np.float64)
        assert (np.abs(y.astype(np.float64) - x) <= 4 * 2.0**-24 * m).all()
        assert (y[1] == x[1]).all()


def test_enhance_zero_pullout_is_mono():
    x = _noise(np.random.default_rng(4), 3, 256)
    s = _settings(3)
    s["enhance_pan_pullout"][:, 3] = 0.0
    y = ref.EnhanceStage(3, 3).block(x, s)
    c = (x[..., 0] + x[..., 1]) * f32(0.5)
    assert (y[..., 0] == c).all() and (y[..., 1] == c).all()


@pytest.mark.parametrize("sr", [44100.0, 48000.0, 96000.0])
@pytest.mark.parametrize("ms", [0.0, 0.02, 1.0, 50.0])
def test_enhance_right_impulse_arrives_delay_frames_later(sr, ms):
    """The delay against integer arithmetic: floor(ms sr / 1000) with ms the f32 the POD holds."""
    want = int(Fraction(float(f32(ms))) * Fraction(sr) / 1000)
    assert want == {0.0: 0, 0.02: int(sr == 96000.0), 1.0: int(sr // 1000), 50.0: int(sr // 20)}[ms]
    assert ref.delay_frames(f32(ms), sr) == want
    F, k0 = 512, 37
    blocks = (k0 + want) // F + 2
    x = np.zeros((1, F * blocks, 2), f32)
    x[0, k0, 1] = 1.0
    s = _settings(1)
    s["enhance_time_pullout_ms"][:, 0] = ms
    st = ref.EnhanceStage(0, 1, sr)
    y = np.concatenate([st.block(x[:, b * F : (b + 1) * F], s) for b in range(blocks)], axis=1)
    expect = np.zeros_like(x)
    expect[0, k0 + want, 1] = 1.0
    assert (y == expect).all()
    assert st.pos[0] == F * blocks


def test_enhance_surround_adds_to_the_left_and_takes_from_the_right():
    rng = np.random.default_rng(5)
    n, F = 3, 512
    s = _settings(n)
    s["enhance_surround"][:, 0] = (0.25, 1.0, 0.6)
    s["enhance_time_pullout_ms"][:, 0] = (0.0, 2.0, 7.5)
    s["enhance_pan_pullout"][:, 0] = (1.0, 2.5, 0.5)
    st = ref.EnhanceStage(0, n)
    xs = [_noise(rng, n, F) for _ in range(3)]
    y = np.concatenate([st.block(x, s) for x in xs], axis=1)
    x = np.concatenate(xs, axis=1)
    pull, sur = s["enhance_pan_pullout"][:, 0][:, None], s["enhance_surround"][:, 0][:, None]
    c = (x[..., 0] + x[..., 1]) * f32(0.5)
    l, r = c + (x[..., 0] - c) * pull, c + (x[..., 1] - c) * pull
    mid = (l + r) * f32(0.5)
    for k in range(n):
        d = int(ref.delay_frames(s["enhance_time_pullout_ms"][k, 0], 48000.0))
        o = np.concatenate([np.zeros(d, f32), mid[k, : 3 * F - d]]) * sur[k]
        assert (y[k, :, 0] == l[k] + o).all() and (y[k, :, 1] == r[k] - o).all()
        # the left-plus-right sum is unchanged to rounding (two more f32 roundings of magnitude <= |l| + |o|, |r| + |o|)
        bound = 2.0**-23 * (np.abs(l[k]) + np.abs(r[k]) + 2 * np.abs(o)).astype(np.float64)
        assert (np.abs((y[k, :, 0].astype(np.float64) + y[k, :, 1]) - (l[k].astype(np.float64) + r[k])) <= bound).all()


def test_enhance_one_512_block_equals_two_256_blocks():
    rng = np.random.default_rng(6)
    n = 8
    s = ref.draw_settings(rng, n, _capi())
    a, b = ref.EnhanceStage(2, n), ref.EnhanceStage(2, n)
    for _ in range(12):  # 6144 frames: the 4096-frame ring wraps
        x = _noise(rng, n, 512)
        ya = a.block(x, s)
        yb = np.concatenate([b.block(x[:, :256], s), b.block(x[:, 256:], s)], axis=1)
        np.testing.assert_array_equal(ya, yb)
    np.testing.assert_array_equal(a.ring, b.ring)


def test_enhance_surround_switch_reads_the_other_modes_history():
    """Block 1 without surround writes r into the ring; block 2 with surround reads those values as its delayed mid
    for the first `delay` frames (and the other way round in block 3)."""
    rng = np.random.default_rng(7)
    F, d = 256, 96
    s = _settings(1)
    s["enhance_time_pullout_ms"][:, 0] = 2.0
    assert ref.delay_frames(f32(2.0), 48000.0) == d
    st = ref.EnhanceStage(0, 1)
    x1, x2, x3 = (_noise(rng, 1, F) for _ in range(3))
    y1 = st.block(x1, s)
    c1 = (x1[0, :, 0] + x1[0, :, 1]) * f32(0.5)
    r1 = c1 + (x1[0, :, 1] - c1)
    assert (y1[0, d:, 1] == r1[: F - d]).all() and (y1[0, :d, 1] == 0).all()
    s2 = s.copy()
    s2["enhance_surround"][:, 0] = 0.5
    y2 = st.block(x2, s2)
    c2 = (x2[0, :, 0] + x2[0, :, 1]) * f32(0.5)
    l2, r2 = c2 + (x2[0, :, 0] - c2), c2 + (x2[0, :, 1] - c2)
    o = r1[F - d :] * f32(0.5)  # block 1's right ears, not mids
    assert (y2[0, :d, 0] == l2[:d] + o).all() and (y2[0, :d, 1] == r2[:d] - o).all()
    y3 = st.block(x3, s)
    mid2 = (l2 + r2) * f32(0.5)
    assert (y3[0, :d, 1] == mid2[F - d :]).all()  # block 2's mids come out as right ears


# ----------------------------------------------------------------------------------------------------------- limiter
def _limiter_case(seed, n=40, F=512, scale=2.0):
    rng = np.random.default_rng(seed)
    s = ref.draw_settings(rng, n, _capi())
    x = (rng.standard_normal((n, F, 2)) * scale).astype(f32)
    return s, x


@pytest.mark.parametrize("j", [0, 3])
def test_limiter_never_exceeds_the_ceiling_and_keeps_the_sign(j):
    s, x = _limiter_case(10 + j)
    corners = [(-0.1, 0.0, 2.0), (-20.0, -30.0, 6.0), (-0.1, 0.0, 0.0), (-20.0, 0.0, 0.0)]
    for k, (c, t, sc) in enumerate(corners):
        s["limiter_ceiling_db"][k, j], s["limiter_threshold_db"][k, j], s["limiter_soft_clip_db"][k, j] = c, t, sc
    y = ref.LimiterStage(j, len(x)).block(x, s)
    ceiling = ref.limiter_constants(s, j)[0][:, None, None]
    assert np.isfinite(y).all()
    assert (np.abs(y) <= ceiling).all()
    nz = x != 0
    assert (np.sign(y[nz]) == np.sign(x[nz])).all()


def test_limiter_below_soft_clip_and_ceiling_is_the_makeup_product_bitwise():
    s, x = _limiter_case(12, scale=0.3)
    y = ref.LimiterStage(1, len(x)).block(x, s)
    ceiling, makeup, scv, _, _ = (k[:, None, None] for k in ref.limiter_constants(s, 1))
    p = x * makeup
    low = (np.abs(p) < scv) & (np.abs(p) < ceiling)
    assert low.mean() > 0.2
    assert (y[low] == p[low]).all()


def test_limiter_matches_an_f64_loop():
    s, x = _limiter_case(13, n=24, F=128)
    y = ref.LimiterStage(2, len(x)).block(x, s)
    want = ref.limiter_f64(x, s, 2)
    for k in range(len(x)):
        assert rel_rms(y[k], want[k]) <= TOL, (k, rel_rms(y[k], want[k]))


def test_draw_settings_pass_the_ranges_and_hit_the_edges():
    s = ref.draw_settings(np.random.default_rng(14), 400, _capi())
    for name, e in ref._EDGES.items():
        assert (s[name] >= f32(e[0])).all() and (s[name] <= f32(e[1])).all(), name
        assert (s[name] == f32(e[0])).any() and (s[name] == f32(e[1])).any(), name
    assert 0.3 < (s["enhance_surround"] > 0).mean() < 0.7
