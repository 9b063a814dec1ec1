"""CPU checks of the GAS_FX_EQ6 / _EQ10 / _EQ21 restatement (tests/fx_eq_ref.py) against closed forms and an f64 loop,
and of gas_fx_eq_settings' C layout and the new exports.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import fx_eq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (ref.EQ6, ref.EQ10, ref.EQ21)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sr", [44100.0, 48000.0])
def test_coefficient_table_closed_forms(kind, sr):
    """Every band is the unity-peak resonator H_k(z) = c1 (1 - z^-2) / (1 - c3 z^-1 + c2 z^-2): |H| = 1 at the centre,
    sqrt(1/2) at the lower edge frq_l, 0 at DC and Nyquist, and stable."""
    c1, c2, c3, ok = ref.coefficients(kind, sr, as_f64=True)
    assert ok.all()  # no band falls back to zero coefficients at these rates
    _, _, th, th_l = ref.band_geometry(kind, sr)
    np.testing.assert_allclose(c1, (1.0 - c2) / 2.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(c3, (1.0 + c2) * np.cos(th), rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.abs(ref.response(c1, c2, c3, th)), 1.0, rtol=0, atol=1e-6)
    # The lower edge to 1e-6 except where the f64 formula cancels: a, b and c are differences of terms near s whose
    # result is of order th^4, so the lowest bands of EQ21 carry up to 7.4e-6 (22 Hz at 48 kHz) of f64 rounding.
    edge = np.abs(np.abs(ref.response(c1, c2, c3, th_l)) - np.sqrt(0.5))
    assert edge.max() <= 1e-5, edge
    assert edge[ref.band_geometry(kind, sr)[0] >= 100.0].max() <= 1e-6, edge
    assert np.abs(ref.response(c1, c2, c3, 0.0)).max() == 0.0
    assert np.abs(ref.response(c1, c2, c3, np.pi)).max() <= 1e-9  # (e^{-j pi} is -1 only to f64 rounding)
    c1f, c2f, c3f, _ = ref.coefficients(kind, sr)
    radius = np.array([np.abs(np.roots([1.0, -float(b), float(a)])).max() for a, b in zip(c2f, c3f)])
    assert (radius < 1.0).all(), radius
    assert radius.max() > 0.99  # the long recurrences the kernel must not scan


def test_coefficient_table_at_32khz():
    """At 32 kHz no band falls back to zero coefficients either; the bands at or above Nyquist (EQ10's and EQ21's
    16 kHz, EQ21's 22 kHz) lose the unity peak, and the 16 kHz bands sit on the unit circle."""
    for kind, above in ((ref.EQ6, []), (ref.EQ10, [9]), (ref.EQ21, [19, 20])):
        c1, c2, c3, ok = ref.coefficients(kind, 32000.0, as_f64=True)
        assert ok.all(), kind
        f = np.array(ref.FREQS[kind])
        assert list(np.nonzero(f >= 16000.0)[0]) == above
        _, _, th, _ = ref.band_geometry(kind, 32000.0)
        below = f < 16000.0
        np.testing.assert_allclose(np.abs(ref.response(c1, c2, c3, th))[below], 1.0, atol=1e-6)


def test_no_band_falls_back_at_common_rates():
    """The fallback to zero coefficients (a == 0 or a negative discriminant) is taken by no band of any preset at the
    common mix rates from 8 to 48 kHz."""
    for sr in (8000.0, 11025.0, 16000.0, 22050.0, 24000.0, 32000.0, 44100.0, 48000.0):
        for kind in KINDS:
            with np.errstate(invalid="ignore"):
                assert ref.coefficients(kind, sr)[3].all(), (sr, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_dc_decays_to_zero(kind):
    st = ref.EqStage(kind, 0, 1, 48000.0)
    s = np.zeros(1, np.dtype([("band_gain_db", np.float32, (4, 21))]))
    F = 24000
    y = st.block(np.ones((1, F, 2), np.float32), s)
    assert np.abs(y[0, :32]).max() > 0.1
    assert np.abs(y[0, -256:]).max() < 1e-4


# The f32 recurrence of a band whose poles sit near 1 carries a rounding bias of its own: against the f32-rounded
# coefficients' exact response the settled tail of the lowest bands is off by up to 2.3e-4 (EQ10's 31.25 Hz and EQ21's
# 22 Hz, 48 kHz; it does not shrink with a longer run or fit window), while the same recurrence in f64 is within 2e-6 (what is
# left of the transient).  The engine computes in f32 too, so the restatement keeps that bias; the f32 bound is 3e-4,
# the f64 one 1e-5.
@pytest.mark.parametrize("kind,sr,frames", [(ref.EQ6, 48000.0, 12000), (ref.EQ10, 48000.0, 16000), (ref.EQ21, 48000.0, 24000), (ref.EQ6, 44100.0, 12000), (ref.EQ10, 44100.0, 16000)])
def test_sine_at_each_band_centre_settles_to_the_sum_of_responses(kind, sr, frames):
    """All gains 0 dB, one source per band centre: the tail matches amplitude and phase of sum_k H_k(e^{jw})."""
    f = np.array(ref.FREQS[kind])
    B = len(f)
    w = 2.0 * np.pi * f / np.float64(np.float32(sr))
    t = np.arange(frames)
    x = np.sin(w[:, None] * t[None, :]).astype(np.float32)
    x = np.stack([x, x], axis=2)
    st = ref.EqStage(kind, 2, B, sr)
    s = np.zeros(B, np.dtype([("band_gain_db", np.float32, (4, 21))]))
    y = st.block(x, s)
    c1, c2, c3, _ = ref.coefficients(kind, sr)
    y64 = ref.eq_f64(x, c1, c2, c3, np.ones((B, B)))
    tail = np.arange(frames - 2048, frames)
    for k in range(B):
        H = ref.response(c1, c2, c3, w[k]).sum()
        basis = np.stack([np.sin(w[k] * tail), np.cos(w[k] * tail)], axis=1)
        for out, bound in ((y[k, tail, 0], 3e-4), (y[k, tail, 1], 3e-4), (y64[k, tail, 0], 1e-5)):
            (a, b), *_ = np.linalg.lstsq(basis, out.astype(np.float64), rcond=None)
            got = a + 1j * b  # sin(wt) -> Im(H e^{jwt}) = Re(H) sin(wt) + Im(H) cos(wt)
            assert abs(got - H) <= bound, (kind, f[k], got, H, bound)


def test_restatement_matches_an_f64_loop():
    rng = np.random.default_rng(3)
    dt = np.dtype([("band_gain_db", np.float32, (4, 21))])
    errs = []
    for blk in range(100):
        kind = KINDS[blk % 3]
        j = blk % 4
        n, F = 3, 128
        s = np.zeros(n, dt)
        s["band_gain_db"] = rng.uniform(-60, 24, s["band_gain_db"].shape)
        x = rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)
        st = ref.EqStage(kind, j, n, 48000.0)
        y = st.block(x, s)
        B = st.B
        g = ref.db2lin_block(s["band_gain_db"][:, j, :B])
        want = ref.eq_f64(x, st.c1, st.c2, st.c3, g)
        errs.append(np.sqrt(np.mean((y - want) ** 2)) / np.sqrt(np.mean(want**2)))
    assert max(errs) <= 1e-5, max(errs)


def test_settings_layout_matches_the_c_header(gas, tmp_path):
    """gas_fx_eq_settings compiled from the C header with the system C compiler: size and offsets of the numpy dtype."""
    capi = gas.capi
    src = tmp_path / "l.c"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "gas_amd.h"\n'
        "int main(void) { printf(\"%zu %zu %zu %d %d %d %d %d\\n\", sizeof(gas_fx_eq_settings), offsetof(gas_fx_eq_settings, band_gain_db[1][0]),"
        " offsetof(gas_fx_eq_settings, band_gain_db[3][20]), GAS_EQ_MAX_BANDS, GAS_FX_EQ6, GAS_FX_EQ10, GAS_FX_EQ21, GAS_ABI_VERSION); return 0; }\n"
    )
    exe = tmp_path / "l"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    dt = capi.FX_EQ_SETTINGS_DTYPE
    assert int(got[0]) == dt.itemsize == 336
    assert int(got[1]) == 21 * 4 and int(got[2]) == (3 * 21 + 20) * 4
    assert dt.fields["band_gain_db"][1] == 0 and dt.fields["band_gain_db"][0].shape == (4, 21)
    assert [int(v) for v in got[3:]] == [21, capi.FX_EQ6, capi.FX_EQ10, capi.FX_EQ21, 2]
    assert (capi.FX_EQ6, capi.FX_EQ10, capi.FX_EQ21) == (16, 17, 18)
    d = capi.fx_eq_settings_defaults(3)
    assert d.dtype == dt and (d["band_gain_db"] == 0).all()


def test_new_symbols_are_exported(gas):
    lib = gas.load_library()
    for name in ("gas_fx_eq_settings_publish", "gas_ctx_reserve_fx_eq", "gas_host_set_effect_settings_eq"):
        assert hasattr(lib, name), name
    assert "gas_fx_eq_settings_publish" in gas.capi.EXPORTS and "gas_ctx_reserve_fx_eq" in gas.capi.EXPORTS
