"""GAS_FLAG_HRTF_BLEND_FADE without a GPU: the composed fade reference against the only fade arithmetic the project
already has (the oracle run with crossfade=True), and the ABI surface."""
import os
import re

import numpy as np
import pytest

import hrtf_blend_fade_ref as fref
import hrtf_blend_ref as ref
from helpers import rel_rms


@pytest.mark.parametrize("F", [128, 384])
def test_one_row_blends_reproduce_the_crossfade_oracle(gas, ob, F):
    """3 sources, 5 blocks, directions change on blocks 1 and 3 (source 2 only on block 3).  One-row blends, so the
    composed reference must be what the oracle's cross-fade renders.  Bound 1e-6 relative RMS, that of
    test_hrtf_blend_reference.py: the two differ by the oracle's f32 rows under the f64 lerp and, at F = 384 where 1/F
    is not a power of two, by one ulp of t (the oracle divides i / n, the product multiplies i * (1 / F))."""
    from godot_audio_spatializer_amd import synth

    rng = np.random.default_rng(41)
    n, dirs = 3, 32
    chain = (ob.FX_HRTF,)
    hrir = synth.synthetic_hrir(rng, dirs=dirs)
    composed = fref.BlendFadeReference(ob, n, F, chain, hrir)
    xf = ob.BatchOracle(ob.KIND_EFFECT, n, F, chain=chain, hrir=hrir, crossfade=True)
    d = rng.integers(0, dirs, n)
    worst = 0.0
    for b in range(5):
        if b in (1, 3):
            move = np.array([True, True, b == 3])
            d = np.where(move, (d + 1 + rng.integers(0, dirs - 1, n)) % dirs, d)
        p = synth.draw_params(rng, n, dirs=dirs, frames=F)
        p["hrtf_dir"] = d
        src = synth.draw_sources(rng, n, F)
        # even blocks name the direction by an explicit one-row blend, odd ones by the all-zero row (hrtf_dir)
        blends = ref.one_row(d) if b % 2 == 0 else np.zeros(n, gas.capi.HRTF_BLEND_DTYPE)
        rows, peaks, mix = composed.block(p, blends, src)
        _, xpeaks, x64 = xf.block(p.astype(ob.PARAMS_DTYPE), src, want64=True)
        err = rel_rms(mix, x64[0])
        print(f"F {F} block {b}: composed vs cross-fade oracle {err:.3e}")
        worst = max(worst, err)
        np.testing.assert_allclose(peaks, xpeaks, rtol=2e-5, atol=1e-7)
    assert worst <= 1e-6


def test_effective_row():
    K_DTYPE = np.dtype([("dir", np.uint32, (4,)), ("weight", np.float32, (4,))])
    b = np.zeros(1, K_DTYPE)
    d, w = fref.effective_row(b[0], 7, 32)
    assert list(d) == [7, 0, 0, 0] and list(w) == [1, 0, 0, 0]
    d, w = fref.effective_row(b[0], 99, 32)  # clamped as hrtf_dir is
    assert list(d) == [0, 0, 0, 0] and list(w) == [1, 0, 0, 0]
    b["dir"][0], b["weight"][0] = (5, 6, 40, 8), (0, 0.25, 0.5, 0.25)
    d, w = fref.effective_row(b[0], 7, 32)
    assert list(d) == [6, 0, 8, 0] and list(w) == [0.25, 0.5, 0.25, 0]
    assert fref.same_row((d, w), fref.effective_row(b[0], 9, 32))  # hrtf_dir does not enter a row with weights
    b["weight"][0, 1] = np.nextafter(np.float32(0.25), np.float32(1))
    assert not fref.same_row((d, w), fref.effective_row(b[0], 7, 32))  # one bit of one weight
    t, one_t = fref.ramp(384)
    assert t.dtype == np.float32 and t[0] == 0 and t[383] == np.float32(383) * (np.float32(1) / np.float32(384))


def test_flag_value(gas):
    K = gas.capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gas_amd.h")).read()
    m = re.search(r"^#define GAS_FLAG_HRTF_BLEND_FADE (\d+)u$", header, re.M)
    assert m and int(m.group(1)) == 256
    assert K.FLAG_HRTF_BLEND_FADE == 256
    assert K.FLAG_HRTF_BLEND_FADE & (K.FLAG_HRTF_INTERPOLATE | K.FLAG_BATCHED_LAUNCH | K.FLAG_XCD_ORDER) == 0
