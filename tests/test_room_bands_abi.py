"""gas_conv_ir_from_room_bands and gas_conv_ir_from_room_hrtf_bands through the layers that need no GPU: the struct and
the two entries are declared in include/gas_amd.h directly below gas_conv_ir_from_room_hrtf with their rule, the struct
compiled from the header with the system C compiler has the size and offsets of capi.ROOM_BANDS_DTYPE (and of the
reference's own copy), the library exports the symbols, capi binds them, and a NULL context, descriptor or bands is
refused before any device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, HRTF = "gas_conv_ir_from_room_bands", "gas_conv_ir_from_room_hrtf_bands"


def header():
    with open(os.path.join(ROOT, "include", "gas_amd.h")) as f:
        return f.read()


def test_header_declares_the_struct_and_the_calls_with_their_rule():
    h = header()
    args = {}
    for name in (PLAIN, HRTF):
        m = re.search(r"^int %s\(([^;]*)\);" % name, h, re.M)
        assert m, name
        args[name] = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert args[PLAIN] == ["ctx", "desc", "bands", "channels", "taps", "out_taps", "out_ir"]
    assert args[HRTF] == ["ctx", "desc", "bands", "hrir", "n_az", "n_el", "hrir_taps", "taps", "out_taps", "out_ir"]
    s = re.search(r"typedef struct gas_room_bands \{(.*?)\} gas_room_bands;", h, re.S)
    assert s, "no struct"
    fields = re.findall(r"(\w+)(?:\[[^\]]*\])*;", re.sub(r"/\*.*?\*/", "", s.group(1), flags=re.S))
    assert fields == ["n_bands", "filter_taps", "crossover_hz", "reflectance", "air_db_per_m", "reserved"]
    assert re.search(r"^#define GAS_ROOM_MAX_BANDS 8$", h, re.M) and re.search(r"^#define GAS_ROOM_BAND_FILTER_MAX_TAPS 4095$", h, re.M)
    # directly below gas_conv_ir_from_room_hrtf: nothing but this block's comment, the defines and the struct in between
    above = re.search(r"^int gas_conv_ir_from_room_hrtf\([^;]*\);\n", h, re.M)
    between = h[above.end() : h.index("int " + PLAIN + "(")]
    assert "\nint " not in between and between.count("typedef") == 1
    comment = between[between.index("/* NEW") : between.index("#define GAS_ROOM_MAX_BANDS")]
    assert comment.rstrip().endswith("*/") and comment.count("/*") == 1
    for phrase in (
        "room.reflectance := bands.reflectance[b]",
        "validated as before but not used",
        "lambda_b = (ln 10 / 20) air_db_per_m[b] c / rate",
        "g_b[k] = exp(-(lambda_b k))",
        "u_b[e][k] = ((double)acc_b[e][k] 2^-32) g_b[k]",
        "g is exactly 1",
        "w[j] = 0.42 - 0.5 cos(2 pi j / (L - 1)) + 0.08 cos(4 pi j / (L - 1))",
        "lp_i = s_i / sum_j s_i[j]",
        "F_(B-1) = delta_D - lp_(B-2)",
        "y[e][t] = sum_b sum_(j<L) F_b[j] u_b[e][t + D - j]",
        "nothing in this step is atomic",
        "h[e][t] = (float)((double)level y[e][t])",
        "bitwise gas_conv_ir_from_room",
        "exactly `level`",
        "Two runs of one call give the same bits",
        "a NULL bands",
        "reserved != 0",
        "neither read nor checked",
        "GAS_ERR_UNSUPPORTED_CHAIN",
        "Out of scope:",
        "minimum-phase band filters",
        "gas_multi",
    ):
        assert phrase in comment, phrase
    assert re.search(r"^#define GAS_ABI_VERSION 2\b", h, re.M)


def test_struct_layout_matches_the_c_header(gas, tmp_path):
    import room_bands_ref

    dt = gas.capi.ROOM_BANDS_DTYPE
    fields = list(dt.names)
    src = tmp_path / "l.c"
    body = " ".join(f'printf("%zu ", offsetof(gas_room_bands, {f}));' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gas_amd.h"\n' f'int main(void) {{ printf("%zu %zu %zu %zu ", sizeof(gas_room_bands), sizeof(gas_room_ir), sizeof(gas_room), sizeof(gas_listener)); {body} return 0; }}\n')
    exe = tmp_path / "l"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == dt.itemsize == 264
    assert got[1:4] == [184, 96, 64]  # the structs it stands next to keep their sizes
    assert got[4:] == [dt.fields[f][1] for f in fields] == [0, 4, 8, 36, 228, 260]
    assert dt.fields["reflectance"][0].shape == (8, 6) and dt.fields["crossover_hz"][0].shape == (7,) and dt.fields["air_db_per_m"][0].shape == (8,)
    assert (gas.capi.ROOM_MAX_BANDS, gas.capi.ROOM_BAND_FILTER_MAX_TAPS) == (8, 4095)
    assert room_bands_ref.ROOM_BANDS_DTYPE == dt  # the reference states the layout on its own


def test_library_exports_and_capi_binds(gas):
    lib = gas.load_library()
    for name, n in ((PLAIN, 7), (HRTF, 10)):
        assert hasattr(lib, name) and name in gas.capi.EXPORTS
        assert len(getattr(lib, name).argtypes) == n
    assert callable(gas.SpatializerContext.conv_ir_from_room_bands) and callable(gas.SpatializerContext.conv_ir_from_room_hrtf_bands)
    b = gas.capi.default_room_bands()
    assert b.dtype == gas.capi.ROOM_BANDS_DTYPE and b.shape == (1,)
    assert (int(b["n_bands"][0]), int(b["filter_taps"][0]), int(b["reserved"][0])) == (3, 255, 0)
    assert b["crossover_hz"][0, :2].tolist() == [500.0, 4000.0] and not b["crossover_hz"][0, 2:].any()
    assert (b["reflectance"][0, :3] > 0).all() and not b["reflectance"][0, 3:].any()
    one = gas.capi.default_room_bands(crossover_hz=(), reflectance=((0.5, 0.6, 0.7, 0.8, 0.9, 1.0),), air_db_per_m=(0.0,))
    assert int(one["n_bands"][0]) == 1 and one["reflectance"][0, 0].tolist() == [np.float32(v) for v in (0.5, 0.6, 0.7, 0.8, 0.9, 1.0)]


@pytest.mark.parametrize("missing", ["ctx", "desc", "bands"])
def test_a_null_pointer_is_refused_before_the_device(gas, missing):
    """No context can exist without a device, so the context is NULL throughout; a NULL descriptor or bands next to it
    must be refused in that same first check and never be read.  (With a live context: tests/test_gpu_room_bands.py.)"""
    lib = gas.load_library()
    d = gas.capi.default_room_ir()
    b = gas.capi.default_room_bands()
    hrir = np.zeros((4, 2, 8), np.float32)
    hrir[:, :, 0] = 1.0
    out = np.full((2, 8), np.nan, np.float32)
    ir = C.c_uint32(0xDEADBEEF)
    dp = None if missing == "desc" else d.ctypes.data
    bp = None if missing == "bands" else b.ctypes.data
    assert getattr(lib, PLAIN)(None, dp, bp, 2, 8, out.ctypes.data, C.byref(ir)) == -1
    assert getattr(lib, HRTF)(None, dp, bp, hrir.ctypes.data, 4, 1, 8, 8, out.ctypes.data, C.byref(ir)) == -1
    assert np.isnan(out).all() and ir.value == 0xDEADBEEF
