"""gas_conv_ir_from_room_hrtf through the layers that need no GPU: the entry is declared in include/gas_amd.h below
gas_conv_ir_from_room with its rule and what it leaves out, the library exports the symbol, capi binds it, and a NULL
context is refused before any device call."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gas_conv_ir_from_room_hrtf"


def header():
    with open(os.path.join(ROOT, "include", "gas_amd.h")) as f:
        return f.read()


def test_header_declares_the_call_with_its_rule():
    h = header()
    m = re.search(r"^int gas_conv_ir_from_room_hrtf\(([^;]*)\);", h, re.M)
    assert m, "not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "desc", "hrir", "n_az", "n_el", "hrir_taps", "taps", "out_taps", "out_ir"]
    # below the one-channel call, whose own comment block and struct stay where they are
    mono = re.search(r"^int gas_conv_ir_from_room\(", h, re.M)
    assert mono and mono.start() < m.start()
    assert h.index("} gas_room_ir;") < m.start()
    comment = h[h.rindex("/* NEW", 0, m.start()) : m.start()]
    assert comment.rstrip().endswith("*/") and comment.count("/*") == 1
    for phrase in (
        "ear 0 is left, ear 1 is right",
        "ear_spacing is neither",
        "channels = 1",
        "max(dist, d0)",
        "az = atan2(p_x, -p_z)",
        "llround(az / 2pi n_az)",
        "dir = ei n_az + ai",
        "hrtf_dir",
        "g_j = a0 H[dir][e][j] + a1 H[dir][e][j - 1]",
        "llrint(g_j 2^32)",
        "above 4 in magnitude",
        "bitwise the one-channel",
        "Two runs of one call give the same bits",
        "GAS_ERR_UNSUPPORTED_CHAIN",
        "min_order = 3",
        "Out of scope:",
        "nearest cell only",
        "four-channel results",
        "GAS_FX_EARLY_REFLECTIONS",
        "air absorption",
        "shell-per-workgroup",
        "gas_multi",
    ):
        assert phrase in comment, phrase


def test_library_exports_and_capi_binds(gas):
    lib = gas.load_library()
    assert hasattr(lib, NAME) and NAME in gas.capi.EXPORTS
    assert len(getattr(lib, NAME).argtypes) == 9
    assert callable(gas.SpatializerContext.conv_ir_from_room_hrtf)


def test_a_null_context_is_refused_before_the_device(gas):
    lib = gas.load_library()
    d = gas.capi.default_room_ir()
    hrir = np.zeros((4, 2, 8), np.float32)
    hrir[:, :, 0] = 1.0
    out = np.full((2, 8), np.nan, np.float32)
    assert getattr(lib, NAME)(None, d.ctypes.data, hrir.ctypes.data, 4, 1, 8, 8, out.ctypes.data, None) == -1
    assert np.isnan(out).all()
