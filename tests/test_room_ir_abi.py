"""gas_conv_ir_from_room through the layers that need no GPU: the struct and the entry are declared in
include/gas_amd.h, the struct compiled from the header with the system C compiler has the size and offsets of
capi.ROOM_IR_DTYPE (and of the reference's own copy), the library exports the symbol and capi binds it."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "gas_amd.h")) as f:
        return f.read()


def test_header_declares_the_struct_and_the_call():
    h = header()
    m = re.search(r"^int gas_conv_ir_from_room\(([^;]*)\);", h, re.M)
    assert m, "not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "desc", "channels", "taps", "out_taps", "out_ir"]
    s = re.search(r"typedef struct gas_room_ir \{(.*?)\} gas_room_ir;", h, re.S)
    assert s, "no struct"
    fields = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", s.group(1), flags=re.S))
    assert fields == ["room", "source", "listener", "ear_spacing", "min_order", "max_order"]
    # declared after the types it holds by value, and described with its rule and what it leaves out
    assert h.index("} gas_room;") < s.start() and h.index("} gas_listener;") < s.start()
    comment = h[h.rindex("/* ----", 0, s.start()):s.start()]
    for phrase in ("llrint(share 2^32)", "max(dist, d0)", "min_order = 3", "Out of scope:", "air absorption", "gas_multi"):
        assert phrase in comment, phrase


def test_struct_layout_matches_the_c_header(gas, tmp_path):
    import room_ir_ref

    dt = gas.capi.ROOM_IR_DTYPE
    fields = list(dt.names)
    src = tmp_path / "l.c"
    body = " ".join(f'printf("%zu ", offsetof(gas_room_ir, {f}));' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gas_amd.h"\n' f'int main(void) {{ printf("%zu %zu %zu ", sizeof(gas_room_ir), sizeof(gas_room), sizeof(gas_listener)); {body} return 0; }}\n')
    exe = tmp_path / "l"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == dt.itemsize == 184
    assert got[1:3] == [gas.capi.ROOM_DTYPE.itemsize, gas.capi.LISTENER_DTYPE.itemsize] == [96, 64]
    assert got[3:] == [dt.fields[f][1] for f in fields] == [0, 96, 108, 172, 176, 180]
    assert dt.fields["room"][0] == gas.capi.ROOM_DTYPE and dt.fields["listener"][0] == gas.capi.LISTENER_DTYPE
    assert dt.fields["min_order"][0] == np.uint32 and dt.fields["source"][0].shape == (3,)
    assert room_ir_ref.ROOM_IR_DTYPE == dt  # the reference states the layout on its own


def test_library_exports_and_capi_binds(gas):
    lib = gas.load_library()
    assert hasattr(lib, "gas_conv_ir_from_room") and "gas_conv_ir_from_room" in gas.capi.EXPORTS
    assert len(lib.gas_conv_ir_from_room.argtypes) == 6
    assert callable(gas.SpatializerContext.conv_ir_from_room)
    d = gas.capi.default_room_ir(min_order=3)
    assert d.dtype == gas.capi.ROOM_IR_DTYPE and d.shape == (1,) and d["min_order"][0] == 3
    assert (d["room"]["half_extent"][0] == (4.0, 2.5, 3.0)).all() and (d["listener"]["basis"][0] == np.eye(3)).all()


def test_the_refusals_that_come_before_the_device(gas):
    """A NULL context or descriptor never reaches a device call."""
    lib = gas.load_library()
    d = gas.capi.default_room_ir()
    out = np.zeros((1, 8), np.float32)
    assert lib.gas_conv_ir_from_room(None, d.ctypes.data, 1, 8, out.ctypes.data, None) == -1
