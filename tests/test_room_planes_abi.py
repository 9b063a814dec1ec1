"""gas_conv_ir_from_planes through the layers that need no GPU: the structs and the entry are declared in
include/gas_amd.h, the structs compiled from the header with the system C compiler have the sizes and offsets of
capi.ROOM_PLANE_DTYPE and capi.ROOM_PLANES_DTYPE (and of the reference's own copies), the library exports the symbol and
capi binds it."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "gas_amd.h")) as f:
        return f.read()


def fields_of(h, name):
    s = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S)
    assert s, name
    return s, re.findall(r"(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", s.group(1), flags=re.S))


def test_header_declares_the_structs_and_the_call():
    h = header()
    m = re.search(r"^int gas_conv_ir_from_planes\(([^;]*)\);", h, re.M)
    assert m, "not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "desc", "channels", "taps", "out_taps", "out_ir"]
    assert re.search(r"^#define GAS_ROOM_MAX_PLANES 16$", h, re.M) and re.search(r"^#define GAS_ROOM_PLANES_MAX_ORDER 8$", h, re.M)
    assert re.search(r"^#define GAS_ABI_VERSION 2\b", h, re.M)
    plane, plane_fields = fields_of(h, "gas_room_plane")
    planes, planes_fields = fields_of(h, "gas_room_planes")
    assert plane_fields == ["normal", "offset", "reflectance"]
    assert planes_fields == ["planes", "n_planes", "speed_of_sound", "level", "source", "listener", "ear_spacing", "min_order", "max_order"]
    # after the box call and the listener it holds by value, before the binaural box call; described with its rule
    box = re.search(r"^int gas_conv_ir_from_room\(", h, re.M)
    assert box.start() < plane.start() < planes.start() < m.start() < h.index("int gas_conv_ir_from_room_hrtf(")
    assert h.index("} gas_listener;") < planes.start()
    comment = h[h.rindex("/* NEW: gas_conv_ir_from_planes", 0, plane.start()) : plane.start()]
    for phrase in ("(n_x x_x + n_y x_y) + n_z x_z", "q_i != q_{i+1}", "P (P - 1)^(K - 1)", "void unless t > 0", "u = a / (a - b)", "count twice", "max(dist, d0)", "llrint(share 2^32)", "[0.999, 1.001]", "2^28", "Out of scope:", "non-convex", "gas_multi"):
        assert phrase in comment, phrase
    # the box calls' "rooms that are not boxes" now name this call
    box_comment = h[h.rindex("/* ----", 0, box.start()) : box.start()]
    assert "rooms that are not boxes" in box_comment and "gas_conv_ir_from_planes" in box_comment


def test_struct_layouts_match_the_c_header(gas, tmp_path):
    import room_planes_ref

    plane, planes = gas.capi.ROOM_PLANE_DTYPE, gas.capi.ROOM_PLANES_DTYPE
    src = tmp_path / "l.c"
    body = " ".join(f'printf("%zu ", offsetof(gas_room_plane, {f}));' for f in plane.names) + " ".join(f'printf("%zu ", offsetof(gas_room_planes, {f}));' for f in planes.names)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gas_amd.h"\n' f'int main(void) {{ printf("%zu %zu %zu %d %d ", sizeof(gas_room_plane), sizeof(gas_room_planes), sizeof(gas_listener), GAS_ROOM_MAX_PLANES, GAS_ROOM_PLANES_MAX_ORDER); {body} return 0; }}\n')
    exe = tmp_path / "l"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:5] == [plane.itemsize, planes.itemsize, gas.capi.LISTENER_DTYPE.itemsize, gas.capi.ROOM_MAX_PLANES, gas.capi.ROOM_PLANES_MAX_ORDER] == [20, 420, 64, 16, 8]
    assert got[5:8] == [plane.fields[f][1] for f in plane.names] == [0, 12, 16]
    assert got[8:] == [planes.fields[f][1] for f in planes.names] == [0, 320, 324, 328, 332, 344, 408, 412, 416]
    assert planes.fields["planes"][0] == np.dtype((plane, (16,))) and planes.fields["listener"][0] == gas.capi.LISTENER_DTYPE
    assert planes.fields["n_planes"][0] == np.uint32 and planes.fields["max_order"][0] == np.uint32 and plane.fields["normal"][0].shape == (3,)
    # the reference states the layouts on its own
    assert room_planes_ref.ROOM_PLANE_DTYPE == plane and room_planes_ref.ROOM_PLANES_DTYPE == planes
    assert (room_planes_ref.MAX_PLANES, room_planes_ref.MAX_ORDER) == (16, 8)


def test_library_exports_and_capi_binds(gas):
    lib = gas.load_library()
    assert hasattr(lib, "gas_conv_ir_from_planes") and "gas_conv_ir_from_planes" in gas.capi.EXPORTS
    assert len(lib.gas_conv_ir_from_planes.argtypes) == 6
    assert callable(gas.SpatializerContext.conv_ir_from_planes)
    d = gas.capi.default_room_planes(min_order=1)
    assert d.dtype == gas.capi.ROOM_PLANES_DTYPE and d.shape == (1,) and (d["n_planes"][0], d["min_order"][0], d["max_order"][0]) == (7, 1, 3)
    n = d["planes"]["normal"][0, :7].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6) and (d["listener"]["basis"][0] == np.eye(3)).all()
    # source and listener are strictly inside every half-space of the default
    for x in (d["source"][0], d["listener"]["origin"][0]):
        assert (n @ x.astype(np.float64) - d["planes"]["offset"][0, :7] > 0.1).all()


def test_planes_from_box(gas):
    """Six planes in gas_room's wall order whose inside is the box: the centre is h_a inside the two walls of axis a, and
    a rotated box keeps that."""
    import er_rooms_ref as E

    K = gas.capi
    room = K.default_rooms(half_extent=(2.5, 2.0, 1.5), origin=(3.0, -7.0, 11.0), reflectance=(0.9, 0.85, 0.8, 0.75, 0.7, 0.95))
    p = K.planes_from_box(room)
    assert p.dtype == K.ROOM_PLANE_DTYPE and p.shape == (6,)
    assert (p["normal"] == [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]).all()
    assert (p["offset"] == [0.5, -5.5, -9.0, 5.0, 9.5, -12.5]).all()
    assert (p["reflectance"] == room["reflectance"][0]).all()
    B = E.random_basis(np.random.default_rng(3))
    room["basis"] = B
    q = K.planes_from_box(room)
    centre = q["normal"].astype(np.float64) @ np.array([3.0, -7.0, 11.0]) - q["offset"]
    assert np.allclose(centre, [2.5, 2.5, 2.0, 2.0, 1.5, 1.5], atol=1e-5)
    assert np.allclose(q["normal"][0::2], B.T, atol=1e-7) and np.allclose(q["normal"][1::2], -B.T, atol=1e-7)
    d = K.default_room_planes(planes=p, source=(4.0, -6.5, 11.25), listener_origin=(2.0, -6.75, 10.5), max_order=4)
    assert d["n_planes"][0] == 6 and (d["planes"][0, :6] == p).all() and not d["planes"]["normal"][0, 6:].any()


def test_the_refusals_that_come_before_the_device(gas):
    """A NULL context or descriptor never reaches a device call."""
    lib = gas.load_library()
    d = gas.capi.default_room_planes()
    out = np.zeros((1, 8), np.float32)
    assert lib.gas_conv_ir_from_planes(None, d.ctypes.data, 1, 8, out.ctypes.data, None) == -1
    assert not out.any()
