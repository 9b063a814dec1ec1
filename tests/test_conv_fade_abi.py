"""gas_conv_fade_to / gas_conv_fade_remaining through the layers that need no GPU: declared in include/gas_amd.h with
their argument names, exported by the library, bound by capi; the cap is defined and the header carries the formula."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "gas_conv_fade_to": (["ctx", "conv", "ir", "dry", "wet", "fade_blocks"], "conv_fade_to"),
    "gas_conv_fade_remaining": (["ctx", "conv", "out_blocks"], "conv_fade_remaining"),
}


def header():
    with open(os.path.join(ROOT, "include", "gas_amd.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_declares_the_entry(name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header(), re.M)
    assert m, "not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ENTRIES[name][0]


def test_header_states_the_cap_and_the_fade_formula():
    h = header()
    assert re.search(r"^#define GAS_CONV_MAX_FADE_BLOCKS 4096\b", h, re.M)
    end = h.index("#define GAS_CONV_MAX_FADE_BLOCKS")
    comment = h[h.rindex("/*", 0, end):end]
    assert "NEW" in comment
    assert "y[t] = (1 - s) * y^A[t] + s * y^B[t]" in comment
    assert "s = (float)(b * F + i) * (1.0f / (float)(N * F))" in comment
    # the convolvers' own block keeps its rule, and no longer lists fades as out of scope
    end = h.index("#define GAS_MAX_CONVOLVERS")
    block = h[h.rindex("/*", 0, end):end]
    scope = block[block.index("Out of scope:"):]
    assert "fading" not in scope and "level ramps" not in scope
    for kept in ("true stereo", "non-uniform partitioning", "gas_multi", "host layer", "godot_module/"):
        assert kept in scope
    assert re.search(r"^#define GAS_ABI_VERSION", h, re.M)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_and_capi_binds(gas, name):
    lib = gas.load_library()
    assert hasattr(lib, name) and name in gas.capi.EXPORTS
    assert len(getattr(lib, name).argtypes) == len(ENTRIES[name][0])
    assert callable(getattr(gas.SpatializerContext, ENTRIES[name][1]))
