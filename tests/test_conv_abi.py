"""The bus convolvers through the layers that need no GPU: declared in include/gas_amd.h with their argument names,
exported by the library, bound by capi."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "gas_ctx_reserve_conv": (["ctx", "convolvers", "max_ir_taps"], "reserve_conv"),
    "gas_conv_ir_load": (["ctx", "ir", "channels", "taps", "out_ir"], "conv_ir_load"),
    "gas_conv_ir_free": (["ctx", "ir"], "conv_ir_free"),
    "gas_conv_create": (["ctx", "ir", "out_conv"], "conv_create"),
    "gas_conv_destroy": (["ctx", "conv"], "conv_destroy"),
    "gas_conv_reset": (["ctx", "conv"], "conv_reset"),
    "gas_conv_set_ir": (["ctx", "conv", "ir"], "conv_set_ir"),
    "gas_conv_set_levels": (["ctx", "conv", "dry", "wet"], "conv_set_levels"),
    "gas_conv_process": (["ctx", "convs", "n", "in", "out", "frames", "mem"], "conv_process"),
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


def test_header_states_the_pool_limit_and_the_rule():
    h = header()
    assert re.search(r"^#define GAS_MAX_CONVOLVERS 24\b", h, re.M)
    end = h.index("#define GAS_MAX_CONVOLVERS")
    comment = h[h.rindex("/*", 0, end):end]
    assert "NEW" in comment and "dry * x_e[t] + wet * sum_{j=0}^{T-1} h_e[j] * x_e[t - j]" in comment


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_and_capi_binds(gas, name):
    lib = gas.load_library()
    assert hasattr(lib, name) and name in gas.capi.EXPORTS
    assert len(getattr(lib, name).argtypes) == len(ENTRIES[name][0])
    assert callable(getattr(gas.SpatializerContext, ENTRIES[name][1]))
