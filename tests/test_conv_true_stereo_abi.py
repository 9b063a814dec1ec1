"""Four-channel ("true stereo") impulse responses and gas_conv_ir_get_info through the layers that need no GPU: the
entry is declared in include/gas_amd.h with its argument names, exported by the library and bound by capi; the
convolver comment carries the true-stereo rule next to the two-channel one and no longer calls it out of scope."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "gas_amd.h")) as f:
        return f.read()


def test_header_declares_get_info():
    m = re.search(r"^int gas_conv_ir_get_info\(([^;]*)\);", header(), re.M)
    assert m, "not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "ir", "out_channels", "out_taps"]


def test_header_states_both_rules():
    h = header()
    end = h.index("#define GAS_MAX_CONVOLVERS")
    comment = h[h.rindex("/*", 0, end):end]
    assert "dry * x_e[t] + wet * sum_{j=0}^{T-1} h_e[j] * x_e[t - j]" in comment  # the two-channel line stays
    assert "y_e[t] = dry * x_e[t] + wet * sum_{j=0}^{T-1} ( h_{0e}[j] * x_0[t - j] + h_{1e}[j] * x_1[t - j] )" in comment
    assert "c = 2 * i + e" in comment and "LL, LR, RL, RR" in comment
    scope = comment[comment.index("Out of scope:"):]
    assert "four-channel" not in scope and "IRs" not in scope
    for kept in ("non-uniform partitioning", "gas_multi", "host layer", "godot_module/"):
        assert kept in scope
    m = re.search(r"^int gas_conv_ir_load\(([^;]*)\);", h, re.M)
    assert "1, 2 or 4" in m.group(1)
    assert "four times a mono IR's" in re.sub(r"\s*\n \*\s*", " ", h)


def test_library_exports_and_capi_binds(gas):
    lib = gas.load_library()
    assert hasattr(lib, "gas_conv_ir_get_info") and "gas_conv_ir_get_info" in gas.capi.EXPORTS
    assert len(lib.gas_conv_ir_get_info.argtypes) == 4
    assert callable(gas.SpatializerContext.conv_ir_get_info)
