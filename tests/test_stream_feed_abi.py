"""gas_source_feed_rows and gas_host_set_mixed through the layers that need no GPU: declared in the headers, exported by
the library, bound by capi with the header's argument list; GAS_ABI_VERSION and the gas_pcm_format values untouched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gas_source_feed_rows"
C_TYPES = {"gas_ctx *": C.c_void_p, "const uint32_t *": C.c_void_p, "const void *": C.c_void_p, "int": C.c_int32, "uint32_t": C.c_uint32}


def header(name="gas_amd.h"):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def declared_args(text, name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", text, re.M)
    assert m, f"{name} is not declared"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    split = [re.match(r"(.*?)(\w+)$", a).groups() for a in args]
    return [(t.strip(), n) for t, n in split]


def test_header_declares_the_entry():
    args = declared_args(header(), NAME)
    assert [n for _, n in args] == ["ctx", "slots", "rows", "format", "channels", "n", "frames", "mem"]


def test_library_exports_and_capi_binds_the_headers_signature(gas):
    lib = gas.load_library()
    assert hasattr(lib, NAME) and NAME in gas.capi.EXPORTS
    want = [C_TYPES[t] for t, _ in declared_args(header(), NAME)]
    assert list(getattr(lib, NAME).argtypes) == want
    assert callable(getattr(gas.SpatializerContext, "source_feed_rows"))


def test_route_diagnostic_is_declared_exported_and_bound(gas):
    assert declared_args(header(), "gas_stream_last_fused") == [("gas_ctx *", "ctx")]
    lib = gas.load_library()
    assert hasattr(lib, "gas_stream_last_fused") and "gas_stream_last_fused" in gas.capi.EXPORTS
    assert callable(getattr(gas.SpatializerContext, "stream_last_fused"))


def test_header_comment_states_the_contract():
    h = header()
    end = h.index("int " + NAME + "(")
    comment = h[h.rindex("/*", 0, end):end]
    for word in ("GAS_PCM_S16", "GAS_PCM_F32", "GAS_MEM_HOST", "GAS_MEM_DEVICE", "GAS_FLAG_BATCHED_LAUNCH", "has_frames = 1", "draining", "gas_stream_positions", "replaces", "gas_source_free", "gas_source_reset", "gas_source_bind_stream", "GAS_ERR_INVALID_ARGUMENT", "GAS_ERR_BAD_SLOT", "GAS_ERR_FRAME_COUNT", "GAS_ERR_DEVICE"):
        assert word in comment, word


def test_no_new_format_and_the_abi_version_stays():
    h = header()
    assert re.search(r"#define GAS_ABI_VERSION 2\b", h)
    body = h[h.index("typedef enum gas_pcm_format"):]
    body = body[: body.index("} gas_pcm_format;")]
    assert re.findall(r"GAS_PCM_\w+ = (\d+)", body) == ["0", "1", "2", "3"]


def test_host_layer_declares_exports_and_binds_set_mixed(gas):
    args = declared_args(header("gas_amd_host.h"), "gas_host_set_mixed")
    assert args == [("gas_host *", "host"), ("int", "on")]
    lib = gas.load_library()
    assert hasattr(lib, "gas_host_set_mixed")
    assert callable(getattr(gas.capi.BatchedSpatializerHost, "set_mixed"))
    assert "unless gas_host_set_mixed opted in" in header("gas_amd_host.h")
