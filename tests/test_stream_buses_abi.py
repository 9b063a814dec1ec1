"""gas_process_block_streams_buses through the layers that need no GPU: declared in include/gas_amd.h, exported by the
library, bound by capi; and gas_stream_positions documented as answering for either stream entry."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gas_process_block_streams_buses"


def header():
    with open(os.path.join(ROOT, "include", "gas_amd.h")) as f:
        return f.read()


def test_header_declares_the_entry():
    m = re.search(r"^int " + NAME + r"\(([^;]*)\);", header(), re.M)
    assert m, "not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    names = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["ctx", "slots", "n", "frames", "out", "n_buses", "peaks", "has_frames", "mem"]


def test_library_exports_and_capi_binds(gas):
    lib = gas.load_library()
    assert hasattr(lib, NAME) and NAME in gas.capi.EXPORTS
    assert len(getattr(lib, NAME).argtypes) == 9
    assert callable(getattr(gas.SpatializerContext, "process_block_streams_buses"))


def test_stream_positions_comment_names_both_entries():
    h = header()
    end = h.index("int gas_stream_positions(")
    comment = h[h.rindex("/*", 0, end):end]
    assert "gas_process_block_streams" in re.sub(NAME, "", comment) and NAME in comment
