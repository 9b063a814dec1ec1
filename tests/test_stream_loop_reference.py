"""gas_stream_set_loop without a GPU: the index map of tests/stream_loop_ref.py against brute-force loops, and the new
entries' declaration, export and constants."""
import os
import re

import numpy as np
import pytest

import stream_loop_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 1200
MODES = [lref.LOOP_FORWARD, lref.LOOP_PINGPONG]


def brute_force(b, e, mode, count):
    """Walk the stream the way a player would: up to e, then back to b (FORWARD) or turn round (PINGPONG)."""
    out, pos, step = [], 0, 1
    for _ in range(count):
        out.append(pos)
        if mode == lref.LOOP_FORWARD:
            pos = b if pos + 1 == e else pos + 1
        elif step == 1 and pos + 1 == e:
            step = -1  # the end frame plays twice
        elif step == -1 and pos == b:
            step = 1  # ... and so does the first
        else:
            pos += step
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [1, 2, 37, 64, 511, 512, 513])
@pytest.mark.parametrize("b", [0, 123])
@pytest.mark.parametrize("tail", [0, 200])
def test_map_against_brute_force(mode, L, b, tail):
    e = b + L
    assert e + tail <= FRAMES
    count = b + 5 * L + 700
    want = brute_force(b, e, mode, count)
    got = lref.loop_map(np.arange(count), b, e, mode)
    np.testing.assert_array_equal(got, want)
    assert got.max() == e - 1 and got[b:].min() == b  # frames from e on never play
    for k in (0, b, b + L - 1, b + L, count - 1):
        assert int(lref.loop_map(k, b, e, mode)) == want[k]  # scalar form


@pytest.mark.parametrize("L", [1, 2, 37, 512])
def test_pingpong_period_and_symmetry(L):
    b, e = 50, 50 + L
    k = np.arange(b, b + 6 * L)
    m = lref.loop_map(k, b, e, lref.LOOP_PINGPONG)
    np.testing.assert_array_equal(m[: 4 * L], m[2 * L :])  # period 2L
    np.testing.assert_array_equal(m[:L], np.arange(b, e))
    np.testing.assert_array_equal(m[L : 2 * L], np.arange(b, e)[::-1])  # the way back mirrors the way there
    assert m[L - 1] == m[L] == e - 1 and m[2 * L - 1] == m[2 * L] == b  # both end frames twice
    f = lref.loop_map(k, b, e, lref.LOOP_FORWARD)
    np.testing.assert_array_equal(f[: 5 * L], f[L:])  # period L


def test_unroll():
    rng = np.random.default_rng(3)
    pcm = (rng.uniform(-1, 1, (300, 2)) * 32767).astype(np.int16)
    same = lref.unroll(pcm, 10, 20, lref.LOOP_DISABLED, 5000)
    assert same.dtype == pcm.dtype and np.array_equal(same, pcm)  # a DISABLED stream is the stream
    u = lref.unroll(pcm, 100, 0, lref.LOOP_FORWARD, 1000)  # end 0 = the stream's length
    assert u.shape == (1000, 2) and u.dtype == pcm.dtype
    np.testing.assert_array_equal(u[:300], pcm)
    np.testing.assert_array_equal(u[300:500], pcm[100:300])
    u = lref.unroll(pcm[:, 0], 100, 250, lref.LOOP_PINGPONG, 700)
    np.testing.assert_array_equal(u[:250], pcm[:250, 0])
    np.testing.assert_array_equal(u[250:400], pcm[100:250, 0][::-1])
    np.testing.assert_array_equal(u[400:550], pcm[100:250, 0])


def test_entries_are_declared_and_exported(gas):
    header = open(os.path.join(ROOT, "include", "gas_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int gas_stream_set_loop\(gas_ctx \*ctx, uint32_t stream, int mode, uint64_t loop_begin, uint64_t loop_end\);", code)
    assert re.search(r"int gas_stream_get_loop\(gas_ctx \*ctx, uint32_t stream, int \*\w+, uint64_t \*\w+, uint64_t \*\w+\);", code)
    lib = gas.load_library()
    for name in ("gas_stream_set_loop", "gas_stream_get_loop"):
        assert hasattr(lib, name) and name in gas.capi.EXPORTS
    assert lib.gas_abi_version() == 2  # two entry points more, nothing else


def test_loop_constants_equal_the_headers(gas):
    K = gas.capi
    header = open(os.path.join(ROOT, "include", "gas_amd.h")).read()
    for name, py in (("DISABLED", K.LOOP_DISABLED), ("FORWARD", K.LOOP_FORWARD), ("PINGPONG", K.LOOP_PINGPONG)):
        m = re.search(r"\bGAS_LOOP_%s = (\d+)," % name, header)
        assert m and int(m.group(1)) == py == getattr(lref, "LOOP_" + name)
