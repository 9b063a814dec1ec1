"""csrc/gas_switches.h -- the one reader of the environment's run-time switches, which gas_ctx_create calls once per
context -- in a stand-alone program (tests/switches_host_program.cpp, its own main, plain g++, no HIP) built with
-fsanitize=address,undefined -fno-sanitize-recover=all and run as an ordinary child process.  For every variable: unset,
"0", "1" and its further legal values against the meanings written out below (those of the scattered readers this
header replaced); and a second fill after setenv must see the new value."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

# variable -> (field, {value in the environment (None: unset): the field's value})
MEANING = {
    "GAS_STREAM_ROWS_FIRST": ("rows_first", {None: 0, "0": 0, "1": 1}),
    "GAS_ADPCM_SPAN": ("adpcm_span", {None: 1, "0": 0, "1": 1}),
    "GAS_QOA_SPAN": ("qoa_span", {None: 1, "0": 0, "1": 1}),
    "GAS_UNI_FLT": ("uni_flt", {None: 1, "0": 0, "1": 1}),
    "GAS_UNI_ER": ("uni_er_mode", {None: 1, "0": 0, "1": 1, "2": 2}),
    "GAS_XCD_ORDER_AUTO_MIN": ("xcd_order_auto_min", {None: 0xFFFFFFFF, "0": 0, "1": 1, "4096": 4096, "65536": 65536, "4294967295": 0xFFFFFFFF}),
    "GAS_SHELF_SCAN": ("shelf_scan", {None: 1, "0": 0, "1": 1}),
    "GAS_BIQUAD_PIPE": ("biquad_pipe", {None: 1, "0": 0, "1": 1}),
}
DEFAULTS = {field: values[None] for field, values in MEANING.values()}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path_factory.mktemp("switches_host") / "switches_host_program")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "godot-audio-spatializer_amd", "csrc"), os.path.join(HERE, "switches_host_program.cpp"), "-o", exe])
    return exe


def fills(program, env, *args):
    """-> one {field: value} per line the program prints, run with none of the switches set but `env`."""
    clean = {k: v for k, v in os.environ.items() if k not in MEANING}
    out = subprocess.run([program, *args], text=True, capture_output=True, env=dict(clean, **env))
    assert out.stderr == "", out.stderr[-2000:]  # the sanitizers' reports go there
    assert out.returncode == 0, out.stdout[-200:]
    return [{k: int(v) for k, v in (item.split("=") for item in line.split())} for line in out.stdout.splitlines()]


def test_defaults_with_nothing_set(program):
    assert fills(program, {}) == [DEFAULTS]


@pytest.mark.parametrize("name", list(MEANING))
def test_every_value_means_what_it_meant(program, name):
    field, values = MEANING[name]
    for value, want in values.items():
        if value is not None:
            assert fills(program, {name: value}) == [dict(DEFAULTS, **{field: want})], (name, value)  # and no other field moves


@pytest.mark.parametrize("name", list(MEANING))
def test_a_second_fill_sees_the_new_value(program, name):
    field, values = MEANING[name]
    legal = [v for v in values if v is not None]
    for before, after in zip([None] + legal, legal + [None]):
        got = fills(program, {} if before is None else {name: before}, name, "-" if after is None else after)
        assert got == [dict(DEFAULTS, **{field: values[before]}), dict(DEFAULTS, **{field: values[after]})], (name, before, after)
