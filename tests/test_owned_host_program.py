"""csrc/gas_owned.h -- the one owner of a context's device buffers, pinned buffers and events -- against a fake runtime
(malloc / free, live objects counted per kind, the k-th allocation made to fail) in a stand-alone program
(tests/owned_host_program.cpp, its own main, plain g++) built with -fsanitize=address,undefined
-fno-sanitize-recover=all and run as an ordinary child process.  Every object must be freed exactly once on every path
-- drop, release_all, the destructor, a failed grow, a run of allocations that fails at any point -- and the sanitizers
must stay silent.  A second build with -fsanitize=thread runs the two-thread case.  These are the only checks of the
paths behind a failed runtime allocation: no GPU test provokes one."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def build(tmp_path_factory, name, sanitize):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path_factory.mktemp(name) / "owned_host_program")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + sanitize + ["-I" + os.path.join(ROOT, "godot-audio-spatializer_amd", "csrc"), os.path.join(HERE, "owned_host_program.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory, "owned_host", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def program_tsan(tmp_path_factory):
    return build(tmp_path_factory, "owned_host_tsan", ["-fsanitize=thread"])


def check(cmd, env=None):
    out = subprocess.run(cmd, text=True, capture_output=True, env=env)
    assert out.stderr == "", out.stderr[-4000:]  # the sanitizers' reports go there
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout[-2000:]


@pytest.mark.parametrize("case", ["basic", "grow", "fail_each", "refuse", "scope", "threads"])
def test_owner_frees_everything_exactly_once(program, case):
    check([program, case])


def test_two_threads_on_one_owner_under_tsan(program_tsan):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66")
    # GCC's ThreadSanitizer runtime expects the kernel's default 28 bits of mmap randomisation; where a kernel uses more,
    # the executable can be mapped outside its ranges ("FATAL: ThreadSanitizer: unexpected memory mapping").  Address
    # randomisation off for this one child process (setarch -R) keeps it in them.
    setarch = shutil.which("setarch")
    no_aslr = [setarch, platform.machine(), "-R"] if setarch else []
    if no_aslr and subprocess.run(no_aslr + ["true"], capture_output=True).returncode != 0:
        no_aslr = []  # the personality flag is not permitted here: run as before
    check(no_aslr + [program_tsan, "threads"], env=env)
