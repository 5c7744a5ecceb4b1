"""CPU: the host walk of the zstd level-3 dictionary parse (lzbench_amd/csrc/zstd_dfast_dict_parse.h) as a stand-alone
program under the host sanitizers (lzbench_amd/csrc/zstd_dfast_dict_walk_main.cpp): built here with
-fsanitize=address,undefined and run as a child process over the constructed pairs, dictionary and chunk in
exact-size heap buffers plus the 16 readable bytes.  Nothing is loaded into Python."""
import os
import shutil
import struct
import subprocess

import pytest

import zstd_dfast_dict_inputs as K

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lzbench_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("walk") / "zstd_dfast_dict_walk")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "zstd_dfast_dict_walk_main.cpp")],
                       capture_output=True, text=True)
    if r.returncode and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    assert r.returncode == 0, r.stderr
    return exe


def test_walk_over_the_constructed_pairs(program, tmp_path):
    C = K.constructed()
    path = tmp_path / "pairs.bin"
    with open(path, "wb") as f:
        for d, c, _, _ in C.values():
            f.write(struct.pack("<II", len(d), len(c)) + d.tobytes() + c.tobytes())
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1].endswith(f"{len(C)} pairs, every chunk rebuilt")
    for line, (name, (_, _, event, _)) in zip(lines, C.items()):
        counters = [int(x) for x in line.split("events")[1].split()]
        assert len(counters) == K.NEVENTS and counters[event] > 0, (name, line)


def test_walk_over_its_own_pairs(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
