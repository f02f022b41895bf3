"""The compacted-entry packing and the lookup-table index
(renegade_amd/csrc/msm_digits.hpp) on the host: tests/host/entry_index_check.cpp
is a stand-alone program that round-trips (poly, w, i, mag, sign) through
(key, val), checks msm_lookup_index against ((w*N + i) << (c-1)) + mag - 1
for c = 8..10 and n = 2..32768, and checks the row guard on both sides of
2^31.  Built once plainly and once under the address and undefined-behaviour
sanitizers; nothing sanitized is loaded into Python."""
import shutil
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
HOST_SRC = REPO / "tests" / "host" / "entry_index_check.cpp"


def build_and_run(tmp_path, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / name
    cmd = [cxx, "-std=c++17", "-O1", *extra, str(HOST_SRC), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "entry_index_check ok" in r.stdout


def test_entry_index(tmp_path):
    build_and_run(tmp_path, "entry_index_check", [])


def test_entry_index_sanitized(tmp_path):
    build_and_run(tmp_path, "entry_index_check_san",
                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
