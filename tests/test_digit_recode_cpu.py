"""The shared signed-digit recoding (renegade_amd/csrc/msm_digits.hpp) on
the host: tests/host/digit_recode_check.cpp is a stand-alone program that
calls msm_recode_digit for edge and random scalars at c = 8..13 and checks
magnitudes, the half rule, the digit sum and the top carry.  Built once
plainly and once under the address and undefined-behaviour sanitizers;
nothing sanitized is loaded into Python."""
import shutil
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
HOST_SRC = REPO / "tests" / "host" / "digit_recode_check.cpp"


def build_and_run(tmp_path, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / name
    cmd = [cxx, "-std=c++17", "-O1", *extra, str(HOST_SRC), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "digit_recode_check ok" in r.stdout


def test_digit_recode(tmp_path):
    build_and_run(tmp_path, "digit_recode_check", [])


def test_digit_recode_sanitized(tmp_path):
    build_and_run(tmp_path, "digit_recode_check_san",
                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
