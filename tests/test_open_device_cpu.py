"""No-GPU side of rounds 4 and 5 on the device: the entry points refuse
without a device, the Python model the GPU tests compare against obeys the
properties it is trusted for, and the three-piece host formulation in
plonk_rounds.hpp equals the single function it replaced (a stand-alone host
program, also run under the address and undefined-behaviour sanitizers;
nothing sanitized is loaded into Python)."""
import ctypes
import random
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import py_ref as ref
from tests.test_open_device import suffix_sums

REPO = Path(__file__).resolve().parent.parent
R = ref.R
U64P = ctypes.POINTER(ctypes.c_uint64)
ptr = lambda a: a.ctypes.data_as(U64P)
RNG_ERR_NO_GPU = -1


def test_refuses_without_gpu():
    from renegade_amd import load_prover
    plib = load_prover()
    horner, open_pk = plib.lib.rng_poly_horner, plib.lib.rng_open_pk  # exported
    if plib.gpu_available:
        pytest.skip("GPU present; refusal paths not reachable")
    buf = np.zeros(4 * 64, dtype=np.uint64)
    out = np.zeros(4 * 64, dtype=np.uint64)
    for mode in (0, 1):
        assert horner(None, ptr(buf), 8, 1, 1, 0, ptr(buf), mode, ptr(out)) == RNG_ERR_NO_GPU
    for mode in (0, 1, 2):
        assert open_pk(None, None, 1, ptr(buf), ptr(buf), ptr(buf), mode,
                       ptr(out)) == RNG_ERR_NO_GPU
    assert not out.any()


def test_wrappers_present():
    from renegade_amd.prover import ProverCtx
    assert callable(ProverCtx.poly_horner) and callable(ProverCtx.open_pk)
    assert (ProverCtx.OPEN_AUTO, ProverCtx.OPEN_DEVICE, ProverCtx.OPEN_HOST) == (0, 1, 2)
    assert (ProverCtx.HORNER_EVAL, ProverCtx.HORNER_DIVIDE) == (0, 1)


@pytest.mark.parametrize("length", [1, 2, 5, 17])
def test_model_properties(length):
    rng = random.Random(length)
    c = [rng.randrange(R) for _ in range(length)]
    for x in (rng.randrange(R), 0, 1, R - 1):
        s = suffix_sums(c, x)
        assert len(s) == length
        # S[0] is the evaluation
        assert s[0] == sum(cj * pow(x, j, R) for j, cj in enumerate(c)) % R
        # c(X) = q(X) (X - x) + S[0], coefficient by coefficient
        q = s[1:]
        prod = [0] * length
        for i, qi in enumerate(q):
            prod[i + 1] = (prod[i + 1] + qi) % R
            prod[i] = (prod[i] - x * qi) % R
        prod[0] = (prod[0] + s[0]) % R
        assert prod == c
        if x == 0:  # the shift
            assert q == c[1:] and s[0] == c[0]


HOST_SRC = REPO / "tests" / "host" / "open_rounds_check.cpp"


def build_and_run(tmp_path, name, extra):
    """Compile the stand-alone host program with the host compiler (the HIP
    headers are only read for their host-side definitions) and run it."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / name
    rocm = Path(shutil.which("hipcc")).resolve().parent.parent if shutil.which("hipcc") \
        else Path("/opt/rocm")
    cmd = [cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{rocm / 'include'}",
           *extra, str(HOST_SRC), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "open_rounds_check ok" in r.stdout


def test_three_piece_rounds_equal_single_function(tmp_path):
    build_and_run(tmp_path, "open_rounds_check", [])


def test_three_piece_rounds_sanitized(tmp_path):
    build_and_run(tmp_path, "open_rounds_check_san",
                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
