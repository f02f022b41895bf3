"""No-GPU side of the grand-product primitive: the entry points refuse
without a device, and the Python model the GPU tests compare against obeys
the properties it is trusted for."""
import ctypes
import random

import numpy as np
import pytest

from tests import py_ref as ref
from tests.test_perm_product import K5, pack, ref_z, terms, unpack

R = ref.R
U64P = ctypes.POINTER(ctypes.c_uint64)
ptr = lambda a: a.ctypes.data_as(U64P)
RNG_ERR_NO_GPU = -1


def test_refuses_without_gpu():
    from renegade_amd import load_prover
    plib = load_prover()
    if plib.gpu_available:
        pytest.skip("GPU present; refusal paths not reachable")
    buf = np.zeros(4 * 5 * 8, dtype=np.uint64)
    out = np.zeros(4 * 8, dtype=np.uint64)
    assert plib.lib.rng_perm_product(None, ptr(buf), ptr(buf), ptr(buf), ptr(buf), 8, 1,
                                     ptr(out)) == RNG_ERR_NO_GPU
    assert plib.lib.rng_perm_product_pk(None, None, ptr(buf), ptr(buf), 1, 1,
                                        ptr(out)) == RNG_ERR_NO_GPU
    assert not out.any()


def test_pack_roundtrip():
    vals = [0, 1, R - 1, 12345678901234567890123]
    a = pack(vals)
    assert a.dtype == np.uint64 and a.size == 16
    assert unpack(a) == vals
    assert list(a[4:8]) == ref.int_to_limbs(ref.to_mont(1, R))


def test_reference_model_properties():
    n = 16
    rng = random.Random(1)
    w = ref.fr_root_of_unity(n)
    wires = [rng.randrange(R) for _ in range(5 * n)]
    beta, gamma = rng.randrange(R), rng.randrange(R)
    ident = [K5[j] * pow(w, t, R) % R for j in range(5) for t in range(n)]
    assert ref_z(wires, ident, K5, beta, gamma, n) == [1] * n
    # a wire-value-preserving permutation: swap two slots that hold equal values
    wires[3] = wires[2 * n + 7]
    sigma = list(ident)
    sigma[3], sigma[2 * n + 7] = sigma[2 * n + 7], sigma[3]
    z = ref_z(wires, sigma, K5, beta, gamma, n)
    num, den = terms(wires, sigma, K5, beta, gamma, n)
    assert z[0] == 1 and any(v != 1 for v in z)
    for i in range(n):  # the recurrence, wrap-around included
        assert z[(i + 1) % n] * den[i] % R == z[i] * num[i] % R
    # a zero denominator zeroes everything after z[0]
    g0 = -(wires[5] + beta * sigma[5]) % R
    assert ref_z(wires, sigma, K5, beta, g0, n) == [1] + [0] * (n - 1)
