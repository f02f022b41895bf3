"""Permutation grand product z(X) on the GPU (perm_kernels.hip) vs a pure
Python model of the host loop, bit-exact (equality of u64 arrays, no
tolerance).

Boundaries of the implementation (perm_kernels.hip: PERM_WG = 256 threads,
PERM_EPT = 4 scan positions per thread, PERM_TILE = 1024 per workgroup,
PERM_MAX_TILES = 128 tiles per sequence) and the sizes on each side:
  - a thread's 4 positions partly / fully used:          n = 2      | n = 4
  - one thread / several threads / all 256 hold data:     n = 4 | 64, 256, 512 | 1024
  - one pass (single tile) -> reduce/prefix/apply passes: n = 1024   | n = 2048
  - tile-prefix workgroup partly / fully used:            n = 4096, 8192, 32768 | n = 131072
  - batch 1 / several proofs / the batch cap:             batch 1 | 5 | 128

The reference mirrors the host loop: running products, the batch-inverse
semantics with pow(total, R - 2, R) (a zero total gives zeros), z[0] = 1.
"""
import ctypes
import os
import random
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(REPO))

from tests import py_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

R = ref.R
U64P = ctypes.POINTER(ctypes.c_uint64)
RNG_OK, RNG_ERR_BAD_ARG = 0, -2
K5 = [pow(7, j, R) for j in range(5)]  # coset_ks (plonk_circuit.hpp)
SRS_POWER = 13                          # covers the settlement circuit (n = 4096)


def ptr(a):
    return a.ctypes.data_as(U64P)


def pack(vals):
    """canonical ints -> flat u64 array of Montgomery limbs"""
    buf = b"".join(ref.to_mont(v, R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).copy()


def unpack(a):
    """flat u64 array of Montgomery limbs -> canonical ints"""
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    rinv = pow(ref.R256, -1, R)
    return [int.from_bytes(b[i:i + 32], "little") * rinv % R for i in range(0, len(b), 32)]


def terms(wires, sigma, k5, beta, gamma, n):
    w = ref.fr_root_of_unity(n)
    num, den = [], []
    wi = 1
    for i in range(n):
        a = b = 1
        for j in range(5):
            wv = wires[j * n + i]
            a = a * (wv + beta * k5[j] * wi + gamma) % R
            b = b * (wv + beta * sigma[j * n + i] + gamma) % R
        num.append(a)
        den.append(b)
        wi = wi * w % R
    return num, den


def ref_z(wires, sigma, k5, beta, gamma, n):
    """The host loop on canonical ints: z of one proof."""
    num, den = terms(wires, sigma, k5, beta, gamma, n)
    pre, acc = [], 1
    for d in den:  # hbatch_inverse
        pre.append(acc)
        acc = acc * d % R
    inv = pow(acc, R - 2, R)
    dinv = [0] * n
    for i in range(n - 1, -1, -1):
        dinv[i] = inv * pre[i] % R
        inv = inv * den[i] % R
    z = [1] * n
    for i in range(1, n):
        z[i] = z[i - 1] * num[i - 1] % R * dinv[i - 1] % R
    return z


def gen_test_ptau(lib, power, seed=42):
    lib.rng_srs_test_ptau_size.restype = ctypes.c_uint64
    lib.rng_srs_test_ptau_size.argtypes = [ctypes.c_int]
    lib.rng_srs_gen_test_ptau.argtypes = [ctypes.c_int, ctypes.c_uint64,
                                          ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t]
    size = lib.rng_srs_test_ptau_size(power)
    assert size
    buf = (ctypes.c_uint8 * size)()
    assert lib.rng_srs_gen_test_ptau(power, seed, buf, size) == 0
    return bytes(buf)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("num_public", ctypes.c_uint64),
                ("selectors", U64P), ("sigma", U64P),
                ("num_link_groups", ctypes.c_uint64), ("link_offsets", U64P)]


def declare(lib):
    lib.rng_testcirc_build.restype = ctypes.c_void_p
    lib.rng_testcirc_build.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.rng_circ_build_settlement.restype = ctypes.c_void_p
    lib.rng_circ_build_settlement.argtypes = [ctypes.c_uint64]
    lib.rng_circ_n.restype = ctypes.c_uint64
    lib.rng_circ_n.argtypes = [ctypes.c_void_p]
    lib.rng_circ_npub.restype = ctypes.c_uint64
    lib.rng_circ_npub.argtypes = [ctypes.c_void_p]
    lib.rng_circ_get.argtypes = [ctypes.c_void_p, U64P, U64P, U64P, U64P]
    lib.rng_circ_free.argtypes = [ctypes.c_void_p]
    lib.rng_preprocess.restype = ctypes.c_void_p
    lib.rng_preprocess.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.rng_pk_free.argtypes = [ctypes.c_void_p]
    lib.rng_prove.argtypes = [ctypes.c_void_p, ctypes.c_void_p, U64P, U64P,
                              ctypes.c_uint64, U64P, U64P]
    lib.rng_prove_cohort.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                     U64P, U64P, U64P, U64P, U64P]


def build_circuit(lib, ctx, which):
    """-> dict(n, npub, sigma idx, wires, pubs, pk) for 'test' or 'settlement'"""
    h = (lib.rng_testcirc_build(777, 6) if which == "test"
         else lib.rng_circ_build_settlement(42))
    assert h
    n, npub = int(lib.rng_circ_n(h)), int(lib.rng_circ_npub(h))
    sel = np.zeros(13 * n * 4, dtype=np.uint64)
    sigma = np.zeros(5 * n, dtype=np.uint64)
    wires = np.zeros(5 * n * 4, dtype=np.uint64)
    pubs = np.zeros(max(1, npub * 4), dtype=np.uint64)
    lib.rng_circ_get(h, ptr(sel), ptr(sigma), ptr(wires), ptr(pubs))
    lib.rng_circ_free(h)
    assert n + 3 <= (1 << SRS_POWER) + 3
    pk = lib.rng_preprocess(ctx.h, ctypes.byref(Desc(n, npub, ptr(sel), ptr(sigma), 0, None)))
    assert pk, "rng_preprocess failed"
    return dict(n=n, npub=npub, sigma=sigma, wires=wires, pubs=pubs, pk=pk)


# ---------------------------------------------------------------- fixtures

@pytest.fixture(scope="module")
def plib():
    from renegade_amd import load_prover
    lib = load_prover()
    if not lib.gpu_available:
        pytest.skip("no GPU visible")
    declare(lib.lib)
    return lib


@pytest.fixture(scope="module")
def ctx(plib):
    c = plib.init(gen_test_ptau(plib.lib, SRS_POWER), (1 << SRS_POWER) + 2)
    yield c
    c.close()


def random_case(seed, n, batch):
    """-> (packed inputs, expected z as a (batch, n, 4) u64 array)"""
    rng = random.Random(seed)
    wires = [rng.randrange(R) for _ in range(5 * n * batch)]
    sigma = [rng.randrange(R) for _ in range(5 * n)]
    bg = [rng.randrange(R) for _ in range(2 * batch)]
    expect = []
    for p in range(batch):
        expect += ref_z(wires[5 * n * p:5 * n * (p + 1)], sigma, K5, bg[2 * p],
                        bg[2 * p + 1], n)
    return ((pack(wires), pack(sigma), pack(K5), pack(bg)),
            pack(expect).reshape(batch, n, 4))


def mismatch(got, expect):
    bad = np.nonzero((got != expect).any(axis=2))
    return f"first differing (proof, row): {list(zip(*[b[:6].tolist() for b in bad]))}"


# ------------------------------------------------------------------- cases

@pytest.mark.parametrize("n,batch", [(2, 1), (4, 1), (64, 1), (256, 1), (512, 1),
                                     (1024, 1), (2048, 1), (4096, 1), (8192, 1),
                                     (32768, 1), (131072, 1), (4096, 5), (64, 128)])
def test_random_vs_reference(ctx, n, batch):
    """Random wires AND random sigma (no permutation structure to hide an
    indexing error), each proof with its own beta and gamma."""
    args, expect = random_case(1000 + 7 * n + batch, n, batch)
    got = ctx.perm_product(*args, n, batch)
    assert np.array_equal(got, expect), mismatch(got, expect)


@pytest.mark.parametrize("n", [2, 512, 8192])
def test_identity_permutation(ctx, n):
    """sigma[j][t] = k_j w^t makes num == den row by row: z == 1 everywhere."""
    rng = random.Random(50 + n)
    w = ref.fr_root_of_unity(n)
    wp = [pow(w, t, R) for t in range(n)]
    sigma = [K5[j] * wp[t] % R for j in range(5) for t in range(n)]
    wires = [rng.randrange(R) for _ in range(5 * n)]
    bg = [rng.randrange(R), rng.randrange(R)]
    got = ctx.perm_product(pack(wires), pack(sigma), pack(K5), pack(bg), n, 1)
    expect = pack([1] * n).reshape(1, n, 4)
    assert np.array_equal(got, expect), mismatch(got, expect)


@pytest.mark.parametrize("which", ["test", "settlement"])
def test_real_permutation_pk(plib, ctx, which):
    """The provers' own round-2 call against a real key: device == host loop
    == reference, and the product wraps around: z[n-1] num(n-1) = den(n-1)."""
    c = build_circuit(plib.lib, ctx, which)
    try:
        n = c["n"]
        rng = random.Random(77)
        beta, gamma = rng.randrange(R), rng.randrange(R)
        bg = pack([beta, gamma])
        dev = ctx.perm_product_pk(c["pk"], c["wires"], bg, n, 1, mode=ctx.Z_DEVICE)
        host = ctx.perm_product_pk(c["pk"], c["wires"], bg, n, 1, mode=ctx.Z_HOST)
        auto = ctx.perm_product_pk(c["pk"], c["wires"], bg, n, 1, mode=ctx.Z_AUTO)
    finally:
        plib.lib.rng_pk_free(ctypes.c_void_p(c["pk"]))
    w = ref.fr_root_of_unity(n)
    wp = [pow(w, t, R) for t in range(n)]
    sigma = [K5[int(s) // n] * wp[int(s) % n] % R for s in c["sigma"]]
    wires = unpack(c["wires"])
    expect = ref_z(wires, sigma, K5, beta, gamma, n)
    assert np.array_equal(dev, host), mismatch(dev, host)
    assert np.array_equal(auto, host)
    assert np.array_equal(dev, pack(expect).reshape(1, n, 4))
    num, den = terms(wires, sigma, K5, beta, gamma, n)
    assert expect[n - 1] * num[n - 1] % R == den[n - 1]
    assert unpack(dev[0, n - 1])[0] * num[n - 1] % R == den[n - 1]
    assert any(v != 1 for v in expect)  # a real permutation, not the identity


@pytest.mark.parametrize("r", [0, 256, 511])
def test_zero_denominator(plib, ctx, r):
    """gamma = -(w[0][r] + beta sigma[0][r]) makes den(r) = 0: the host's
    batch inversion then yields z[0] = 1 and zeros after, with RNG_OK."""
    n = 512
    rng = random.Random(900 + r)
    wires = [rng.randrange(R) for _ in range(5 * n)]
    sigma = [rng.randrange(R) for _ in range(5 * n)]
    beta = rng.randrange(R)
    gamma = -(wires[r] + beta * sigma[r]) % R
    expect = ref_z(wires, sigma, K5, beta, gamma, n)
    assert expect == [1] + [0] * (n - 1)
    out = np.full(4 * n, 0xA5, dtype=np.uint64)
    a_w, a_s, a_k, a_bg = pack(wires), pack(sigma), pack(K5), pack([beta, gamma])
    rc = plib.lib.rng_perm_product(ctx.h, ptr(a_w), ptr(a_s), ptr(a_k), ptr(a_bg), n, 1,
                                   ptr(out))
    assert rc == RNG_OK
    assert np.array_equal(out, pack(expect))


def test_bad_arguments(plib, ctx):
    n = 8
    wires, sigma, k5, bg = pack([1] * 5 * n), pack([2] * 5 * n), pack(K5), pack([3, 4])
    out = np.full(4 * n, 0xA5, dtype=np.uint64)
    f = plib.lib.rng_perm_product

    def call(n_=n, batch=1, w=ptr(wires), s=ptr(sigma), k=ptr(k5), b=ptr(bg), o=ptr(out),
             c=ctx.h):
        return f(c, w, s, k, b, n_, batch, o)

    assert call() == RNG_OK  # the valid call the bad ones are variations of
    out[:] = 0xA5
    for kw in (dict(n_=3), dict(n_=0), dict(n_=1 << 18), dict(batch=0), dict(batch=129),
               dict(w=None), dict(s=None), dict(k=None), dict(b=None), dict(o=None),
               dict(c=None)):
        assert call(**kw) == RNG_ERR_BAD_ARG, kw
    assert (out == 0xA5).all()  # nothing ran


def test_threads(ctx):
    """Four threads at once, each with its own data: per-thread scratch and
    streams must not mix."""
    n = 4096
    cases = [random_case(4000 + t, n, 1) for t in range(4)]
    got = [None] * 4
    gate = threading.Barrier(4)

    def run(t):
        gate.wait()
        for _ in range(3):
            got[t] = ctx.perm_product(*cases[t][0], n, 1)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in range(4):
        assert got[t] is not None and np.array_equal(got[t], cases[t][1]), f"thread {t}"


# ------------------------------------------- prover paths agree (case 7)

def child_main(outfile):
    """Prove the test circuit (rng_prove) and the settlement circuit
    (rng_prove, rng_prove_cohort k = 3) under the inherited RNG_Z_DEVICE and
    save proofs and link hints."""
    from renegade_amd import load_prover
    plib = load_prover()
    plib.require_gpu()
    lib = plib.lib
    declare(lib)
    ctx = plib.init(gen_test_ptau(lib, SRS_POWER), (1 << SRS_POWER) + 2)
    out = {}
    for which, seed in (("test", 9), ("settlement", 7)):
        c = build_circuit(lib, ctx, which)
        n = c["n"]
        hint_len = 4 * (n + 2) + 9
        proof = np.zeros(157, dtype=np.uint64)
        hint = np.zeros(hint_len, dtype=np.uint64)
        rc = lib.rng_prove(ctx.h, ctypes.c_void_p(c["pk"]), ptr(c["wires"]), ptr(c["pubs"]),
                           seed, ptr(proof), ptr(hint))
        assert rc == 0, f"rng_prove({which}) rc={rc}"
        out[which + "_proof"], out[which + "_hint"] = proof, hint
        if which == "settlement":
            k = 3
            wires_all, pubs_all = np.tile(c["wires"], k), np.tile(c["pubs"], k)
            seeds = np.array([31, 32, 7], dtype=np.uint64)
            proofs = np.zeros(157 * k, dtype=np.uint64)
            hints = np.zeros(hint_len * k, dtype=np.uint64)
            rc = lib.rng_prove_cohort(ctx.h, ctypes.c_void_p(c["pk"]), k, ptr(wires_all),
                                      ptr(pubs_all), ptr(seeds), ptr(proofs), ptr(hints))
            assert rc == 0, f"rng_prove_cohort rc={rc}"
            out["cohort_proofs"], out["cohort_hints"] = proofs, hints
        lib.rng_pk_free(ctypes.c_void_p(c["pk"]))
    ctx.close()
    np.savez(outfile, **out)


def test_prover_paths_agree(plib, tmp_path):
    """RNG_Z_DEVICE=0 (host loops) and =1 (device stage) give the same proofs
    and link hints, element for element, from both provers.  The existing
    suite pins the default path against the oracle; this pins the other."""
    results = []
    for mode in ("0", "1"):
        outfile = tmp_path / f"z{mode}.npz"
        env = dict(os.environ, RNG_Z_DEVICE=mode)
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(outfile)],
                           cwd=str(REPO), env=env, timeout=300, capture_output=True,
                           text=True)
        # a failed child ends the test here: the second one is not started
        assert r.returncode == 0, f"RNG_Z_DEVICE={mode} child rc={r.returncode}\n{r.stderr[-2000:]}"
        results.append(np.load(outfile))
    host, dev = results
    assert sorted(host.files) == sorted(dev.files) and len(host.files) == 6
    for key in host.files:
        assert np.array_equal(host[key], dev[key]), f"{key} differs between the paths"
        assert host[key].any()
    # the cohort's third proof shares seed 7 with the single settlement proof
    assert np.array_equal(dev["cohort_proofs"][2 * 157:], dev["settlement_proof"])


if __name__ == "__main__":
    child_main(sys.argv[1])
