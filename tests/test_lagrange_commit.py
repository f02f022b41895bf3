"""Round-1 commitments on the Lagrange path (lagrange_kernels.hip: G1 inverse
NTT for the bases, compacted non-zero digits) vs the CPU oracle, bit-exact.

Everything runs through rng_commit_lagrange, i.e. the same msm_lagrange_run
call both provers make.  The expected value always comes from the oracle:
orc.ntt(..., inverse=True) of the evaluations, the blinding applied here as
k_blind_wires_batch applies it, then orc.msm over the first n + 2 SRS
records.

The G1 NTT kernels take one path for every n (one launch per radix-2 pass,
no size threshold), so the domain sizes below are the issue's 2, 4, 64, 1024
plus 8 and 512 for a pass count in between.
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
CS = (8, 10, 13)  # window sizes with table support
IDENTITY = np.array([0] * 8 + [1], dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(U64P)


@pytest.fixture(scope="module")
def plib():
    from renegade_amd import load_prover
    lib = load_prover()
    if not lib.gpu_available:
        pytest.skip("no GPU visible")
    return lib


@pytest.fixture(scope="module")
def srs10(orc):
    ptau = orc.srs_generate_ptau(10, seed=42)
    g1, _, _ = orc.srs_parse(ptau, (1 << 10) + 2)
    return ptau, g1


@pytest.fixture(scope="module")
def ctx(plib, srs10):
    ptau, _ = srs10
    c = plib.init(ptau, (1 << 10) + 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_c(plib, srs10):
    """One context per explicit window size: a domain keeps window tables for
    two values of c (the sparse and the dense choice), and the tests below
    put all three table-backed sizes through the same domains."""
    ptau, _ = srs10
    ctxs = {c: plib.init(ptau, (1 << 10) + 2) for c in CS}
    yield ctxs
    for c in ctxs.values():
        c.close()


def pack(vals):
    """canonical ints -> flat canonical u64 array (4 per value)"""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        assert 0 <= v < R
        if v:
            out[i] = ref.int_to_limbs(v)
    return out.reshape(-1)


def expected(orc, g1, evals, blinders, n):
    """Oracle commitment of one poly: inverse NTT of the evaluations, the
    blinding of k_blind_wires_batch, MSM over the first n + 2 SRS records."""
    data = np.zeros(4 * n, dtype=np.uint64)
    for i, v in enumerate(evals):
        if v:
            data[4 * i:4 * i + 4] = ref.int_to_limbs(ref.to_mont(v, R))
    orc.ntt(data, n, inverse=True)
    wp = [ref.from_mont(ref.limbs_to_int(data[4 * i:4 * i + 4]), R) for i in range(n)]
    wp += [0, 0]
    b0, b1 = blinders
    wp[0] = (wp[0] - b0) % R
    wp[1] = (wp[1] - b1) % R
    wp[n] = (wp[n] + b0) % R
    wp[n + 1] = (wp[n + 1] + b1) % R
    bases = np.ascontiguousarray(g1[:n + 2]).reshape(-1)
    return orc.msm(bases, pack(wp), n + 2, window_c=8)


def commit(ctx, polys, blinders, n, c=0):
    flat = np.concatenate([pack(p) for p in polys])
    bl = None
    if blinders is not None:
        bl = np.concatenate([pack(list(b)) for b in blinders])
    return ctx.commit_lagrange(flat, n, len(polys), blinders=bl, window_c=c)


def check(ctx, orc, g1, polys, blinders, n, c=0):
    got = commit(ctx, polys, blinders, n, c)
    bl = blinders if blinders is not None else [(0, 0)] * len(polys)
    exp = np.stack([expected(orc, g1, p, b, n) for p, b in zip(polys, bl)])
    bad = [b for b in range(len(polys)) if not np.array_equal(got[b], exp[b])]
    assert not bad, f"n={n} c={c}: records {bad} differ from the oracle"
    return got, exp


def unit(n, i):
    e = [0] * n
    e[i] = 1
    return e


def sparse_poly(rng, n):
    """settlement-like: 80 % zeros, some ones, some values below 2^64, a few
    full-width"""
    out = []
    for _ in range(n):
        u = rng.random()
        if u < 0.80:
            out.append(0)
        elif u < 0.91:
            out.append(1)
        elif u < 0.99:
            out.append(rng.randrange(1 << 64))
        else:
            out.append(rng.randrange(R))
    return out


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


# ----------------------------------------------------------- bases

@pytest.mark.parametrize("n", [2, 4, 8, 64])
def test_every_base(ctx, orc, srs10, n):
    """e_i commits to [L_i(tau)]: every i, one batch."""
    _, g1 = srs10
    check(ctx, orc, g1, [unit(n, i) for i in range(n)], None, n)


@pytest.mark.parametrize("n", [512, 1024])
def test_bases_large(ctx, orc, srs10, n):
    _, g1 = srs10
    rng = random.Random(77 + n)
    idx = [0, 1, n // 2, n - 1] + rng.sample(range(2, n - 1), 8)
    check(ctx, orc, g1, [unit(n, i) for i in idx], None, n)


@pytest.mark.parametrize("n", [2, 4, 64, 1024])
def test_blinding_bases(ctx, orc, srs10, n):
    """zero evaluations: blinders (1, 0) give [tau^n] - [tau^0], (0, 1) give
    [tau^(n+1)] - [tau^1]"""
    _, g1 = srs10
    got, _ = check(ctx, orc, g1, [[0] * n, [0] * n], [(1, 0), (0, 1)], n)
    assert got[0][8] == 0 and got[1][8] == 0 and not np.array_equal(got[0], got[1])


# ------------------------------------------------------ compaction

@pytest.mark.parametrize("c", CS)
def test_all_zero_batch(ctx_c, c):
    n = 64
    got = commit(ctx_c[c], [[0] * n] * 3, None, n, c)
    for b in range(3):
        assert np.array_equal(got[b], IDENTITY)


@pytest.mark.parametrize("c", CS)
def test_compaction_edges(ctx_c, orc, srs10, c):
    _, g1 = srs10
    n = 256  # n ones: one bucket of 256 entries, past the 128-entry cap
    rng = random.Random(1300 + c)
    half = 1 << (c - 1)
    full_digits = (1 << (c * (253 // c))) - 1  # every digit 2^c-1: carry chain
    special = [1, 2, R - 1, R - 2, (1 << 253) - 1, (1 << 128) - 1,
               half,             # digit == half: stays positive, no carry
               half + 1,         # negative digit with carry
               (1 << c) + half,
               full_digits]
    edges = [0] * n
    for p, s in zip(rng.sample(range(n), len(special)), special):
        edges[p] = s
    single = [0] * n
    single[rng.randrange(n)] = rng.randrange(1, R)
    polys = [rand_poly(rng, n),
             [0] * n,          # all-zero poly inside a non-zero batch
             single,           # exactly one non-zero value
             [1] * n,
             [R - 1] * n,
             edges,
             sparse_poly(rng, n)]
    got, _ = check(ctx_c[c], orc, g1, polys, None, n, c)
    assert np.array_equal(got[1], IDENTITY)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("B", [1, 5, 13])
def test_mixed_batches(ctx_c, orc, srs10, B, c):
    """dense random polys next to settlement-like sparse ones, with blinders"""
    _, g1 = srs10
    n = 128
    rng = random.Random(2100 + 16 * c + B)
    polys = [rand_poly(rng, n) if b % 3 == 0 else sparse_poly(rng, n) for b in range(B)]
    blinders = [(rng.randrange(R), rng.randrange(R)) for _ in range(B)]
    check(ctx_c[c], orc, g1, polys, blinders, n, c)


@pytest.mark.parametrize("c", CS)
def test_cohort_sized_batch(ctx_c, orc, srs10, c):
    """B = 240 (5 wires x 48 proofs) at n = 64"""
    _, g1 = srs10
    n, B = 64, 240
    rng = random.Random(2400 + c)
    polys = [rand_poly(rng, n) if b % 7 == 0 else sparse_poly(rng, n) for b in range(B)]
    polys[17] = [0] * n
    blinders = [(rng.randrange(R), rng.randrange(R)) for _ in range(B)]
    blinders[17] = (0, 0)
    got, _ = check(ctx_c[c], orc, g1, polys, blinders, n, c)
    assert np.array_equal(got[17], IDENTITY)


def test_auto_window_rule(ctx, orc, srs10):
    """window_c = 0: the prover's own rule, on a sparse and on a dense batch
    at the largest domain of this SRS"""
    _, g1 = srs10
    n = 1024
    rng = random.Random(5150)
    blinders = [(rng.randrange(R), rng.randrange(R)) for _ in range(5)]
    check(ctx, orc, g1, [sparse_poly(rng, n) for _ in range(5)], blinders, n)
    check(ctx, orc, g1, [rand_poly(rng, n) for _ in range(5)], blinders, n)


# ---------------------------------------------------- bad arguments

def test_bad_arguments(plib, ctx):
    n = 64
    evals = pack([1] * n)
    out = np.full(9, 0xA5, dtype=np.uint64)
    f = plib.lib.rng_commit_lagrange
    assert f(ctx.h, n, ptr(evals), None, 1, 0, ptr(out)) == RNG_OK
    out[:] = 0xA5
    big = pack([1] * 2048)  # n + 2 > srs_count (1027)
    assert f(ctx.h, 2048, ptr(big), None, 1, 0, ptr(out)) == RNG_ERR_BAD_ARG
    assert f(ctx.h, n, ptr(evals), None, 0, 0, ptr(out)) == RNG_ERR_BAD_ARG  # B = 0
    assert f(ctx.h, 48, ptr(evals), None, 1, 0, ptr(out)) == RNG_ERR_BAD_ARG  # not 2^k
    assert f(ctx.h, n, ptr(evals), None, 1, 7, ptr(out)) == RNG_ERR_BAD_ARG   # c < 8
    assert f(ctx.h, n, None, None, 1, 0, ptr(out)) == RNG_ERR_BAD_ARG
    assert (out == 0xA5).all()  # nothing ran


# ---------------------------------------------------------- threads

def test_threads_race_lazy_build(plib, orc, srs10):
    """Four threads on one FRESH context commit the same batch at once: they
    race the lazy build of the bases and the table."""
    ptau, g1 = srs10
    n, B = 1024, 3
    rng = random.Random(6060)
    polys = [sparse_poly(rng, n), rand_poly(rng, n), [1] * n]
    blinders = [(rng.randrange(R), rng.randrange(R)) for _ in range(B)]
    exp = np.stack([expected(orc, g1, p, b, n) for p, b in zip(polys, blinders)])
    fresh = plib.init(ptau, (1 << 10) + 2)
    got = [None] * 4
    gate = threading.Barrier(4)

    def run(t):
        gate.wait()
        got[t] = commit(fresh, polys, blinders, n)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    fresh.close()
    for t in range(4):
        assert got[t] is not None and np.array_equal(got[t], exp), f"thread {t}"


# ---------------------------------------------- prover paths agree

def child_main(outfile):
    """Prove the small test circuit and the settlement circuit through
    rng_prove and through rng_prove_cohort (k = 3) under the inherited
    RNG_R1_LAGRANGE; save proofs and link hints.  A marker line on stderr
    precedes every call, so the parent can tell from the RNG_MSM_DEBUG lines
    which commitments took the compacted path."""
    from renegade_amd import load_prover
    from tests.test_perm_product import SRS_POWER, build_circuit, declare, gen_test_ptau
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
        print(f"@@ {which} single n={n}", file=sys.stderr, flush=True)
        rc = lib.rng_prove(ctx.h, ctypes.c_void_p(c["pk"]), ptr(c["wires"]), ptr(c["pubs"]),
                           seed, ptr(proof), ptr(hint))
        assert rc == 0, f"rng_prove({which}) rc={rc}"
        out[which + "_proof"], out[which + "_hint"] = proof, hint
        k = 3
        wires_all, pubs_all = np.tile(c["wires"], k), np.tile(c["pubs"], k)
        seeds = np.array([31, 32, seed], dtype=np.uint64)
        proofs = np.zeros(157 * k, dtype=np.uint64)
        hints = np.zeros(hint_len * k, dtype=np.uint64)
        print(f"@@ {which} cohort n={n}", file=sys.stderr, flush=True)
        rc = lib.rng_prove_cohort(ctx.h, ctypes.c_void_p(c["pk"]), k, ptr(wires_all),
                                  ptr(pubs_all), ptr(seeds), ptr(proofs), ptr(hints))
        assert rc == 0, f"rng_prove_cohort({which}) rc={rc}"
        out[which + "_cohort_proofs"], out[which + "_cohort_hints"] = proofs, hints
        # the cohort's third proof shares its seed with the single proof
        assert np.array_equal(proofs[2 * 157:], proof), which
        lib.rng_pk_free(ctypes.c_void_p(c["pk"]))
    print("@@ end", file=sys.stderr, flush=True)
    ctx.close()
    np.savez(outfile, **out)


def compacted_by_section(stderr):
    """marker -> number of '(compacted)' MSM debug lines that followed it"""
    counts, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("@@ "):
            cur = " ".join(line.split()[1:3])
            counts[cur] = 0
        elif cur is not None and line.startswith("[msm]") and "(compacted)" in line:
            counts[cur] += 1
    return counts


def test_prover_paths_agree(plib, tmp_path):
    """RNG_R1_LAGRANGE=0 (coefficient commit) and =1 (Lagrange commit) give
    the same proofs and link hints, byte for byte, from rng_prove and
    rng_prove_cohort (k = 3) on the small test circuit and on the settlement
    circuit.  The provers fall back to the coefficient path silently where a
    domain has no bases or the witness is dense, so the RNG_MSM_DEBUG lines
    must show that with =1 both settlement calls really committed on the
    compacted path (exactly one MSM each: round 1), and with =0 none did."""
    results, compacted = [], []
    for mode in ("0", "1"):
        outfile = tmp_path / f"lag{mode}.npz"
        env = dict(os.environ, RNG_R1_LAGRANGE=mode, RNG_MSM_DEBUG="1")
        env.pop("RNG_MSM_C", None)
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(outfile)],
                           cwd=str(REPO), env=env, timeout=300, capture_output=True,
                           text=True)
        # a failed child ends the test here: the second one is not started
        assert r.returncode == 0, (f"RNG_R1_LAGRANGE={mode} child rc={r.returncode}\n"
                                   f"{r.stderr[-2000:]}")
        results.append(np.load(outfile))
        compacted.append(compacted_by_section(r.stderr))
    coeff, lag = results
    assert sorted(coeff.files) == sorted(lag.files) and len(coeff.files) == 8
    for key in coeff.files:
        assert np.array_equal(coeff[key], lag[key]), f"{key} differs between the paths"
        assert coeff[key].any()
    assert not any(compacted[0].values()), compacted[0]
    assert compacted[1]["settlement single"] == 1, compacted[1]
    assert compacted[1]["settlement cohort"] == 1, compacted[1]


if __name__ == "__main__":
    child_main(sys.argv[1])
