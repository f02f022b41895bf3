"""Round 3 of the prover on the GPU, through rng_quotient_pk (the coset
extension of 7k polynomials, k_quotient_batch, the inverse coset NTT and
k_quot_chunks_batch, against the key's own coset tables) vs the Python-int
model of tests/quotient_model.py, bit-exact (equality of u64 arrays, no
tolerance).  The model is proven without a GPU in tests/test_quotient_cpu.py.

Keys come from rng_preprocess on random columns: all 13 selector columns
random residues and sigma a random permutation of the 5n slots, so no column
and no slot is left unexercised; the inputs satisfy no circuit, so the
quotient coefficients from 5(n+2) up, which the chunk split drops, are live
and compared too.

Sizes (m = 8n is the transform size of the stage):
  n = 8    the smallest legal key: k_ntt_small, z_shift wraps for t >= 56
  n = 16   the second size at which the model is all naive bignum sums
  n = 128  m = 1024, the last single-pass NTT size
  n = 256  m = 2048, the first two-pass size and the filled-block kernels
  n = 512  m = 4096, a second two-pass shape; n + 3 = 515 straddles two
           256-thread blocks of the staging kernels
  k = 1, 3 and the cap 128 (at n = 8: an NTT batch of 896)
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
from tests import quotient_model as qm  # noqa: E402
from tests.test_perm_product import (Desc, build_circuit, declare, gen_test_ptau,  # noqa: E402
                                     pack, ptr, unpack)
from tests.test_quotient_cpu import assert_identity, satisfied_case  # noqa: E402

pytestmark = pytest.mark.gpu

R = ref.R
RNG_OK, RNG_ERR_BAD_ARG = 0, -2
AUTO, OUT_OF_PLACE, IN_PLACE = 0, 1, 2
SRS_POWER = 10
SIZES = [8, 16, 128, 256, 512]


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


def preprocess(plib, ctx, n, sel, sigma):
    """sel: 13 columns of n canonical ints, sigma: 5n slot indices -> pk"""
    sel_a = pack([v for col in sel for v in col])
    sig_a = np.array(sigma, dtype=np.uint64)
    pk = plib.lib.rng_preprocess(ctx.h, ctypes.byref(Desc(n, 0, ptr(sel_a), ptr(sig_a), 0, None)))
    assert pk, "rng_preprocess failed"
    return pk


def random_key_inputs(rng, n, only_column=None):
    sel = [[rng.randrange(R) if only_column in (None, s) else 0 for _ in range(n)]
           for s in range(qm.NUM_SEL)]
    sigma = list(range(5 * n))
    rng.shuffle(sigma)
    return sel, sigma


class Keys:
    """One random key per size, made on first use and shared by every test:
    the device handle and the model's tables."""

    def __init__(self, plib, ctx, orc):
        self.plib, self.ctx, self.orc, self.made = plib, ctx, orc, {}

    def get(self, n):
        if n not in self.made:
            sel, sigma = random_key_inputs(random.Random(9000 + n), n)
            model = qm.Key(qm.Transforms(qm.route_for(n), self.orc), n, sel, sigma)
            self.made[n] = (preprocess(self.plib, self.ctx, n, sel, sigma), model)
        return self.made[n]

    def free(self):
        for pk, _ in self.made.values():
            self.plib.lib.rng_pk_free(ctypes.c_void_p(pk))


@pytest.fixture(scope="module")
def keys(plib, ctx, orc):
    k = Keys(plib, ctx, orc)
    yield k
    k.free()


# ----------------------------------------------------------------- helpers

def random_inputs(rng, n, k):
    """Every proof its own polynomials (7 x (n+3)), challenges and blinders."""
    polys = [[[rng.randrange(R) for _ in range(n + 3)] for _ in range(7)] for _ in range(k)]
    chal = [[rng.randrange(R) for _ in range(3)] for _ in range(k)]
    blind = [[rng.randrange(R) for _ in range(4)] for _ in range(k)]
    return polys, chal, blind


def pack_inputs(polys, chal, blind):
    p = pack([c for proof in polys for poly in proof for c in poly])
    c = pack([v for ch in chal for v in ch])
    b = None if blind is None else pack([v for bl in blind for v in bl])
    return p, c, b


def run(ctx, pk, n, packed, mode, k):
    p, c, b = packed
    return ctx.quotient_pk(pk, p, c, n, k, blinders=b, mode=mode)


def model_outputs(model, polys, chal, blind):
    """-> (chunks (k, 5, n+3, 4), quot (k, 8n, 4)) as the hook lays them out"""
    n, k = model.n, len(polys)
    chunks, quot = [], []
    for p in range(k):
        c, q = qm.quotient(model, polys[p], *chal[p], None if blind is None else blind[p])
        chunks += [v for chunk in c for v in chunk]
        quot += q
    return pack(chunks).reshape(k, 5, n + 3, 4), pack(quot).reshape(k, 8 * n, 4)


def assert_same(got, want, what):
    """got, want: (chunks, quot) pairs; names the first differing
    (proof, chunk, coefficient) and (proof, quotient coefficient)."""
    if not np.array_equal(got[1], want[1]):
        bad = np.nonzero((got[1] != want[1]).any(axis=2))
        first = list(zip(*[b[:4].tolist() for b in bad]))
        pytest.fail(f"{what}: {len(bad[0])} quotient coefficients differ, first "
                    f"(proof, coeff): {first}")
    if not np.array_equal(got[0], want[0]):
        bad = np.nonzero((got[0] != want[0]).any(axis=3))
        first = list(zip(*[b[:4].tolist() for b in bad]))
        pytest.fail(f"{what}: {len(bad[0])} chunk coefficients differ, first "
                    f"(proof, chunk, coeff): {first}")


def check_against_model(ctx, pk, model, polys, chal, blind, what=""):
    """Both arms equal the model (hence each other), mode 0 equals them."""
    n, k = model.n, len(polys)
    want = model_outputs(model, polys, chal, blind)
    packed = pack_inputs(polys, chal, blind)
    for mode, name in ((OUT_OF_PLACE, "out-of-place arm"), (IN_PLACE, "in-place arm"),
                       (AUTO, "mode 0")):
        got = run(ctx, pk, n, packed, mode, k)
        assert_same(got, want, f"{what} n={n} k={k} {name} vs model")
    return want


# ------------------------------------------------------------------- cases

@pytest.mark.parametrize("n,k", [(n, k) for n in SIZES for k in (1, 3)] + [(8, 128)])
def test_random_vs_model(ctx, keys, n, k):
    pk, model = keys.get(n)
    polys, chal, blind = random_inputs(random.Random(100 * n + k), n, k)
    want = check_against_model(ctx, pk, model, polys, chal, blind)
    # the inputs satisfy no circuit: the part the chunk split drops is live
    assert want[1][:, 5 * (n + 2):].any()


def test_one_selector_at_a_time(plib, ctx, orc):
    """13 keys, each with one live selector column: a wrong column index in
    the gate equation shows under the name of the column."""
    n, k = 8, 13
    rng = random.Random(1300)
    polys, chal, blind = random_inputs(rng, n, k)
    names = ["LC0", "LC1", "LC2", "LC3", "MUL0", "MUL1", "HASH0", "HASH1", "HASH2", "HASH3",
             "O", "C", "ECC"]
    tf = qm.Transforms(qm.NAIVE)
    for s, name in enumerate(names):
        sel, sigma = random_key_inputs(rng, n, only_column=s)
        model = qm.Key(tf, n, sel, sigma)
        pk = preprocess(plib, ctx, n, sel, sigma)
        try:
            check_against_model(ctx, pk, model, polys, chal, blind, what=f"selector {name} only,")
        finally:
            plib.lib.rng_pk_free(ctypes.c_void_p(pk))


@pytest.mark.parametrize("n", [8, 128])
def test_special_values(ctx, keys, n):
    """Challenges from {0, 1, r-1} (all three zero included), blinders NULL /
    zero / r-1, and the degenerate polynomials, as proofs of one cohort each."""
    pk, model = keys.get(n)
    rng = random.Random(500 + n)
    rand_polys, _, _ = random_inputs(rng, n, 1)
    base = rand_polys[0]
    # challenges: every proof the same random polynomials
    chal = [[0, 0, 0], [1, 1, 1], [R - 1, R - 1, R - 1], [0, 1, R - 1], [R - 1, 0, 1],
            [1, R - 1, 0], [0, rng.randrange(R), rng.randrange(R)],
            [rng.randrange(R), 0, rng.randrange(R)], [rng.randrange(R), rng.randrange(R), 0]]
    k = len(chal)
    for blind in (None, [[0] * 4] * k, [[R - 1] * 4] * k):
        check_against_model(ctx, pk, model, [base] * k, chal, blind,
                            what=f"special challenges, blinders {blind and blind[0][0]},")
    # polynomials, under random challenges and blinders
    zero = [0] * (n + 3)
    one = [1] + [0] * (n + 2)
    top = [R - 1] * (n + 3)

    def with_pi(slot):  # PI nonzero in one evaluation slot only: v * L_slot
        evals = [0] * n
        evals[slot] = rng.randrange(1, R)
        return base[:6] + [model.tf.interpolate(evals) + [0, 0, 0]]

    polys = [[zero] * 7, base[:5] + [one] + [base[6]], [zero] * 5 + [one, zero], [top] * 7,
             with_pi(0), with_pi(n - 1)]
    _, chal, blind = random_inputs(rng, n, len(polys))
    want = check_against_model(ctx, pk, model, polys, chal, blind, what="special polynomials,")
    # all-zero wires, z and PI leave q_C - alpha^2 L1, which Z_H does not divide
    assert want[1][0, 5 * (n + 2):].any()


@pytest.mark.parametrize("slot", [0, 5, 6])
@pytest.mark.parametrize("p", [0, 4])
def test_cohort_slots_independent(ctx, keys, slot, p):
    """One coefficient of one slot of proof p changed: out_quot of proof p
    changes, the other four proofs stay byte-equal."""
    n, k = 16, 5
    pk, model = keys.get(n)
    rng = random.Random(1600)
    polys, chal, blind = random_inputs(rng, n, k)
    for mode in (OUT_OF_PLACE, IN_PLACE):
        before = run(ctx, pk, n, pack_inputs(polys, chal, blind), mode, k)
        changed = [[list(poly) for poly in proof] for proof in polys]
        changed[p][slot][n // 2] = (changed[p][slot][n // 2] + 1) % R
        after = run(ctx, pk, n, pack_inputs(changed, chal, blind), mode, k)
        for out in (0, 1):
            for other in range(k):
                same = np.array_equal(before[out][other], after[out][other])
                assert same == (other != p), (mode, out, other)
        assert_same(after, model_outputs(model, changed, chal, blind), "changed cohort vs model")


def test_satisfied_circuit_identity(plib, ctx, orc):
    """A real key and a satisfying witness: the quotient has no coefficient
    from 5(n+2) up, and the chunks recombine to num / Z_H at a random point,
    with num from the circuit's columns by Horner and the barycentric formula
    (no NTT and no coset table on the reference side)."""
    case = satisfied_case(plib.lib, orc, 4343)
    n = case["n"]
    c = build_circuit(plib.lib, ctx, "test")
    try:
        assert c["n"] == n and np.array_equal(c["sigma"], case["sigma_u64"])
        assert np.array_equal(c["wires"], case["wires_u64"])
        packed = pack_inputs([case["polys"]], [case["challenges"]], [case["blinders"]])
        outs = [run(ctx, c["pk"], n, packed, mode, 1) for mode in (OUT_OF_PLACE, IN_PLACE)]
    finally:
        plib.lib.rng_pk_free(ctypes.c_void_p(c["pk"]))
    assert_same(outs[0], outs[1], "out-of-place vs in-place arm")
    chunks, quot = outs[0]
    assert quot[0, :5 * (n + 2)].any()
    assert not quot[0, 5 * (n + 2):].any(), "the numerator is not divisible by Z_H"
    flat = unpack(chunks[0])
    assert_identity(case, [flat[i * (n + 3):(i + 1) * (n + 3)] for i in range(5)])


def test_shape_changes_on_one_thread(ctx, keys):
    """The scratch regrows and is reused across shapes, both directions."""
    def body():
        for n, k in ((8, 128), (512, 1), (8, 3), (256, 3)):
            pk, model = keys.get(n)
            polys, chal, blind = random_inputs(random.Random(31 * n + k), n, k)
            check_against_model(ctx, pk, model, polys, chal, blind, what="shape sequence,")

    # a thread of its own: its scratch starts empty whatever ran before
    err = []

    def guarded():
        try:
            body()
        except BaseException as e:  # noqa: BLE001 - carried to the test's thread
            err.append(e)

    th = threading.Thread(target=guarded)
    th.start()
    th.join()
    if err:
        raise err[0]


def test_threads(ctx, keys):
    """Four threads at once on one context, different (n, k): per-thread
    scratch and streams must not mix.  Each equals its own single-threaded
    result."""
    shapes = [(8, 5), (16, 3), (128, 2), (256, 1)]
    args, want = [], []
    for t, (n, k) in enumerate(shapes):
        pk, _ = keys.get(n)
        packed = pack_inputs(*random_inputs(random.Random(4400 + t), n, k))
        args.append((pk, n, packed, OUT_OF_PLACE if t % 2 else IN_PLACE, k))
        want.append(run(ctx, *args[t]))
    got = [None] * 4
    gate = threading.Barrier(4)

    def work(t):
        gate.wait()
        for _ in range(3):
            got[t] = run(ctx, *args[t])

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in range(4):
        assert got[t] is not None, f"thread {t}"
        assert_same(got[t], want[t], f"thread {t} vs single-threaded")


def test_bad_arguments(plib, ctx, keys):
    n = 8
    pk, _ = keys.get(n)
    p, c, b = pack_inputs(*random_inputs(random.Random(1), n, 1))
    chunks = np.full(4 * 5 * (n + 3), 0xA5, dtype=np.uint64)
    quot = np.full(4 * 8 * n, 0xA5, dtype=np.uint64)
    f = plib.lib.rng_quotient_pk

    def call(k=1, mode=1, pk_=pk, polys=ptr(p), chal=ptr(c), blind=ptr(b), oc=ptr(chunks),
             oq=ptr(quot), h=ctx.h):
        return f(h, ctypes.c_void_p(pk_) if pk_ else None, k, polys, chal, blind, mode, oc, oq)

    for kw in (dict(k=0), dict(k=129), dict(mode=3), dict(mode=-1), dict(pk_=None),
               dict(polys=None), dict(chal=None), dict(oc=None), dict(h=None)):
        assert call(**kw) == RNG_ERR_BAD_ARG, kw
    assert (chunks == 0xA5).all() and (quot == 0xA5).all()  # nothing ran
    # the two optional pointers: NULL blinders are zeros, NULL out_quot skips
    assert call(blind=None, oq=None) == RNG_OK
    assert (quot == 0xA5).all() and not (chunks == 0xA5).all()
    zeros = pack([0] * 4)
    want = chunks.copy()
    assert call(blind=ptr(zeros)) == RNG_OK
    assert np.array_equal(chunks, want)


# ------------------------------------------------ RNG_NTT_FILL arms (child)

def fill_child_main(outfile):
    """out_quot and the chunks at n = 256, k = 3 under the inherited
    RNG_NTT_FILL, from a fixed random key and fixed random inputs."""
    from renegade_amd import load_prover
    plib = load_prover()
    plib.require_gpu()
    declare(plib.lib)
    ctx = plib.init(gen_test_ptau(plib.lib, SRS_POWER), (1 << SRS_POWER) + 2)
    n, k = 256, 3
    sel, sigma = random_key_inputs(random.Random(9000 + n), n)
    pk = preprocess(plib, ctx, n, sel, sigma)
    packed = pack_inputs(*random_inputs(random.Random(2560), n, k))
    out = {}
    for mode in (OUT_OF_PLACE, IN_PLACE):
        out[f"chunks{mode}"], out[f"quot{mode}"] = run(ctx, pk, n, packed, mode, k)
    plib.lib.rng_pk_free(ctypes.c_void_p(pk))
    ctx.close()
    np.savez(outfile, **out)


def test_ntt_fill_arms(plib, tmp_path):
    """RNG_NTT_FILL=0 and =1 (the plain and the filled-block NTT kernels)
    give byte-equal quotients and chunks at n = 256, k = 3."""
    results = []
    for fill in ("0", "1"):
        outfile = tmp_path / f"fill{fill}.npz"
        env = dict(os.environ, RNG_NTT_FILL=fill)
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(outfile)],
                           cwd=str(REPO), env=env, timeout=300, capture_output=True, text=True)
        # a failed child ends the test here: the second one is not started
        assert r.returncode == 0, f"RNG_NTT_FILL={fill} child rc={r.returncode}\n{r.stderr[-2000:]}"
        results.append(dict(np.load(outfile)))
    plain, filled = results
    assert sorted(plain) == sorted(filled) and len(plain) == 4
    for key in plain:
        assert np.array_equal(plain[key], filled[key]), f"{key} differs between the fill arms"
        assert plain[key].any()
    assert np.array_equal(plain["quot1"], plain["quot2"])


if __name__ == "__main__":
    fill_child_main(sys.argv[1])
