"""No-GPU side of the round-3 hook: rng_quotient_pk refuses without a device,
and the Python model that judges the kernels (tests/quotient_model.py) is
itself proven first: its naive bignum route and its orc.ntt route agree where
both can run, and on a satisfied circuit its quotient has no coefficient from
5(n+2) up and its chunks satisfy the quotient identity at a random point,
where the numerator is computed from the circuit's columns by Horner and the
barycentric formula alone (no transform, no coset table)."""
import random
from pathlib import Path

import numpy as np
import pytest

from tests import py_ref as ref
from tests import quotient_model as qm
from tests.test_perm_product import declare, ptr, ref_z, unpack

REPO = Path(__file__).resolve().parent.parent
R = ref.R
RNG_ERR_NO_GPU = -1


def test_generator_is_the_headers():
    text = (REPO / "include" / "bn254_params.h").read_text()
    assert f"#define FR_GENERATOR {qm.G}\n" in text
    assert qm.G == ref.FR_GEN


def test_refuses_without_gpu():
    from renegade_amd import load_prover
    plib = load_prover()
    f = plib.lib.rng_quotient_pk  # exported
    if plib.gpu_available:
        pytest.skip("GPU present; refusal paths not reachable")
    buf = np.zeros(4 * 7 * 11, dtype=np.uint64)
    out = np.zeros(4 * 64, dtype=np.uint64)
    for mode in (0, 1, 2):
        assert f(None, None, 1, ptr(buf), ptr(buf), None, mode, ptr(out),
                 ptr(out)) == RNG_ERR_NO_GPU
    assert not out.any()


def test_wrapper_present():
    from renegade_amd.prover import ProverCtx
    assert callable(ProverCtx.quotient_pk)
    assert (ProverCtx.QUOT_AUTO, ProverCtx.QUOT_OUT_OF_PLACE, ProverCtx.QUOT_IN_PLACE) == (0, 1, 2)


def random_key_inputs(rng, n):
    sel = [[rng.randrange(R) for _ in range(n)] for _ in range(qm.NUM_SEL)]
    sigma = list(range(5 * n))
    rng.shuffle(sigma)
    return sel, sigma


@pytest.mark.parametrize("n", [8, 16])
def test_model_routes_agree(orc, n):
    rng = random.Random(300 + n)
    sel, sigma = random_key_inputs(rng, n)
    keys = [qm.Key(qm.Transforms(route, orc), n, sel, sigma) for route in (qm.NAIVE, qm.ORC)]
    for name in ("sel_coef", "sig_coef", "l1_coef", "sel_coset", "sig_coset", "l1_coset"):
        assert getattr(keys[0], name) == getattr(keys[1], name), name
    polys = [[rng.randrange(R) for _ in range(n + 3)] for _ in range(7)]
    ch = [rng.randrange(R) for _ in range(3)]
    bl = [rng.randrange(R) for _ in range(4)]
    naive, viaorc = (qm.quotient(k, polys, *ch, bl) for k in keys)
    assert naive == viaorc
    assert any(naive[1][5 * (n + 2):])  # no circuit is satisfied: the top part is live
    assert qm.route_for(n) == qm.NAIVE and qm.route_for(2 * qm.NAIVE_MAX_N) == qm.ORC


def test_model_pieces():
    """The helpers the identity rests on, against direct sums."""
    rng = random.Random(5)
    n = 8
    evals = [rng.randrange(R) for _ in range(n)]
    coef = qm.Transforms(qm.NAIVE).interpolate(evals)
    w = ref.fr_root_of_unity(n)
    assert [qm.horner(coef, pow(w, i, R)) for i in range(n)] == evals
    zeta = rng.randrange(R)
    assert qm.eval_from_evals(evals, zeta) == qm.horner(coef, zeta)
    assert qm.horner(coef, zeta) == sum(c * pow(zeta, j, R) for j, c in enumerate(coef)) % R
    # blinding adds a multiple of X^n - 1: the values on H stay
    bw = qm.blind_wire(coef, n, 11, 12)
    bz = qm.blind_z(coef, n, 13, 14, 15)
    assert len(bw) == len(bz) == n + 3 and bw[n + 2] == 0
    assert [qm.horner(bw, pow(w, i, R)) for i in range(n)] == evals
    assert [qm.horner(bz, pow(w, i, R)) for i in range(n)] == evals
    assert bz[0] == (coef[0] - 15) % R and bz[n + 2] == 13 and bw[1] == (coef[1] - 12) % R
    # the chunk blinders cancel in the recombination
    quot = [rng.randrange(R) for _ in range(5 * (n + 2))] + [0] * (8 * n - 5 * (n + 2))
    plain = qm.split_chunks(quot, n, None)
    blind = qm.split_chunks(quot, n, [21, 22, 23, 24])
    assert plain != blind and blind[1][0] == (plain[1][0] - 21) % R and blind[4][n + 2] == 0
    assert qm.chunks_at(plain, n, zeta) == qm.chunks_at(blind, n, zeta) == qm.horner(quot, zeta)


def satisfied_case(lib, orc, seed):
    """The test circuit (the one build_circuit(lib, ctx, "test") preprocesses)
    with blinded wires, z and PI as round 3 receives them.  Host code only."""
    declare(lib)
    h = lib.rng_testcirc_build(777, 6)
    assert h
    n, npub = int(lib.rng_circ_n(h)), int(lib.rng_circ_npub(h))
    sel_a = np.zeros(13 * n * 4, dtype=np.uint64)
    sigma = np.zeros(5 * n, dtype=np.uint64)
    wires_a = np.zeros(5 * n * 4, dtype=np.uint64)
    pubs_a = np.zeros(max(1, npub * 4), dtype=np.uint64)
    lib.rng_circ_get(h, ptr(sel_a), ptr(sigma), ptr(wires_a), ptr(pubs_a))
    lib.rng_circ_free(h)
    sel_flat, wires = unpack(sel_a), unpack(wires_a)
    sel = [sel_flat[s * n:(s + 1) * n] for s in range(13)]
    pubs = unpack(pubs_a)[:npub]
    rng = random.Random(seed)
    beta, gamma, alpha = (rng.randrange(R) for _ in range(3))
    sigma = [int(s) for s in sigma]
    z = ref_z(wires, qm.sigma_evals(sigma, n), qm.K5, beta, gamma, n)
    tf = qm.Transforms(qm.route_for(n), orc)
    polys = [qm.blind_wire(tf.interpolate(wires[j * n:(j + 1) * n]), n, rng.randrange(R),
                           rng.randrange(R)) for j in range(5)]
    polys.append(qm.blind_z(tf.interpolate(z), n, *(rng.randrange(R) for _ in range(3))))
    polys.append(tf.interpolate(pubs + [0] * (n - npub)) + [0, 0, 0])
    blinders = [rng.randrange(R) for _ in range(4)]
    return dict(n=n, sel=sel, sigma=sigma, sigma_u64=np.array(sigma, dtype=np.uint64),
                wires_u64=wires_a, polys=polys, challenges=[beta, gamma, alpha],
                blinders=blinders, tf=tf, zeta=rng.randrange(R))


def assert_identity(case, chunks):
    """(sum_i chunk_i(zeta) zeta^(i(n+2))) (zeta^n - 1) == num(zeta)"""
    n, zeta = case["n"], case["zeta"]
    num = qm.numerator_at(n, case["sel"], case["sigma"], case["polys"], *case["challenges"], zeta)
    assert num != 0
    assert qm.chunks_at(chunks, n, zeta) * (pow(zeta, n, R) - 1) % R == num


@pytest.fixture(scope="module")
def satisfied(orc):
    from renegade_amd import load_prover
    case = satisfied_case(load_prover().lib, orc, 4242)
    key = qm.Key(case["tf"], case["n"], case["sel"], case["sigma"])
    case["chunks"], case["quot"] = qm.quotient(key, case["polys"], *case["challenges"],
                                               case["blinders"])
    return case


def test_model_top_coefficients_vanish_on_satisfied_circuit(satisfied):
    n, quot = satisfied["n"], satisfied["quot"]
    assert len(quot) == 8 * n
    assert not any(quot[5 * (n + 2):])
    assert quot[5 * n + 7]  # blinded inputs: the quotient has its full degree, 5n + 7


def test_model_satisfies_quotient_identity(satisfied):
    assert_identity(satisfied, satisfied["chunks"])
    # and the check can fail: one coefficient off breaks it
    bad = [list(c) for c in satisfied["chunks"]]
    bad[2][1] = (bad[2][1] + 1) % R
    with pytest.raises(AssertionError):
        assert_identity(satisfied, bad)
