"""Rounds 4 and 5 on the GPU (open_kernels.hip): the batched Horner scan, the
combination kernel behind rng_open_pk and both provers under RNG_OPEN_DEVICE,
bit-exact (equality of u64 arrays, no tolerance).

Boundaries of the implementation (open_kernels.hip: OPEN_WG = 256 threads,
OPEN_EPT = 4 positions per thread, OPEN_TILE = 1024 per workgroup,
OPEN_MAX_LEN = 2^17 + 3, OPEN_MAX_TILES = 129 tiles per sequence,
OPEN_MAX_SEQ = 640 sequences per call) and the lengths on each side:
  - nothing to divide / the shortest quotient:              len 1 (evaluate only) | 2
  - a thread's 4 positions partly / fully / just over:      len 2, 3 | 4 | 5
  - thread 63 / 64 (the last lane of a wave and the next):  len 255, 256 | 257
  - one tile partly / fully used -> three launches:         len 1023 | 1024 | 1025, 1027
  - 3, 5, 9, 33 tiles (n + 3 at n = 2048 .. 32768):         len 2050, 4099, 8195, 32771
  - the tile-prefix workgroup at its cap of 129 totals:     len 131075
  - one sequence / per-item polys / shared polys:           (group, batch, shared) =
                                                            (1,1,0) | (5,3,0) | (4,3,1)
  - the sequence cap:                                       (5,128,0) = 640 at len 1027

The model is Python ints: S = 0; for c in reversed(coeffs): S = (c + x*S) % R.
S[0] is the evaluation, S[1:] the quotient by (X - x).
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
from tests.test_perm_product import (SRS_POWER, build_circuit, child_main, declare,  # noqa: E402
                                     gen_test_ptau, pack, ptr, unpack)

pytestmark = pytest.mark.gpu

R = ref.R
RNG_OK, RNG_ERR_BAD_ARG = 0, -2
EVAL, DIVIDE = 0, 1
MAX_LEN = (1 << 17) + 3
MAX_SEQ = 640
GOLD = REPO / "tests" / "golden"


def suffix_sums(coeffs, x):
    """The model: S[i] = c[i] + x S[i+1] for every i."""
    out = [0] * len(coeffs)
    s = 0
    for i in range(len(coeffs) - 1, -1, -1):
        s = (coeffs[i] + x * s) % R
        out[i] = s
    return out


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


def check_both_modes(ctx, polys, points, length, group, batch, shared):
    """polys: one coefficient list per sequence ((b, g) order, or g when
    shared); points: one per item.  Both modes against the model, and the
    two modes against each other."""
    flat = pack([c for poly in polys for c in poly])
    pts = pack(points)
    ev = ctx.poly_horner(flat, pts, length, group, batch, shared, mode=EVAL)
    want_ev, want_q = [], []
    for b in range(batch):
        for g in range(group):
            s = suffix_sums(polys[g if shared else b * group + g], points[b])
            want_ev.append(s[0])
            want_q += s[1:]
    want_ev = pack(want_ev).reshape(batch, group, 4)
    bad = np.nonzero((ev != want_ev).any(axis=2))
    assert np.array_equal(ev, want_ev), f"evaluations differ at (item, poly) {list(zip(*bad))[:6]}"
    if length == 1:
        return
    q = ctx.poly_horner(flat, pts, length, group, batch, shared, mode=DIVIDE)
    want_q = pack(want_q).reshape(batch, group, length - 1, 4)
    bad = np.nonzero((q != want_q).any(axis=3))
    assert np.array_equal(q, want_q), \
        f"quotients differ at (item, poly, coeff) {list(zip(*[b[:6].tolist() for b in bad]))}"
    # mode consistency on the device's own outputs: c[0] + x q[0] == c(x)
    q0 = unpack(q[:, :, 0, :])
    got_ev = unpack(ev)
    for b in range(batch):
        for g in range(group):
            c0 = polys[g if shared else b * group + g][0]
            assert (c0 + points[b] * q0[b * group + g]) % R == got_ev[b * group + g]


def random_polys(rng, count, length):
    return [[rng.randrange(R) for _ in range(length)] for _ in range(count)]


# ------------------------------------------------------- Horner scan cases

SMALL = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1027, 2050, 4099]
LARGE = [8195, 32771, 131075]
SHAPES = [(1, 1, False), (5, 3, False), (4, 3, True)]
CASES = ([(n, g, b, s) for n in SMALL for (g, b, s) in SHAPES] +
         [(n, 1, 2, False) for n in LARGE] + [(1027, 5, 128, False)])


@pytest.mark.parametrize("length,group,batch,shared", CASES)
def test_random_vs_model(ctx, length, group, batch, shared):
    rng = random.Random(7000 + 31 * length + 5 * group + batch)
    polys = random_polys(rng, group if shared else group * batch, length)
    points = [rng.randrange(R) for _ in range(batch)]
    check_both_modes(ctx, polys, points, length, group, batch, shared)


@pytest.mark.parametrize("length", [1027, 4099])
def test_special_points(ctx, length):
    """0, 1, R - 1 and the 1024-th and 4096-th roots of unity (x^1024 = 1
    makes every tile multiplier of the prefix pass 1), five items of one call."""
    rng = random.Random(81 + length)
    points = [0, 1, R - 1, ref.fr_root_of_unity(1024), ref.fr_root_of_unity(4096)]
    polys = random_polys(rng, len(points), length)
    check_both_modes(ctx, polys, points, length, 1, len(points), False)
    # x = 0 read directly: the quotient is the shift, the evaluation c[0]
    flat, pts = pack(polys[0]), pack([0])
    q = ctx.poly_horner(flat, pts, length, mode=DIVIDE)
    assert np.array_equal(q.reshape(-1), flat[4:])
    assert np.array_equal(ctx.poly_horner(flat, pts, length, mode=EVAL).reshape(-1), flat[:4])


@pytest.mark.parametrize("length", [1027, 4099])
def test_special_polynomials(ctx, length):
    rng = random.Random(91 + length)
    only_c0 = [rng.randrange(1, R)] + [0] * (length - 1)
    only_top = [0] * (length - 1) + [rng.randrange(1, R)]
    polys = [[0] * length, only_c0, only_top, [R - 1] * length]
    x = rng.randrange(R)
    check_both_modes(ctx, polys, [x], length, 4, 1, False)
    q = ctx.poly_horner(pack(only_c0), pack([x]), length, mode=DIVIDE)
    assert not q.any()  # a constant divided by (X - x) leaves only the remainder


def test_bad_arguments(plib, ctx):
    length = 8
    polys, pts = pack(list(range(1, 1 + 2 * length))), pack([3, 4])
    out = np.full(4 * 2 * length, 0xA5, dtype=np.uint64)
    f = plib.lib.rng_poly_horner

    def call(n_=length, group=1, batch=2, shared=0, mode=DIVIDE, p=ptr(polys), x=ptr(pts),
             o=ptr(out), c=ctx.h):
        return f(c, p, n_, group, batch, shared, x, mode, o)

    assert call() == RNG_OK  # the valid call the bad ones are variations of
    assert call(mode=EVAL) == RNG_OK
    out[:] = 0xA5
    for kw in (dict(p=None), dict(x=None), dict(o=None), dict(c=None), dict(n_=0),
               dict(n_=1), dict(n_=MAX_LEN + 1), dict(group=0), dict(batch=0),
               dict(group=MAX_SEQ // 2 + 1), dict(group=1 << 40, batch=1 << 40),
               dict(mode=2), dict(mode=-1)):
        assert call(**kw) == RNG_ERR_BAD_ARG, kw
    assert (out == 0xA5).all()  # nothing ran


def test_threads(ctx):
    """Four threads at once on one context, each with its own data:
    per-thread scratch and streams must not mix."""
    length = 4099
    rng = random.Random(4100)
    polys = [[rng.randrange(R) for _ in range(length)] for _ in range(4)]
    points = [rng.randrange(R) for _ in range(4)]
    want = [pack(suffix_sums(polys[t], points[t])) for t in range(4)]
    args = [(pack(polys[t]), pack([points[t]])) for t in range(4)]
    got = [None] * 4
    gate = threading.Barrier(4)

    def run(t):
        gate.wait()
        for _ in range(3):
            ev = ctx.poly_horner(*args[t], length, mode=EVAL)
            q = ctx.poly_horner(*args[t], length, mode=DIVIDE)
            got[t] = np.concatenate([ev.reshape(-1), q.reshape(-1)])

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in range(4):
        assert got[t] is not None and np.array_equal(got[t], want[t]), f"thread {t}"


# ------------------------------------------------- rng_open_pk on real keys

@pytest.fixture(scope="module", params=["test", "settlement"])
def circuit(request, plib, ctx):
    c = build_circuit(plib.lib, ctx, request.param)
    yield c
    plib.lib.rng_pk_free(ctypes.c_void_p(c["pk"]))


def open_inputs(rng, n, k, zero_scalars=False, zero_zeta=False):
    """-> (polys as lists, packed polys, points, scalars): the 11 polynomials
    of each proof with their true lengths, zero-padded to n + 3."""
    lens = [n + 2] * 5 + [n + 3] * 5 + [n + 2]
    polys = [[rng.randrange(R) for _ in range(m)] + [0] * (n + 3 - m)
             for _ in range(k) for m in lens]
    w = ref.fr_root_of_unity(n)
    points = []
    for _ in range(k):
        zeta = 0 if zero_zeta else rng.randrange(R)
        points += [zeta, zeta * w % R]
    scalars = [0 if zero_scalars else rng.randrange(R) for _ in range(29 * k)]
    return polys, pack([c for p in polys for c in p]), points, scalars


@pytest.mark.parametrize("k", [1, 3])
def test_open_pk_device_equals_host(ctx, circuit, k):
    n = circuit["n"]
    polys, flat, points, scalars = open_inputs(random.Random(600 + k), n, k)
    args = (circuit["pk"], flat, pack(points), pack(scalars), n, k)
    dev = ctx.open_pk(*args, mode=ctx.OPEN_DEVICE)
    host = ctx.open_pk(*args, mode=ctx.OPEN_HOST)
    auto = ctx.open_pk(*args, mode=ctx.OPEN_AUTO)
    bad = np.nonzero((dev != host).any(axis=3))
    assert np.array_equal(dev, host), \
        f"first differing (proof, W, coeff): {list(zip(*[b[:6].tolist() for b in bad]))}"
    assert np.array_equal(auto, host)
    assert dev.any()
    for p in range(k):  # W_zeta_w is the quotient of z alone: check it against the model
        z = polys[11 * p + 5]
        want = pack(suffix_sums(z, points[2 * p + 1])[1:]).reshape(n + 2, 4)
        assert np.array_equal(dev[p, 1], want)


def test_open_pk_zero_scalars(ctx, circuit):
    """All 29 scalars zero: W_zeta vanishes, W_zeta_w is still z's quotient."""
    n, k = circuit["n"], 3
    polys, flat, points, scalars = open_inputs(random.Random(610), n, k, zero_scalars=True)
    args = (circuit["pk"], flat, pack(points), pack(scalars), n, k)
    dev = ctx.open_pk(*args, mode=ctx.OPEN_DEVICE)
    assert np.array_equal(dev, ctx.open_pk(*args, mode=ctx.OPEN_HOST))
    assert not dev[:, 0].any()
    for p in range(k):
        want = pack(suffix_sums(polys[11 * p + 5], points[2 * p + 1])[1:]).reshape(n + 2, 4)
        assert np.array_equal(dev[p, 1], want)


def test_open_pk_zeta_zero(ctx, circuit):
    """zeta = 0 (so zeta*w = 0 too): both quotients are plain shifts."""
    n, k = circuit["n"], 1
    polys, flat, points, scalars = open_inputs(random.Random(620), n, k, zero_zeta=True)
    args = (circuit["pk"], flat, pack(points), pack(scalars), n, k)
    dev = ctx.open_pk(*args, mode=ctx.OPEN_DEVICE)
    assert np.array_equal(dev, ctx.open_pk(*args, mode=ctx.OPEN_HOST))
    assert np.array_equal(dev[0, 1].reshape(-1), pack(polys[5][1:]))
    assert dev[0, 0].any()


def test_open_pk_bad_arguments(plib, ctx, circuit):
    n = circuit["n"]
    _, flat, points, scalars = open_inputs(random.Random(630), n, 1)
    pts, sc = pack(points), pack(scalars)
    out = np.full(4 * 2 * (n + 2), 0xA5, dtype=np.uint64)
    f = plib.lib.rng_open_pk

    def call(k=1, mode=1, pk=circuit["pk"], p=ptr(flat), x=ptr(pts), s=ptr(sc), o=ptr(out),
             c=ctx.h):
        return f(c, ctypes.c_void_p(pk) if pk else None, k, p, x, s, mode, o)

    for kw in (dict(k=0), dict(k=129), dict(mode=3), dict(mode=-1), dict(pk=None),
               dict(p=None), dict(x=None), dict(s=None), dict(o=None), dict(c=None)):
        assert call(**kw) == RNG_ERR_BAD_ARG, kw
    assert (out == 0xA5).all()


# ------------------------------------------------------ prover paths agree

TRACE_LINE = "[open_dev] n=%d k=%d device stage"
_children = {}


def run_child(tmp_path, **switches):
    """Proofs and hints of child_main (tests/test_perm_product.py: rng_prove
    on the test circuit, rng_prove and rng_prove_cohort k = 3 on the
    settlement circuit, with link hints) under the given RNG_* switches, and
    the child's stderr.  One child per distinct setting in a session."""
    key = tuple(sorted(switches.items()))
    if key not in _children:
        outfile = tmp_path / ("_".join(f"{k}{v}" for k, v in key) + ".npz")
        env = dict(os.environ, RNG_COHORT_TRACE="1")
        for name in ("RNG_OPEN_DEVICE", "RNG_Z_DEVICE", "RNG_R1_LAGRANGE"):
            env.pop(name, None)
        env.update(switches)
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(outfile)],
                           cwd=str(REPO), env=env, timeout=300, capture_output=True, text=True)
        # a failed child ends the test here: the next one is not started
        assert r.returncode == 0, f"{switches} child rc={r.returncode}\n{r.stderr[-2000:]}"
        _children[key] = (dict(np.load(outfile)), r.stderr)
    return _children[key]


def assert_same_outputs(a, b, what):
    assert sorted(a) == sorted(b) and len(a) == 6
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{key} differs: {what}"
        assert a[key].any()


def test_prover_paths_agree(plib, tmp_path):
    """RNG_OPEN_DEVICE=0 (host rounds) and =1 (device stage) give the same
    proofs and link hints from both provers, the device stage announces
    itself once per proving call and only when on, and the settlement proof
    is the committed fixture."""
    host, host_err = run_child(tmp_path, RNG_OPEN_DEVICE="0")
    dev, dev_err = run_child(tmp_path, RNG_OPEN_DEVICE="1")
    assert_same_outputs(host, dev, "RNG_OPEN_DEVICE 0 vs 1")
    assert "[open_dev]" not in host_err
    lines = [ln for ln in dev_err.splitlines() if ln.startswith("[open_dev]")]
    n_test = next(int(ln.split("n=")[1].split()[0]) for ln in lines)
    assert lines == [TRACE_LINE % (n_test, 1), TRACE_LINE % (4096, 1), TRACE_LINE % (4096, 3)]
    assert n_test != 4096
    # circuit seed 42, blinder seed 7: the fixture of tests/test_golden.py
    gold = np.load(GOLD / "settlement_proof_cseed42_bseed7.npy")
    assert np.array_equal(dev["settlement_proof"], gold)
    assert np.array_equal(dev["cohort_proofs"][2 * 157:], gold)


@pytest.mark.parametrize("other", ["0", "1"])
def test_prover_paths_with_other_stages(plib, tmp_path, other):
    """The device stage reuses buffers that the device grand product and the
    Lagrange commit also touch: both off and both on under RNG_OPEN_DEVICE=1
    against the host rounds."""
    host, _ = run_child(tmp_path, RNG_OPEN_DEVICE="0")
    dev, err = run_child(tmp_path, RNG_OPEN_DEVICE="1", RNG_Z_DEVICE=other,
                         RNG_R1_LAGRANGE=other)
    assert_same_outputs(host, dev, f"RNG_Z_DEVICE = RNG_R1_LAGRANGE = {other}")
    assert err.count("[open_dev]") == 3


if __name__ == "__main__":
    child_main(sys.argv[1])
