"""Direct-lookup fixed-base MSM over the SRS (k_msm_lookup_table /
k_msm_lookup_sum) vs the CPU oracle, bit-exact.

Everything runs through rng_msm_srs_batch with mode 3, i.e. the same
msm_srs_run call the prover's commitments make.  The expected value is
always orc.msm over the first n SRS records, once per polynomial.

The context has 258 SRS points (power 8), so the tables are small (67 MB at
c = 8, 220 MB at c = 10) and n = 255..258 sits around one block of 256 lanes
and at the SRS end.  At these sizes the host picks one scalar per lane; a
child process with RNG_MSM_LOOKUP_L=4 runs the several-scalars-per-lane loop,
and another with RNG_MSM_LOOKUP_MAX_MB=1 the budget fallback.
"""
import ctypes
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(REPO))

from tests import py_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# every window size the selector (msm_lookup_select, prover_api.hip) can return
LOOKUP_CS = (8, 9, 10)
AUTO, FIXED, WINDOWED, LOOKUP = 0, 1, 2, 3
N_SRS = 258
SEED = 42
IDENTITY = np.array([0] * 8 + [1], dtype=np.uint64)
U64P = ctypes.POINTER(ctypes.c_uint64)


def make_ctx(plib, orc):
    ptau = orc.srs_generate_ptau(8, seed=SEED)
    g1, _, _ = orc.srs_parse(ptau, N_SRS - 1)
    assert g1.shape[0] == N_SRS
    return plib.init(ptau, N_SRS - 1), g1


@pytest.fixture(scope="module")
def plib():
    from renegade_amd import load_prover
    lib = load_prover()
    if not lib.gpu_available:
        pytest.skip("no GPU visible")
    return lib


@pytest.fixture(scope="module")
def ctx_g1(plib, orc):
    c, g1 = make_ctx(plib, orc)
    yield c, g1
    c.close()


def pack(polys, n):
    """list of B lists of n ints -> flat canonical u64 array (B*n*4)."""
    out = np.zeros((len(polys), n, 4), dtype=np.uint64)
    for b, poly in enumerate(polys):
        assert len(poly) == n
        for i, s in enumerate(poly):
            assert 0 <= s < ref.R
            if s:
                out[b, i] = ref.int_to_limbs(s)
    return out.reshape(-1)


def oracle(orc, g1, flat, n, B):
    b9 = np.ascontiguousarray(g1[:n]).reshape(-1)
    per = flat.reshape(B, 4 * n)
    return np.stack([orc.msm(b9, np.ascontiguousarray(per[b]), n, window_c=8)
                     for b in range(B)])


def rand_poly(rng, n):
    return [rng.randrange(ref.R) for _ in range(n)]


def tau(orc):
    t = np.zeros(4, dtype=np.uint64)
    orc.lib.orc_derive_tau.argtypes = [ctypes.c_uint64, U64P]
    orc.lib.orc_derive_tau(SEED, t.ctypes.data_as(U64P))
    return sum(int(t[k]) << (64 * k) for k in range(4))


def sized_batch(n, B):
    rng = random.Random(9000 + 31 * n + B)
    polys = [rand_poly(rng, n) for _ in range(B)]
    if B >= 5:
        polys[1] = [0] * n                  # all-zero polynomial -> identity record
        keep = n // 2                       # zero tail
        polys[3] = polys[3][:keep] + [0] * (n - keep)
    return pack(polys, n)


@pytest.mark.parametrize("B", [1, 5, 17])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 258])
def test_sizes_and_batching(ctx_g1, orc, n, B):
    ctx, g1 = ctx_g1
    flat = sized_batch(n, B)
    expect = oracle(orc, g1, flat, n, B)
    if B >= 5:
        assert np.array_equal(expect[1], IDENTITY)
    for c in LOOKUP_CS:
        got = ctx.msm_srs_batch(flat, n, B, window_c=c, mode=LOOKUP)
        assert np.array_equal(got, expect), f"c={c} n={n} B={B}"


def edge_scalars(c):
    half = 1 << (c - 1)
    full_digits = (1 << (c * (253 // c))) - 1   # every digit 2^c - 1: the carry ripples
    special = [half,                            # digit == 2^(c-1): positive, no carry
               half + 1,                        # negative with carry
               (half << c) | half, ((half + 1) << (2 * c)) | (half + 1),
               full_digits, (1 << 253) - 1,     # all ones
               ref.R - 1, ref.R - 2,            # top window
               1, 1 << (c * (253 // c)), 0]
    assert all(0 <= s < ref.R for s in special)
    return special


def edge_batch(c, n=64):
    rng = random.Random(1900 + c)
    special = edge_scalars(c)
    polys = [special + [0] * (n - len(special))]   # the edges alone
    poly = rand_poly(rng, n)                        # and among random filler
    for p, s in zip(rng.sample(range(n), len(special)), special):
        poly[p] = s
    polys.append(poly)
    return pack(polys, n), n


@pytest.mark.parametrize("c", LOOKUP_CS)
def test_digit_edges(ctx_g1, orc, c):
    ctx, g1 = ctx_g1
    flat, n = edge_batch(c)
    got = ctx.msm_srs_batch(flat, n, 2, window_c=c, mode=LOOKUP)
    assert np.array_equal(got, oracle(orc, g1, flat, n, 2))


def equal_opposite_batch(t):
    """P_i = tau^i G: (tau, 1) over (P_0, P_1) adds P_1 to itself, (r - tau, 1)
    adds P_1 to its negative; the same pairs at indices 0 and 256 of a 258-long
    polynomial use P_256 = tau^256 G.  -> (n, flat, B) per layout."""
    t256 = pow(t, 256, ref.R)
    short = [[t, 1], [ref.R - t, 1]]
    long_ = []
    for s0 in (t256, ref.R - t256):
        poly = [0] * N_SRS
        poly[0], poly[256] = s0, 1
        long_.append(poly)
    return [(2, pack(short, 2), 2), (N_SRS, pack(long_, N_SRS), 2)]


def check_equal_opposite(orc, g1, t, results):
    """results: per layout the (2, 9) records; expected 2*tau^k*G and identity"""
    g = np.ascontiguousarray(g1[:1]).reshape(-1)
    for (n, flat, B), got, k in zip(equal_opposite_batch(t), results, (1, 256)):
        expect = oracle(orc, g1, flat, n, B)
        twice = np.array(ref.int_to_limbs(2 * pow(t, k, ref.R) % ref.R), dtype=np.uint64)
        assert np.array_equal(expect[0], orc.msm(g, twice, 1, window_c=8))
        assert np.array_equal(expect[1], IDENTITY)
        assert np.array_equal(got, expect), f"n={n}"


@pytest.mark.parametrize("c", LOOKUP_CS)
def test_equal_and_opposite_operands(ctx_g1, orc, c):
    ctx, g1 = ctx_g1
    t = tau(orc)
    results = [ctx.msm_srs_batch(flat, n, B, window_c=c, mode=LOOKUP)
               for n, flat, B in equal_opposite_batch(t)]
    check_equal_opposite(orc, g1, t, results)


def test_path_switching(ctx_g1, orc):
    """lookup and bucket calls, c = 8 and c = 10, alternating on one thread"""
    ctx, g1 = ctx_g1
    n, B = 257, 5
    flat = sized_batch(n, B)
    expect = oracle(orc, g1, flat, n, B)
    for c, mode in [(8, LOOKUP), (8, FIXED), (10, LOOKUP), (10, FIXED), (8, LOOKUP),
                    (10, FIXED), (10, LOOKUP), (8, FIXED), (0, AUTO), (0, LOOKUP)]:
        got = ctx.msm_srs_batch(flat, n, B, window_c=c, mode=mode)
        assert np.array_equal(got, expect), f"c={c} mode={mode}"


# ---- child processes: the RNG_MSM_LOOKUP_* variables are read once ----

def child_main(what, outfile):
    from renegade_amd import load_prover
    from renegade_amd.prover import ProverError
    from tests.orc_bindings import OracleLib
    orc = OracleLib(str(REPO / "oracle" / "liborc.so"))
    plib = load_prover()
    plib.require_gpu()
    ctx, _ = make_ctx(plib, orc)
    out = {}
    n, B = 258, 5
    flat = sized_batch(n, B)
    if what == "budget":
        out["auto"] = ctx.msm_srs_batch(flat, n, B, mode=AUTO)
        for c in (0, 8):
            try:
                ctx.msm_srs_batch(flat, n, B, window_c=c, mode=LOOKUP)
                out[f"lookup_rc_{c}"] = np.array([0])
            except ProverError as e:
                out[f"lookup_rc_{c}"] = np.array([-2 if "rc=-2" in str(e) else -99])
    else:  # "lanes": several scalars per lane
        t = tau(orc)
        for c in (8, 10):
            out[f"sized_{c}"] = ctx.msm_srs_batch(flat, n, B, window_c=c, mode=LOOKUP)
            for k, (nn, fl, bb) in enumerate(equal_opposite_batch(t)):
                out[f"eqop_{c}_{k}"] = ctx.msm_srs_batch(fl, nn, bb, window_c=c, mode=LOOKUP)
    ctx.close()
    np.savez(outfile, **out)


def run_child(what, tmp_path, **env_add):
    outfile = tmp_path / f"{what}.npz"
    env = dict(os.environ, RNG_MSM_DEBUG="1", **env_add)
    for name in ("RNG_MSM_C", "RNG_MSM_LOOKUP", "RNG_MSM_LOOKUP_C", "RNG_MSM_FIXED"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), what, str(outfile)],
                       cwd=str(REPO), env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, f"{what} child rc={r.returncode}\n{r.stderr[-2000:]}"
    return np.load(outfile), r.stderr


def test_budget_fallback(ctx_g1, orc, tmp_path):
    """With a 1 MB budget no table fits: auto mode takes the bucket pipeline
    (the oracle's result, no lookup line), mode 3 is RNG_ERR_BAD_ARG."""
    _, g1 = ctx_g1
    env_add = {"RNG_MSM_LOOKUP_MAX_MB": "1"}
    res, stderr = run_child("budget", tmp_path, **env_add)
    n, B = 258, 5
    assert np.array_equal(res["auto"], oracle(orc, g1, sized_batch(n, B), n, B))
    msm_lines = [ln for ln in stderr.splitlines() if ln.startswith("[msm]")]
    assert msm_lines and not any("lookup" in ln for ln in msm_lines), stderr[-2000:]
    assert res["lookup_rc_0"][0] == -2 and res["lookup_rc_8"][0] == -2


def test_several_scalars_per_lane(ctx_g1, orc, tmp_path):
    """RNG_MSM_LOOKUP_L=4: one block per polynomial, lane t takes scalars t
    and t + 256, so the terms at indices 0 and 256 meet inside one lane."""
    _, g1 = ctx_g1
    res, stderr = run_child("lanes", tmp_path, RNG_MSM_LOOKUP_L="4")
    n, B = 258, 5
    expect = oracle(orc, g1, sized_batch(n, B), n, B)
    t = tau(orc)
    for c in (8, 10):
        assert f"lookup c={c} L=4 blocks=1" in stderr, stderr[-2000:]
        assert np.array_equal(res[f"sized_{c}"], expect)
        check_equal_opposite(orc, g1, t, [res[f"eqop_{c}_0"], res[f"eqop_{c}_1"]])


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
