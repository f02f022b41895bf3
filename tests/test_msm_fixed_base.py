"""Fixed-base MSM over the SRS (precomputed window tables, one bucket set
per polynomial) vs the CPU oracle, bit-exact.

Everything runs through rng_msm_srs_batch, i.e. the same msm_dev_run call
the prover's commitments use.  The expected value is always orc.msm over the
first n SRS records, called once per polynomial.
"""
import random

import numpy as np
import pytest

from tests import py_ref as ref

pytestmark = pytest.mark.gpu

# every window size msm_fixed_c (msm_kernels.hip) can return
FIXED_CS = (8, 10, 13)
AUTO, FIXED, WINDOWED = 0, 1, 2
N_SRS = 1026


def n_windows(c):
    return (256 + c - 1) // c


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
    """orc.msm over the first n SRS records, once per polynomial."""
    b9 = np.ascontiguousarray(g1[:n]).reshape(-1)
    per = flat.reshape(B, 4 * n)
    return np.stack([orc.msm(b9, np.ascontiguousarray(per[b]), n, window_c=8)
                     for b in range(B)])


def rand_poly(rng, n):
    return [rng.randrange(ref.R) for _ in range(n)]


IDENTITY = np.array([0] * 8 + [1], dtype=np.uint64)


@pytest.mark.parametrize("c", FIXED_CS)
def test_table_rows(ctx, orc, srs10, c):
    """Poly j carries scalars d_i * 2^(c*j): all its digits sit in window j,
    so it reads table row j only — a wrong or missing row fails exactly its
    own j."""
    _, g1 = srs10
    W = n_windows(c)
    rng = random.Random(100 + c)
    polys = []
    for j in range(W):
        dmax = min(100, (ref.R - 1) >> (c * j))  # d < 2^(c-1): no carry out of j
        assert dmax >= 1
        polys.append([rng.randint(1, dmax) << (c * j) for _ in range(N_SRS)])
    flat = pack(polys, N_SRS)
    expect = oracle(orc, g1, flat, N_SRS, W)
    got = ctx.msm_srs_batch(flat, N_SRS, W, window_c=c, mode=FIXED)
    bad = [j for j in range(W) if not np.array_equal(got[j], expect[j])]
    assert not bad, f"c={c}: table rows {bad} differ from the oracle"


@pytest.mark.parametrize("B", [1, 5, 13])
@pytest.mark.parametrize("n", [1, 2, 255, 1026])
def test_sizes_and_batching(ctx, orc, srs10, n, B):
    _, g1 = srs10
    rng = random.Random(7000 + 31 * n + B)
    polys = [rand_poly(rng, n) for _ in range(B)]
    if B >= 5:
        polys[1] = [0] * n  # all-zero polynomial -> identity record
        keep = n // 2       # tail is zero padding (a shorter poly in the batch)
        polys[3] = polys[3][:keep] + [0] * (n - keep)
    flat = pack(polys, n)
    expect = oracle(orc, g1, flat, n, B)
    if B >= 5:
        assert np.array_equal(expect[1], IDENTITY)
    for mode in (FIXED, WINDOWED):
        got = ctx.msm_srs_batch(flat, n, B, mode=mode)
        assert np.array_equal(got, expect), f"mode {mode} n={n} B={B}"
        if B >= 5:
            assert got[1][8] == 1 and not got[1][:8].any()


@pytest.mark.parametrize("c", FIXED_CS)
def test_digit_edges(ctx, orc, srs10, c):
    _, g1 = srs10
    n = 64
    half = 1 << (c - 1)
    full_digits = (1 << (c * (253 // c))) - 1  # every digit 2^c-1: carry chain
    special = [0, 1, 2, ref.R - 1, ref.R - 2, (1 << 253) - 1, (1 << 128) - 1,
               half,             # digit == half: stays positive, no carry
               half + 1,         # negative digit with carry
               (1 << c) + half,
               full_digits]
    assert all(s < ref.R for s in special)
    rng = random.Random(900 + c)
    polys = []
    for b in range(2):
        poly = rand_poly(rng, n)
        pos = rng.sample(range(n), len(special))  # random filler around them
        for p, s in zip(pos, special):
            poly[p] = s
        polys.append(poly)
    flat = pack(polys, n)
    expect = oracle(orc, g1, flat, n, 2)
    got = ctx.msm_srs_batch(flat, n, 2, window_c=c, mode=FIXED)
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("c", FIXED_CS)
def test_long_segments(ctx, orc, srs10, c):
    """Equal scalars put 1026 entries per window into one bucket per digit
    value — far past the 128-entry sub-segment cap — so the split and
    k_msm_seg_merge run on the packed keys."""
    _, g1 = srs10
    rng = random.Random(4242 + c)
    one = rng.randrange(ref.R)
    four = [rng.randrange(ref.R) for _ in range(4)]
    polys = [[one] * N_SRS, [four[i % 4] for i in range(N_SRS)]]
    flat = pack(polys, N_SRS)
    expect = oracle(orc, g1, flat, N_SRS, 2)
    got = ctx.msm_srs_batch(flat, N_SRS, 2, window_c=c, mode=FIXED)
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("B", [7, 8])
@pytest.mark.parametrize("c", FIXED_CS)
def test_key_packing_group_boundary(ctx, orc, srs10, c, B):
    """B+1 a power of two (7) and B a power of two (8): both sides of the
    group-bit count and of the sentinel B << c.  The last polynomial holds
    magnitude-2^(c-1) digits, the largest real key below the sentinel."""
    _, g1 = srs10
    n = 96
    rng = random.Random(555 + 16 * c + B)
    polys = [rand_poly(rng, n) for _ in range(B)]
    half = 1 << (c - 1)
    polys[B - 1][0] = half
    polys[B - 1][n - 1] = half << c
    polys[0][5] = 0
    flat = pack(polys, n)
    expect = oracle(orc, g1, flat, n, B)
    got = ctx.msm_srs_batch(flat, n, B, window_c=c, mode=FIXED)
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("B", [3, 16])  # 16: the batch size from which auto picks c=10
def test_mode_auto_equals_fixed(ctx, orc, srs10, B):
    _, g1 = srs10
    n = 300
    rng = random.Random(31337 + B)
    flat = pack([rand_poly(rng, n) for _ in range(B)], n)
    fixed = ctx.msm_srs_batch(flat, n, B, mode=FIXED)
    auto = ctx.msm_srs_batch(flat, n, B, mode=AUTO)
    assert np.array_equal(auto, fixed)
    assert np.array_equal(fixed, oracle(orc, g1, flat, n, B))


def test_windowed_many_groups_grows_window_sums(ctx, orc, srs10):
    """Windowed mode at c=8, n=8, B=260: G = 260*32 = 8320 key groups,
    chunk 8, 16 chunks per window, one sub-block per window.  G*subb passes
    the 8192 entries window_sums starts with, so the scratch grows, and 16
    chunks per block is no multiple of 64, so k_msm_window_combine (not
    combine2) folds them.  A smaller call afterwards reuses the grown
    scratch."""
    _, g1 = srs10
    n, B, c = 8, 260, 8
    assert B * n_windows(c) > 8192
    rng = random.Random(8320)
    polys = [rand_poly(rng, n) for _ in range(B)]
    polys[1] = [0] * n
    polys[3] = polys[3][:n // 2] + [0] * (n - n // 2)
    flat = pack(polys, n)
    expect = oracle(orc, g1, flat, n, B)
    assert np.array_equal(expect[1], IDENTITY)
    got = ctx.msm_srs_batch(flat, n, B, window_c=c, mode=WINDOWED)
    bad = [b for b in range(B) if not np.array_equal(got[b], expect[b])]
    assert not bad, f"records {bad} differ from the oracle"
    small = ctx.msm_srs_batch(flat[:4 * n * 5], n, 5, window_c=c, mode=WINDOWED)
    assert np.array_equal(small, expect[:5])


def test_table_slots_exhausted(ctx, orc, srs10):
    """A context holds three window tables.  Once c = 8, 10 and 13 own them,
    a fourth window size gets none: fixed-base mode is an error, auto mode
    falls back to the windowed path."""
    from renegade_amd.prover import ProverError
    _, g1 = srs10
    rng = random.Random(909)
    tiny = pack([rand_poly(rng, 4)], 4)
    for c in FIXED_CS:
        got = ctx.msm_srs_batch(tiny, 4, 1, window_c=c, mode=FIXED)
        assert np.array_equal(got, oracle(orc, g1, tiny, 4, 1))
    n, B = 96, 3
    flat = pack([rand_poly(rng, n) for _ in range(B)], n)
    with pytest.raises(ProverError, match="rc=-2"):  # RNG_ERR_BAD_ARG
        ctx.msm_srs_batch(flat, n, B, window_c=9, mode=FIXED)
    got = ctx.msm_srs_batch(flat, n, B, window_c=9, mode=AUTO)
    assert np.array_equal(got, oracle(orc, g1, flat, n, B))
