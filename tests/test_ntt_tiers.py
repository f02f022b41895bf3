"""GPU NTT parity at every dispatch tier, direction and entry point.

`get_plan` / `ntt_dev_run` (renegade_amd/csrc/prover_api.hip) pick a code path
from log2 n:

  1..10   k_ntt_small, one workgroup (1024: the 512-thread load loop runs twice)
  11      two-pass, the only size with split_log = 5 (TA table degenerates)
  12..20  two-pass, k_ntt_col<2> + k_ntt_row<2>; odd sizes have N1 = 2*N2
  21      k_ntt_col<2> at exactly the 64 KiB pair cap + k_ntt_row<1>
  22      k_ntt_col<1> + k_ntt_row<1>, 64 KiB of LDS each
  23, 24  k_ntt_row<1> with N1 = 4096: 128 KiB of dynamic LDS (at 24 the
          column pass too); 2^24 is the documented upper bound

Every comparison here is exact equality of uint64 limbs.

Reference.  Up to 2^20 it is `orc.ntt`, the oracle's serial radix-2 loop.
Above that the loop is too slow, so the big tiers are checked against the
definition out[k] = sum_j in[j] * w^(jk) (inverse: w^-1 and a factor n^-1) in
two complementary ways, which TOGETHER are the reference for 2^21..2^24:

  * closed-form probes (constant, alternating, delta) compare all n outputs.
    A delta at input j must give out[k] = c * (w^j)^k, one `fr_geom_table`
    call: that checks every output slot is written, in the right place, with
    the right twiddle product.  But a delta exercises ONE input slot; a kernel
    that reads some other input slot from the wrong address still passes.
  * dense random input checked at 16 chosen outputs with `fr_poly_eval`
    (Horner).  Each checked output depends on every input slot being read
    and weighted correctly.  But it looks at 16 outputs; a kernel that
    misplaces others still passes.

Neither alone pins the transform; a wrong kernel has to fool both.  The two
helpers are themselves pinned against Python bignums in test_oracle_core.py,
and at 2^10, 2^11 and 2^12 the probes here are cross-checked against
`orc.ntt` in the same test.

Random data is drawn with limbs below 2^61, so values are below 2^253 < r, and
every residue below r is a valid Montgomery element.
"""
import ctypes

import numpy as np
import pytest

from tests import py_ref as ref

pytestmark = pytest.mark.gpu

R = ref.R
RNG_ERR_BAD_ARG = -2
NTT_SMALL_MAX = 1024
U64P = ctypes.POINTER(ctypes.c_uint64)
DIRS = pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])


@pytest.fixture(scope="module")
def plib():
    from renegade_amd import load_prover
    lib = load_prover()
    if not lib.gpu_available:
        pytest.skip("no GPU visible")
    return lib


@pytest.fixture(scope="module")
def ptau10(orc):
    return orc.srs_generate_ptau(10, seed=42)


@pytest.fixture(scope="module")
def ctx(plib, ptau10):
    c = plib.init(ptau10, (1 << 10) + 2)
    yield c
    c.close()


# ---------------------------------------------------------------- helpers

def rand_fr(count, seed):
    return np.random.default_rng(seed).integers(0, 1 << 61, size=4 * count, dtype=np.uint64)


def rand_fr_int(seed):
    return ref.limbs_to_int(rand_fr(1, seed))


def limbs(v):
    return np.array(ref.int_to_limbs(v), dtype=np.uint64)


def split(logn):
    """(N1, N2) as get_plan chooses them."""
    log_n2 = logn // 2
    return 1 << (logn - log_n2), 1 << log_n2


def root(n, inverse):
    w = ref.fr_root_of_unity(n)
    return pow(w, -1, R) if inverse else w


def out_scale(n, inverse):
    """Canonical factor on every output: 1 forward, n^-1 inverse.  Montgomery
    form is linear, so it applies to Montgomery residues as plain integers."""
    return pow(n, -1, R) if inverse else 1


def orc_ntt(orc, data, n, inverse, batch=1):
    out = data.copy()
    for b in range(batch):
        orc.ntt(out[4 * n * b:4 * n * (b + 1)], n, inverse=inverse)
    return out


def one_hot(n, k, value):
    """n Montgomery elements, all zero except element k = value (an int)."""
    a = np.zeros(4 * n, dtype=np.uint64)
    a[4 * k:4 * k + 4] = limbs(value)
    return a


def delta_expect(orc, n, j, c, inverse):
    """Transform of c * delta_j: out[k] = c * (w^j)^k (inverse: w^-1, n^-1)."""
    base = ref.to_mont(pow(root(n, inverse), j, R), R)
    return orc.fr_geom_table(c * out_scale(n, inverse) % R, base, n)


# ------------------------------------------------- 1. sweep against orc.ntt

@DIRS
@pytest.mark.parametrize("logn", range(1, 21))
def test_sweep_vs_oracle(ctx, orc, logn, inverse):
    n = 1 << logn
    data = rand_fr(n, 7000 + 2 * logn + inverse)
    expect = orc_ntt(orc, data, n, inverse)
    ctx.ntt(data, n, inverse=inverse)
    assert np.array_equal(data, expect)


# ------------------------------------------ 2. closed-form full-array probes

PROBE_LOGN = [10, 11, 12, 21, 22, 23, 24]
PROBES = ["const_rm1", "const_zero", "alt_rm1",
          "delta_1", "delta_N1", "delta_last", "delta_rand"]


@DIRS
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("logn", PROBE_LOGN)
def test_closed_form_probe(ctx, orc, logn, probe, inverse):
    n = 1 << logn
    n1, _ = split(logn)
    scale = out_scale(n, inverse)
    if probe.startswith("const"):
        # in[j] = c  ->  out[0] = n*c, zero elsewhere
        c = R - 1 if probe == "const_rm1" else 0
        data = np.tile(limbs(c), n)
        expect = one_hot(n, 0, n * c * scale % R)
    elif probe == "alt_rm1":
        # in[j] = c*(-1)^j  ->  out[n/2] = n*c, zero elsewhere (w^(n/2) = -1
        # in both directions)
        c = R - 1
        data = np.tile(np.concatenate([limbs(c), limbs((R - c) % R)]), n // 2)
        expect = one_hot(n, n // 2, n * c * scale % R)
    else:
        seed = 8000 + 2 * logn + inverse
        j = {"delta_1": 1, "delta_N1": n1, "delta_last": n - 1,
             "delta_rand": int(np.random.default_rng(seed).integers(0, n))}[probe]
        c = rand_fr_int(seed + 100)
        data = one_hot(n, j, c)
        expect = delta_expect(orc, n, j, c, inverse)
    if logn <= 20:
        # the probe's own expectation, cross-checked against the oracle NTT
        assert np.array_equal(orc_ntt(orc, data, n, inverse), expect)
    ctx.ntt(data, n, inverse=inverse)
    assert np.array_equal(data, expect)


# -------------------------------- 3. dense random input at chosen outputs

@DIRS
@pytest.mark.parametrize("logn", PROBE_LOGN)
def test_dense_at_chosen_outputs(ctx, orc, logn, inverse):
    n = 1 << logn
    _, n2 = split(logn)
    seed = 9000 + 2 * logn + inverse
    ks = [0, 1, n // 2, n - 1, n2 - 1, n2, n2 + 1, n - n2]
    ks += [int(k) for k in np.random.default_rng(seed).integers(0, n, size=8)]
    src = rand_fr(n, seed + 100)
    w = root(n, inverse)
    points = np.concatenate([limbs(ref.to_mont(pow(w, k, R), R)) for k in ks])
    evals = orc.fr_poly_eval(src, n, points)
    scale = out_scale(n, inverse)
    expect = [ref.limbs_to_int(evals[4 * i:4 * i + 4]) * scale % R for i in range(len(ks))]
    data = src.copy()
    ctx.ntt(data, n, inverse=inverse)
    got = [ref.limbs_to_int(data[4 * k:4 * k + 4]) for k in ks]
    assert got == expect
    if logn <= 20:
        assert np.array_equal(data, orc_ntt(orc, src, n, inverse))


# ------------------------------------------------------------ 4. batching

# (4, 10: k_ntt_small's blockIdx.x * n; 11, 13: the two-pass kernels' batch
# offset in inverse direction, with split_log = 5 and with N1 = 2*N2)
@pytest.mark.parametrize("logn,batch,inverse", [
    (4, 5, False), (4, 5, True), (10, 5, False), (10, 5, True),
    (11, 3, True), (13, 3, True)])
def test_batch_vs_oracle(ctx, orc, logn, batch, inverse):
    n = 1 << logn
    data = rand_fr(n * batch, 10000 + 2 * logn + inverse)
    expect = orc_ntt(orc, data, n, inverse, batch)
    ctx.ntt(data, n, batch=batch, inverse=inverse)
    assert np.array_equal(data, expect)


@DIRS
def test_batch_2_22_closed_form(ctx, orc, inverse):
    """Batch 2 through k_ntt_col<1> / k_ntt_row<1>: transform 0 is a delta,
    transform 1 a constant.  A wrong blockIdx.x / N1 offset mixes the two."""
    logn = 22
    n = 1 << logn
    j = int(np.random.default_rng(11000 + inverse).integers(0, n))
    c0, c1 = rand_fr_int(11002 + inverse), rand_fr_int(11004 + inverse)
    data = np.concatenate([one_hot(n, j, c0), np.tile(limbs(c1), n)])
    expect = np.concatenate([delta_expect(orc, n, j, c0, inverse),
                             one_hot(n, 0, n * c1 * out_scale(n, inverse) % R)])
    ctx.ntt(data, n, batch=2, inverse=inverse)
    assert np.array_equal(data[:4 * n], expect[:4 * n])
    assert np.array_equal(data[4 * n:], expect[4 * n:])


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_scratch_regrowth(plib, ptau10, orc, entry):
    """Batch 1, then 4, then 1 on a fresh context at 2^13: get_plan allocates
    the plan's scratch, regrows it, then reuses the larger one."""
    n = 1 << 13
    c = plib.init(ptau10, (1 << 10) + 2)
    try:
        for step, batch in enumerate([1, 4, 1]):
            data = rand_fr(n * batch, 12000 + step)
            expect = orc_ntt(orc, data, n, False, batch)
            if entry == "host":
                c.ntt(data, n, batch=batch)
            else:
                d = c.dbuf_from(data)
                try:
                    c.ntt_dev(d, n, batch=batch)
                    c.dbuf_download(d, data)
                finally:
                    c.dbuf_free(d)
            assert np.array_equal(data, expect), f"step {step} batch {batch}"
    finally:
        c.close()


# ------------------------------------------------- 5. device entry points

@DIRS
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("logn", [6, 11, 14])
@pytest.mark.parametrize("entry", ["dev", "oop"])
def test_device_entry_points(ctx, orc, entry, logn, batch, inverse):
    n = 1 << logn
    data = rand_fr(n * batch, 13000 + 4 * logn + 2 * batch + inverse)
    expect = orc_ntt(orc, data, n, inverse, batch)
    got = np.zeros_like(data)
    bufs = []
    try:
        bufs.append(ctx.dbuf_from(data))
        if entry == "dev":
            ctx.ntt_dev(bufs[0], n, batch=batch, inverse=inverse)
            ctx.dbuf_download(bufs[0], got)
        else:
            bufs.append(ctx.dbuf_alloc(data.nbytes))
            ctx.ntt_dev_oop(bufs[0], bufs[1], n, batch=batch, inverse=inverse)
            ctx.dbuf_download(bufs[1], got)
    finally:
        for d in bufs:
            ctx.dbuf_free(d)
    assert np.array_equal(got, expect)


def test_oop_ping_pong(ctx, orc):
    """A -> B forward, then B -> A inverse, as the benchmark does it."""
    n = 1 << 14
    data = rand_fr(n, 14000)
    mid, back = np.zeros_like(data), np.zeros_like(data)
    bufs = []
    try:
        bufs.append(ctx.dbuf_from(data))
        bufs.append(ctx.dbuf_alloc(data.nbytes))
        ctx.ntt_dev_oop(bufs[0], bufs[1], n)
        ctx.dbuf_download(bufs[1], mid)
        ctx.ntt_dev_oop(bufs[1], bufs[0], n, inverse=True)
        ctx.dbuf_download(bufs[0], back)
    finally:
        for d in bufs:
            ctx.dbuf_free(d)
    assert np.array_equal(mid, orc_ntt(orc, data, n, False))
    assert np.array_equal(back, data)


# ------------------------------------------------------ 6. argument contract

def _call(ctx, entry, host, d_in, d_out, n, batch):
    """Raw return code of one entry point (no exception on failure)."""
    lib = ctx.lib
    if entry == "host":
        return lib.rng_ntt_fr(ctx.h, host.ctypes.data_as(U64P), n, batch, 0)
    if entry == "dev":
        return lib.rng_ntt_fr_dev(ctx.h, d_in, n, batch, 0)
    return lib.rng_ntt_fr_dev_oop(ctx.h, d_in, d_out, n, batch, 0)


@pytest.mark.parametrize("n", [0, 1, 3, 1 << 25, 1 << 26])
@pytest.mark.parametrize("entry", ["host", "dev", "oop"])
def test_bad_n_rejected(ctx, entry, n):
    # host: a full-size zero buffer whose pages are never touched when the
    # call is rejected up front, so no version of the library reads past it;
    # device: a small real buffer, because rejection must precede any access
    host = np.zeros(4 * max(n, 4), dtype=np.uint64) if entry == "host" else None
    bufs = []
    try:
        if entry != "host":
            bufs = [ctx.dbuf_alloc(64 * 32), ctx.dbuf_alloc(64 * 32)]
        d_in, d_out = bufs if bufs else (None, None)
        assert _call(ctx, entry, host, d_in, d_out, n, 1) == RNG_ERR_BAD_ARG
    finally:
        for d in bufs:
            ctx.dbuf_free(d)


@pytest.mark.parametrize("n", [64, 2048])
@pytest.mark.parametrize("entry", ["host", "dev", "oop"])
def test_batch_zero_rejected(ctx, entry, n):
    host = rand_fr(n, 15000)
    keep = host.copy()
    bufs = []
    try:
        bufs = [ctx.dbuf_from(host), ctx.dbuf_alloc(host.nbytes)]
        assert _call(ctx, entry, host, bufs[0], bufs[1], n, 0) == RNG_ERR_BAD_ARG
        got = np.zeros_like(host)
        ctx.dbuf_download(bufs[0], got)
    finally:
        for d in bufs:
            ctx.dbuf_free(d)
    assert np.array_equal(host, keep) and np.array_equal(got, keep)


@pytest.mark.parametrize("logn", [11, 14])
def test_oop_alias_rejected_above_small(ctx, logn):
    n = 1 << logn
    data = rand_fr(n, 16000 + logn)
    got = np.zeros_like(data)
    d = ctx.dbuf_from(data)
    try:
        assert _call(ctx, "oop", None, d, d, n, 1) == RNG_ERR_BAD_ARG
        ctx.dbuf_download(d, got)
    finally:
        ctx.dbuf_free(d)
    assert np.array_equal(got, data)  # rejected before any access


@DIRS
@pytest.mark.parametrize("logn", [1, 10])
def test_oop_alias_allowed_on_small_path(ctx, orc, logn, inverse):
    n = 1 << logn
    assert n <= NTT_SMALL_MAX
    data = rand_fr(n, 17000 + 2 * logn + inverse)
    got = np.zeros_like(data)
    d = ctx.dbuf_from(data)
    try:
        ctx.ntt_dev_oop(d, d, n, inverse=inverse)
        ctx.dbuf_download(d, got)
    finally:
        ctx.dbuf_free(d)
    assert np.array_equal(got, orc_ntt(orc, data, n, inverse))
