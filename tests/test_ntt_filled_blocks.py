"""GPU NTT parity for the filled-block passes (k_ntt_col_fill / k_ntt_row_fill).

For 2^11 <= n <= 2^17 `ntt_dev_run` (renegade_amd/csrc/prover_api.hip) runs a
pass whose DFT length N is at most 256 in 256-thread blocks that take
PW = 512 / N columns (rows) each:

  log2 n   N1, N2     column PW   row PW
  11       64, 32     16          8
  12       64, 64     8           8
  13       128, 64    8           4
  14       128, 128   4           4
  15       256, 128   4           2
  16       256, 256   2           2
  17       512, 256   2           k_ntt_row<2>, as before
  18       512, 512   k_ntt_col<2> + k_ntt_row<2>, as before

A block finds its transform as blockIdx.x / (N / PW), so a wrong split shows
only with more than one transform in the batch: every case here is batched,
and each transform of a batch is compared on its own.

Every comparison is exact equality of uint64 limbs against `orc.ntt`, the
oracle's serial radix-2 loop.  Random data is drawn as in test_ntt_tiers.py
(limbs below 2^61, so values are below r).

RNG_NTT_FILL is read once per process, so the switch is tested in two fresh
child processes (this file run as a script).
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(REPO))

from tests import py_ref as ref  # noqa: E402
from tests.test_ntt_tiers import (delta_expect, limbs, one_hot, orc_ntt,  # noqa: E402
                                  out_scale, rand_fr, rand_fr_int)

pytestmark = pytest.mark.gpu

R = ref.R
DIRS = pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
SWITCH_SHAPES = [(12, 2), (15, 2)]  # (log2 n, batch) of the switch test


@pytest.fixture(scope="module")
def plib():
    from renegade_amd import load_prover
    lib = load_prover()
    if not lib.gpu_available:
        pytest.skip("no GPU visible")
    return lib


@pytest.fixture(scope="module")
def ctx(plib, orc):
    c = plib.init(orc.srs_generate_ptau(10, seed=42), (1 << 10) + 2)
    yield c
    c.close()


def assert_each_transform(got, expect, n, batch):
    for b in range(batch):
        lo, hi = 4 * n * b, 4 * n * (b + 1)
        assert np.array_equal(got[lo:hi], expect[lo:hi]), f"transform {b} of {batch}"


# ------------------------- 1. every (PW, N) pair and both boundaries, batch 3

@DIRS
@pytest.mark.parametrize("logn", range(11, 19))
def test_batch3_vs_oracle(ctx, orc, logn, inverse):
    n, batch = 1 << logn, 3
    data = rand_fr(n * batch, 21000 + 2 * logn + inverse)
    expect = orc_ntt(orc, data, n, inverse, batch)
    ctx.ntt(data, n, batch=batch, inverse=inverse)
    assert_each_transform(data, expect, n, batch)


# ------------- 2. distinguishable transforms in one batch, headline sizes

@DIRS
@pytest.mark.parametrize("logn", [12, 15])
def test_distinguishable_batch(ctx, orc, logn, inverse):
    """Transform 0 a delta at a random index, 1 a constant, 2 dense random,
    through the out-of-place device entry point the provers use."""
    n = 1 << logn
    seed = 22000 + 2 * logn + inverse
    j = int(np.random.default_rng(seed).integers(0, n))
    c0, c1 = rand_fr_int(seed + 100), rand_fr_int(seed + 200)
    data = np.concatenate([one_hot(n, j, c0), np.tile(limbs(c1), n),
                           rand_fr(n, seed + 300)])
    closed = [delta_expect(orc, n, j, c0, inverse),
              one_hot(n, 0, n * c1 * out_scale(n, inverse) % R)]
    expect = orc_ntt(orc, data, n, inverse, 3)
    got = np.zeros_like(data)
    bufs = []
    try:
        bufs.append(ctx.dbuf_from(data))
        bufs.append(ctx.dbuf_alloc(data.nbytes))
        ctx.ntt_dev_oop(bufs[0], bufs[1], n, batch=3, inverse=inverse)
        ctx.dbuf_download(bufs[1], got)
    finally:
        for d in bufs:
            ctx.dbuf_free(d)
    assert np.array_equal(got[:4 * n], closed[0]), "delta vs closed form"
    assert np.array_equal(got[4 * n:8 * n], closed[1]), "constant vs closed form"
    assert_each_transform(got, expect, n, 3)


# ------------------------------------------------------------ 3. the switch

def switch_input(logn, batch, inverse):
    return rand_fr((1 << logn) * batch, 23000 + 2 * logn + inverse)


def child_main(outfile):
    """Transform the switch inputs under the inherited RNG_NTT_FILL and save
    the outputs."""
    from renegade_amd import load_prover
    from tests.orc_bindings import OracleLib
    plib = load_prover()
    plib.require_gpu()
    orc = OracleLib(str(REPO / "oracle" / "liborc.so"))
    ctx = plib.init(orc.srs_generate_ptau(10, seed=42), (1 << 10) + 2)
    out = {}
    for logn, batch in SWITCH_SHAPES:
        for inverse in (False, True):
            data = switch_input(logn, batch, inverse)
            ctx.ntt(data, 1 << logn, batch=batch, inverse=inverse)
            out[f"n{logn}_{'inv' if inverse else 'fwd'}"] = data
    ctx.close()
    np.savez(outfile, **out)


def test_switch_both_settings(plib, orc, tmp_path):
    """RNG_NTT_FILL=0 (the 512-thread pair kernels) and =1 (filled blocks), one
    fresh process each: both give the oracle's transform."""
    expect = {}
    for logn, batch in SWITCH_SHAPES:
        for inverse in (False, True):
            expect[f"n{logn}_{'inv' if inverse else 'fwd'}"] = (
                orc_ntt(orc, switch_input(logn, batch, inverse), 1 << logn, inverse, batch),
                1 << logn, batch)
    for mode in ("0", "1"):
        outfile = tmp_path / f"fill{mode}.npz"
        env = dict(os.environ, RNG_NTT_FILL=mode)
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(outfile)],
                           cwd=str(REPO), env=env, timeout=120, capture_output=True,
                           text=True)
        # a failed child ends the test here: the second one is not started
        assert r.returncode == 0, (f"RNG_NTT_FILL={mode} child rc={r.returncode}\n"
                                   f"{r.stderr[-2000:]}")
        got = np.load(outfile)
        assert sorted(got.files) == sorted(expect)
        for key, (want, n, batch) in expect.items():
            for b in range(batch):
                lo, hi = 4 * n * b, 4 * n * (b + 1)
                assert np.array_equal(got[key][lo:hi], want[lo:hi]), \
                    f"RNG_NTT_FILL={mode} {key} transform {b}"


if __name__ == "__main__":
    child_main(sys.argv[1])
