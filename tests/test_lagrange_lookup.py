"""Round-1 commitments as a lookup sum over compacted digits
(k_msm_entry_lookup_sum over the Lagrange lookup table) vs the
CPU oracle, bit-exact.

Everything runs through rng_commit_lagrange, and the expected value is the
oracle's, computed as tests/test_lagrange_commit.py computes it (inverse NTT
of the evaluations, the blinding, orc.msm over the first n + 2 SRS records).
The SRS has power 10, so n <= 1024 and the tables stay small (269 MB at
c = 8, 874 MB at c = 10 for n = 1024).

The sum kernel takes a grid (S, B) of 256-lane blocks.  At these sizes the
host picks S = 1 or 2; child processes force S = 3 and S = 1 through
RNG_R1_LOOKUP_S (read once per process), and others switch the path off
(RNG_R1_LOOKUP=0, RNG_MSM_LOOKUP_MAX_MB=1) to keep the bucket pipeline over
compacted digits covered.  A commit on the new path leaves the sort, chunk
and combine slots of rng_msm_last_times at exactly zero, which is how the
in-process tests know which path ran; the children read the RNG_MSM_DEBUG
lines.
"""
import os
import random
import subprocess
import sys
import threading
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(REPO))

from tests import py_ref as ref  # noqa: E402
from tests.test_lagrange_commit import (IDENTITY, commit, expected,  # noqa: E402
                                        sparse_poly)

pytestmark = pytest.mark.gpu

R = ref.R
CS = (8, 10)
POWER = 10
NS = (2, 4, 64, 256, 1024)
BS = (1, 5, 13, 240)


@pytest.fixture(scope="module")
def plib():
    from renegade_amd import load_prover
    lib = load_prover()
    if not lib.gpu_available:
        pytest.skip("no GPU visible")
    return lib


@pytest.fixture(scope="module")
def srs10(orc):
    ptau = orc.srs_generate_ptau(POWER, seed=42)
    g1, _, _ = orc.srs_parse(ptau, (1 << POWER) + 2)
    return ptau, g1


@pytest.fixture(scope="module")
def ctx_c(plib, srs10):
    """one context per window size, as in test_lagrange_commit"""
    ptau, _ = srs10
    ctxs = {c: plib.init(ptau, (1 << POWER) + 2) for c in CS}
    yield ctxs
    for c in ctxs.values():
        c.close()


def took_entry_lookup(plib):
    """the calling thread's last MSM ran no sort, no window chunks, no combine"""
    t = plib.msm_last_times()
    return t["sort"] == 0 and t["window_chunks"] == 0 and t["final"] == 0


def pool(n):
    """240 settlement-like polys with blinders for domain n; the batches of
    every B are prefixes of it"""
    rng = random.Random(7100 + n)
    polys = [sparse_poly(rng, n) for _ in range(max(BS))]
    blinders = [(rng.randrange(R), rng.randrange(R)) for _ in range(max(BS))]
    return polys, blinders


_EXPECTED = {}  # (n, b) -> oracle record, shared by every B and c


def pool_expected(orc, g1, n, B):
    polys, blinders = pool(n)
    missing = [b for b in range(B) if (n, b) not in _EXPECTED]
    # the oracle calls release the GIL: a few threads cut the B = 240 pools
    with ThreadPoolExecutor(max_workers=8) as ex:
        recs = ex.map(lambda b: expected(orc, g1, polys[b], blinders[b], n), missing)
        for b, rec in zip(missing, recs):
            _EXPECTED[(n, b)] = rec
    return np.stack([_EXPECTED[(n, b)] for b in range(B)])


def same(got, exp, what):
    bad = [b for b in range(len(exp)) if not np.array_equal(got[b], exp[b])]
    assert not bad, f"{what}: records {bad} differ from the oracle"


# ------------------------------------------------ sizes and batches

@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("n", NS)
def test_sizes_and_batches(plib, ctx_c, orc, srs10, n, B, c):
    _, g1 = srs10
    polys, blinders = pool(n)
    exp = pool_expected(orc, g1, n, B)
    got = commit(ctx_c[c], polys[:B], blinders[:B], n, c)
    assert took_entry_lookup(plib)
    same(got, exp, f"n={n} B={B} c={c}")


# ------------------------------------------------ entry-range edges

def edge_polys(c, n):
    rng = random.Random(8200 + c)
    half = 1 << (c - 1)
    full_digits = (1 << (c * (253 // c))) - 1  # every digit 2^c - 1: carry chain
    special = [half,             # digit == half: stays positive, no carry
               half + 1,         # negative digit with carry
               (1 << c) + half, full_digits, R - 1, (1 << 253) - 1]
    edges = [0] * n
    for p, s in zip(rng.sample(range(n), len(special)), special):
        edges[p] = s
    single = [0] * n
    single[rng.randrange(n)] = rng.randrange(1, R)
    polys = [sparse_poly(rng, n),
             [0] * n,            # 1: all-zero poly between non-zero ones
             single,             # 2: exactly one non-zero value
             [0] * n,            # 3: blinders only
             [1] * n,
             sparse_poly(rng, n),
             [R - 1] * n,        # 6: dense, 32 digits per value, among sparse ones
             sparse_poly(rng, n),
             edges]
    blinders = [(0, 0)] * len(polys)
    blinders[3] = (rng.randrange(1, R), rng.randrange(1, R))
    blinders[7] = (rng.randrange(1, R), 0)
    return polys, blinders


@pytest.mark.parametrize("c", CS)
def test_all_zero_batch(plib, ctx_c, c):
    n = 64
    got = commit(ctx_c[c], [[0] * n] * 3, None, n, c)
    assert took_entry_lookup(plib)
    for b in range(3):
        assert np.array_equal(got[b], IDENTITY)


@pytest.mark.parametrize("c", CS)
def test_entry_range_edges(plib, ctx_c, orc, srs10, c):
    _, g1 = srs10
    n = 256
    polys, blinders = edge_polys(c, n)
    got = commit(ctx_c[c], polys, blinders, n, c)
    assert took_entry_lookup(plib)
    exp = np.stack([expected(orc, g1, p, b, n) for p, b in zip(polys, blinders)])
    same(got, exp, f"edges c={c}")
    assert np.array_equal(got[1], IDENTITY)
    assert got[3][8] == 0  # the blinders alone are not the identity


# ------------------------------------------------------- threads

def test_threads_race_lazy_build(plib, orc, srs10):
    """Four threads on one FRESH context commit the same batch at once: they
    race the lazy build of the bases, the window table and the lookup table."""
    ptau, g1 = srs10
    n, B = 1024, 3
    polys, blinders = pool(n)
    polys, blinders = polys[:B], blinders[:B]
    exp = pool_expected(orc, g1, n, B)
    fresh = plib.init(ptau, (1 << POWER) + 2)
    got, lookup = [None] * 4, [None] * 4
    gate = threading.Barrier(4)

    def run(t):
        gate.wait()
        got[t] = commit(fresh, polys, blinders, n)
        lookup[t] = took_entry_lookup(plib)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    fresh.close()
    for t in range(4):
        assert got[t] is not None and np.array_equal(got[t], exp), f"thread {t}"
        assert lookup[t], f"thread {t} left the lookup path"


# ---- child processes: RNG_R1_LOOKUP* and RNG_MSM_LOOKUP_MAX_MB are read once ----

def block_polys(n):
    """entry counts around the 256-lane block: 300 ones (not a multiple of
    256, a second block's worth at S >= 2), 7 ones (lanes > entries), a
    sparse poly, an empty one, and 256 + 1 entries"""
    rng = random.Random(9300)
    assert n == 256

    def ones(k):
        p = [0] * n
        for i in rng.sample(range(n), k):
            p[i] = 1
        return p

    full = [R - 1] * 9 + [0] * (n - 9)   # 9 values x up to 32 digits: about 288 entries
    polys = [ones(250), ones(7), sparse_poly(rng, n), [0] * n, full, ones(255)]
    # full-width blinders add up to 2 x 32 digits (about 314), (1, 1) adds 2 (257)
    blinders = [(rng.randrange(1 << 253, R), rng.randrange(1 << 253, R)), (0, 0), (0, 0),
                (0, 0), (0, 0), (1, 1)]
    return polys, blinders


def child_main(what, outfile):
    from renegade_amd import load_prover
    from tests.orc_bindings import OracleLib
    if what == "prove":
        from tests.test_lagrange_commit import child_main as prove_child
        return prove_child(outfile)
    orc = OracleLib(str(REPO / "oracle" / "liborc.so"))
    plib = load_prover()
    plib.require_gpu()
    ptau = orc.srs_generate_ptau(POWER, seed=42)
    out = {}
    n = 256
    if what == "blocks":
        polys, blinders = block_polys(n)
        for c in CS:
            ctx = plib.init(ptau, (1 << POWER) + 2)
            out[f"c{c}"] = commit(ctx, polys, blinders, n, c)
            ctx.close()
    else:  # "fallback": the caller's c = 8 and the prover's own rule
        polys, blinders = edge_polys(8, n)
        ctx = plib.init(ptau, (1 << POWER) + 2)
        out["c8"] = commit(ctx, polys, blinders, n, 8)
        sparse, sb = pool(n)
        out["auto"] = commit(ctx, sparse[:5], sb[:5], n, 0)
        ctx.close()
    np.savez(outfile, **out)


def run_child(what, tmp_path, tag, **env_add):
    outfile = tmp_path / f"{what}_{tag}.npz"
    env = dict(os.environ, RNG_MSM_DEBUG="1")
    for name in ("RNG_MSM_C", "RNG_MSM_LOOKUP", "RNG_MSM_LOOKUP_MAX_MB", "RNG_R1_LOOKUP",
                 "RNG_R1_LOOKUP_S", "RNG_R1_LAGRANGE", "RNG_MSM_SEGCAP"):
        env.pop(name, None)
    env.update(env_add)
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), what, str(outfile)],
                       cwd=str(REPO), env=env, timeout=300, capture_output=True, text=True)
    # a failed child ends the test here: the next one is not started
    assert r.returncode == 0, f"{what} {env_add} child rc={r.returncode}\n{r.stderr[-2000:]}"
    return np.load(outfile), r.stderr


def msm_lines(stderr):
    return [ln for ln in stderr.splitlines() if ln.startswith("[msm]")]


@pytest.mark.parametrize("S", [3, 1])
def test_blocks_per_poly(orc, srs10, tmp_path, S):
    """S = 3: polys of about 314 and 288 entries and of 257 spread over three
    blocks, the last one wholly empty; S = 1: one block strides over them,
    and 7 entries leave 249 lanes idle."""
    _, g1 = srs10
    n = 256
    polys, blinders = block_polys(n)
    res, stderr = run_child("blocks", tmp_path, f"s{S}", RNG_R1_LOOKUP_S=str(S))
    exp = np.stack([expected(orc, g1, p, b, n) for p, b in zip(polys, blinders)])
    lines = msm_lines(stderr)
    for c in CS:
        same(res[f"c{c}"], exp, f"S={S} c={c}")
        hits = [ln for ln in lines if f"entry-lookup c={c} S={S} " in ln]
        assert len(hits) == 1 and "(compacted)" in hits[0], stderr[-2000:]
    assert np.array_equal(res["c8"][3], IDENTITY)


@pytest.mark.parametrize("env_add", [{"RNG_MSM_LOOKUP_MAX_MB": "1"}, {"RNG_R1_LOOKUP": "0"}],
                         ids=["budget", "switch_off"])
def test_fallback(orc, srs10, tmp_path, env_add):
    """No table (1 MB budget) or the switch at 0: the bucket pipeline over
    compacted digits commits, at the caller's c = 8 and under the prover's
    own rule, and no lookup table is built over the Lagrange bases."""
    _, g1 = srs10
    n = 256
    res, stderr = run_child("fallback", tmp_path, "_".join(env_add), **env_add)
    polys, blinders = edge_polys(8, n)
    exp = np.stack([expected(orc, g1, p, b, n) for p, b in zip(polys, blinders)])
    same(res["c8"], exp, f"fallback {env_add} c=8")
    same(res["auto"], pool_expected(orc, g1, n, 5), f"fallback {env_add} auto")
    lines = msm_lines(stderr)
    bucket = [ln for ln in lines if "(compacted)" in ln and "chunk=" in ln and " c=8 " in ln]
    assert len(bucket) == 2, stderr[-2000:]
    assert not any("entry-lookup" in ln or "lookup table" in ln for ln in lines), stderr[-2000:]


def compacted_paths(stderr):
    """marker -> the paths ('entry-lookup' / 'buckets') of the '(compacted)'
    MSM debug lines that followed it"""
    paths, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("@@ "):
            cur = " ".join(line.split()[1:3])
            paths[cur] = []
        elif cur is not None and line.startswith("[msm]") and "(compacted)" in line:
            paths[cur].append("entry-lookup" if "entry-lookup" in line else "buckets")
    return paths


def test_prover_paths_agree(plib, tmp_path):
    """RNG_R1_LOOKUP=0 and =1 under RNG_R1_LAGRANGE=1 give the same proofs
    and link hints, byte for byte, from rng_prove and rng_prove_cohort (k = 3)
    on the settlement circuit (and the small test circuit), and the debug
    lines show that round 1 of the settlement calls took the bucket pipeline
    with =0 and the lookup sum with =1."""
    results, paths = [], []
    for mode in ("0", "1"):
        res, stderr = run_child("prove", tmp_path, mode, RNG_R1_LOOKUP=mode,
                                RNG_R1_LAGRANGE="1")
        results.append(res)
        paths.append(compacted_paths(stderr))
    off, on = results
    assert sorted(off.files) == sorted(on.files) and len(off.files) == 8
    for key in off.files:
        assert np.array_equal(off[key], on[key]), f"{key} differs between the paths"
        assert off[key].any()
    for section in ("settlement single", "settlement cohort"):
        assert paths[0][section] == ["buckets"], paths[0]
        assert paths[1][section] == ["entry-lookup"], paths[1]


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
