#!/usr/bin/env python3
"""Headline benchmark for the MI355X PlonK-prover backend.

Driver contract: `python bench.py --gpus N --steps K --warmup W` — one rank
per GPU (torchrun for N>1; invoked directly with --gpus N>1 it self-launches
torchrun), rank 0 prints ONE JSON line.  A plain run does only what the
headline figure needs: setup, warmup, the K timed steps, the result line.
`--dump-outputs DIR` additionally writes what the last timed step produced
as DIR/<name>.npy (float64, see dump_u64).  `--full` adds everything else
described below: the cohort-vs-single parity checks, the MSM/NTT kernel
legs (roofline, extra) and the cpu_baseline.

Workload (BASELINE.json configs[3], the config the proofs/sec leg of the
metric is quoted on): one step = one cohort of `--jobs` (default 48)
concurrent `Intent And Balance Private Settlement` TurboPlonk proofs (the
VALID MATCH MPC successor) on the GPU prover — synthetic
fixed-seed witnesses, deterministic generated SRS, measured domain n reported
in config.  A batch is the step unit because the production shape is a
saturated prover pool (native_proof_manager.rs:143-148); all steps' proofs
are queued at once, so the timed region is steady-state at any --steps.
Proof jobs are embarrassingly parallel across GPUs => weak scaling, no
data-path collective; `value` is whole-job proofs/s across all ranks.

With `--full`, the roofline object reports the flagship MSM kernel (BASELINE configs[1]:
2^20-point BN254 G1 Pippenger) measured in the same run with HIP events:
bytes_alg per MSM = W*64*N + 2*32*N = 1088 B/point, the
bucket_reduce kernel's share = W*(64+8)*N.  `extra` carries the NTT 2^22
round-trip leg (configs[2]) and the per-kernel MSM breakdown.

cpu_baseline (`--full`): the CPU oracle prover (oracle/plonk.hpp, kind="port") on the
same circuit tables, all host cores, bounded sample.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (8 TB/s), MI355X_MICROARCH.md
MSM_LOG2N = 20
MSM_WINDOW_C = 16
U64P = ctypes.POINTER(ctypes.c_uint64)


def ptr(a):
    return a.ctypes.data_as(U64P)


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def dump_u64(out_dir, name, a):
    """Write a uint64 array as DIR/<name>.npy in float64 without loss: the
    last axis doubles, holding the (low, high) 32-bit halves of each word."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    halves = a.view(np.uint32).reshape(a.shape[:-1] + (2 * a.shape[-1],))
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    np.save(out_dir / f"{name}.npy", halves.astype(np.float64))


def build_settlement_tables(lib):
    lib.rng_circ_build_settlement.restype = ctypes.c_void_p
    lib.rng_circ_build_settlement.argtypes = [ctypes.c_uint64]
    lib.rng_circ_n.restype = ctypes.c_uint64
    lib.rng_circ_n.argtypes = [ctypes.c_void_p]
    lib.rng_circ_npub.restype = ctypes.c_uint64
    lib.rng_circ_npub.argtypes = [ctypes.c_void_p]
    lib.rng_circ_get.argtypes = [ctypes.c_void_p, U64P, U64P, U64P, U64P]
    lib.rng_circ_free.argtypes = [ctypes.c_void_p]
    h = lib.rng_circ_build_settlement(42)
    assert h, "settlement circuit build failed"
    n = lib.rng_circ_n(h)
    npub = lib.rng_circ_npub(h)
    sel = np.zeros(13 * n * 4, dtype=np.uint64)
    sigma = np.zeros(5 * n, dtype=np.uint64)
    wires = np.zeros(5 * n * 4, dtype=np.uint64)
    pubs = np.zeros(npub * 4, dtype=np.uint64)
    lib.rng_circ_get(h, ptr(sel), ptr(sigma), ptr(wires), ptr(pubs))
    lib.rng_circ_free(h)
    return n, npub, sel, sigma, wires, pubs


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("num_public", ctypes.c_uint64),
                ("selectors", U64P), ("sigma", U64P),
                ("num_link_groups", ctypes.c_uint64), ("link_offsets", U64P)]


def cpu_baseline_proofs(orc, n, npub, sel, sigma, wires, pubs, srs_records, max_degree,
                        cores):
    o = orc.lib
    o.orc_plonk_preprocess.restype = ctypes.c_void_p
    o.orc_plonk_preprocess.argtypes = [ctypes.c_uint64, ctypes.c_uint64, U64P, U64P,
                                       U64P, ctypes.c_uint64]
    o.orc_plonk_prove.argtypes = [ctypes.c_void_p, U64P, U64P, ctypes.c_uint64, U64P]
    pk = o.orc_plonk_preprocess(n, npub, ptr(sel), ptr(sigma), ptr(srs_records),
                                max_degree + 1)
    assert pk
    from concurrent.futures import ThreadPoolExecutor

    def one(seed):
        proof = np.zeros(157, dtype=np.uint64)
        rc = o.orc_plonk_prove(ctypes.c_void_p(pk), ptr(wires), ptr(pubs),
                               ctypes.c_uint64(seed), ptr(proof))
        assert rc == 0
        return proof

    one(0)  # warm
    t0 = time.perf_counter()
    done = 0
    with ThreadPoolExecutor(max_workers=cores) as ex:
        futs = []
        # bound the sample: ~15 s wall target, chunked submission
        while time.perf_counter() - t0 < 15.0 and done < 4 * cores:
            futs.append(ex.submit(one, 1000 + done))
            done += 1
        for f in futs:
            f.result()
    dt = time.perf_counter() - t0
    return {
        "value": round(done / dt, 3),
        "unit": "proofs/s",
        "cores": cores,
        "kind": "port",
        "sample": f"{done} settlement proofs (n={n}) on {cores} threads, oracle prover",
    }


def bundle_mode(args, plib, orc, dist, rank, local_rank, n_gpus):
    """Full production bundle throughput: one step = the complete response of
    native_proof_manager.rs:554-590 — 1 settlement proof (n=4096) + 2
    INTENT AND BALANCE VALIDITY proofs (n=16384) + 2 OUTPUT BALANCE VALIDITY
    proofs (n=8192) + 4 cross-domain link proofs, all on the GPU."""
    lib = plib.lib
    lib.rng_circ_n.restype = ctypes.c_uint64
    lib.rng_circ_n.argtypes = [ctypes.c_void_p]
    lib.rng_circ_npub.restype = ctypes.c_uint64
    lib.rng_circ_npub.argtypes = [ctypes.c_void_p]
    lib.rng_circ_get.argtypes = [ctypes.c_void_p, U64P, U64P, U64P, U64P]
    lib.rng_circ_num_link_groups.restype = ctypes.c_uint64
    lib.rng_circ_num_link_groups.argtypes = [ctypes.c_void_p]
    lib.rng_circ_link_groups.argtypes = [ctypes.c_void_p, U64P]
    lib.rng_circ_free.argtypes = [ctypes.c_void_p]
    lib.rng_circ_build_settlement_bundle.restype = ctypes.c_void_p
    lib.rng_circ_build_settlement_bundle.argtypes = [ctypes.c_uint64]
    lib.rng_circ_build_validity.restype = ctypes.c_void_p
    lib.rng_circ_build_validity.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.rng_circ_build_ob_validity.restype = ctypes.c_void_p
    lib.rng_circ_build_ob_validity.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.rng_link_proofs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, U64P, U64P,
                                    ctypes.c_uint64, ctypes.c_uint64,
                                    ctypes.c_uint64, U64P]

    def fetch(h):
        assert h
        n = lib.rng_circ_n(h)
        npub = lib.rng_circ_npub(h)
        nlg = lib.rng_circ_num_link_groups(h)
        lg = np.zeros(3 * max(1, nlg), dtype=np.uint64)
        lib.rng_circ_link_groups(h, ptr(lg))
        sel = np.zeros(13 * n * 4, dtype=np.uint64)
        sigma = np.zeros(5 * n, dtype=np.uint64)
        wires = np.zeros(5 * n * 4, dtype=np.uint64)
        pubs = np.zeros(max(1, npub * 4), dtype=np.uint64)
        lib.rng_circ_get(h, ptr(sel), ptr(sigma), ptr(wires), ptr(pubs))
        lib.rng_circ_free(h)
        return dict(n=n, npub=npub, lg=lg.reshape(-1, 3), sel=sel, sigma=sigma,
                    wires=wires, pubs=pubs)

    ts = fetch(lib.rng_circ_build_settlement_bundle(42))
    tv = [fetch(lib.rng_circ_build_validity(42, p)) for p in range(2)]
    to = [fetch(lib.rng_circ_build_ob_validity(42, p)) for p in range(2)]
    n_big = max(int(ts["n"]), int(tv[0]["n"]), int(to[0]["n"]))
    power = max(4, int(n_big).bit_length())
    ptau = orc.srs_generate_ptau(power, seed=42)
    max_degree = (1 << power) + 2
    ctx = plib.init(ptau, max_degree)

    def mkpk(t):
        desc = Desc(t["n"], t["npub"], ptr(t["sel"]), ptr(t["sigma"]), 0, None)
        pk = lib.rng_preprocess(ctx.h, ctypes.byref(desc))
        assert pk
        return pk

    pk_s, pk_v, pk_o = mkpk(ts), mkpk(tv[0]), mkpk(to[0])
    groups = sorted((int(r[1]), int(r[0]), int(r[2])) for r in ts["lg"])
    # offsets ascending = party0(17), out0(11), party1(17), out1(11)
    legs = [(groups[0], pk_v, tv[0]), (groups[1], pk_o, to[0]),
            (groups[2], pk_v, tv[1]), (groups[3], pk_o, to[1])]
    pk_big = pk_v if int(tv[0]["n"]) == n_big else pk_s

    def ext(h, n_small, out):
        out[:4 * (n_small + 2)] = h[:4 * (n_small + 2)]
        out[4 * (n_small + 2):-9] = 0
        out[-9:] = h[-9:]

    lib.rng_prove_cohort.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_uint64, U64P, U64P, U64P, U64P, U64P]
    from concurrent.futures import ThreadPoolExecutor
    link_pool = ThreadPoolExecutor(max_workers=16)
    kb = args.jobs  # bundles per step

    def cohort(pk, tables, kk_each, seeds):
        """Prove len(tables)*kk_each proofs under one PK: kk_each copies of
        each table's witness, concatenated table-major."""
        n = int(tables[0]["n"])
        kk = kk_each * len(tables)
        wires = np.concatenate([np.tile(t["wires"], kk_each) for t in tables])
        pubs = np.concatenate([np.tile(t["pubs"], kk_each) for t in tables])
        proofs = np.zeros(157 * kk, dtype=np.uint64)
        hints = np.zeros((4 * (n + 2) + 9) * kk, dtype=np.uint64)
        rc = lib.rng_prove_cohort(ctx.h, ctypes.c_void_p(pk), kk, ptr(wires),
                                  ptr(pubs), ptr(seeds), ptr(proofs), ptr(hints))
        assert rc == 0, f"rng_prove_cohort rc={rc}"
        return proofs, hints.reshape(kk, -1)

    def step(seed_base):
        """One step = `jobs` production bundles: the same-position proofs of
        all bundles prove as cohorts (settlement xk, ib-validity x2k covering
        both parties, ob-validity x2k), then the 4k cross-domain link proofs
        run on a thread pool — the batched shape of
        native_proof_manager.rs:554-590."""
        sd = lambda off: (np.uint64(seed_base + off * 100000) +
                          np.arange(2 * kb, dtype=np.uint64))
        sp, sh = cohort(pk_s, [ts], kb, sd(0)[:kb])
        vp, vh = cohort(pk_v, [tv[0], tv[1]], kb, sd(1))
        op, oh = cohort(pk_o, [to[0], to[1]], kb, sd(2))
        # legs (offset-ascending): validity p0, ob p0, validity p1, ob p1;
        # party p's hints are rows [p*kb, (p+1)*kb) of the 2k cohorts
        leg_hints = [(vh, int(tv[0]["n"]), 0), (oh, int(to[0]["n"]), 0),
                     (vh, int(tv[0]["n"]), 1), (oh, int(to[0]["n"]), 1)]

        def links_for(b):
            hs_e = np.zeros(4 * (n_big + 2) + 9, dtype=np.uint64)
            ext(sh[b], int(ts["n"]), hs_e)
            lps = np.zeros((4, 18), dtype=np.uint64)
            for i, ((off, align, cnt), _pk, _t) in enumerate(legs):
                rows, n_leg, party = leg_hints[i]
                hv_e = np.zeros(4 * (n_big + 2) + 9, dtype=np.uint64)
                ext(rows[party * kb + b], n_leg, hv_e)
                assert lib.rng_link_proofs(ctx.h, ctypes.c_void_p(pk_big),
                                           ptr(hv_e), ptr(hs_e), align, off, cnt,
                                           ptr(lps[i])) == 0
            return lps

        lps = list(link_pool.map(links_for, range(kb)))
        return {"settlement_proofs": sp.reshape(kb, 157),
                "validity_proofs": vp.reshape(2 * kb, 157),
                "ob_validity_proofs": op.reshape(2 * kb, 157),
                "link_proofs": np.stack(lps).reshape(kb, 4 * 18)}

    step_pool = ThreadPoolExecutor(
        max_workers=max(1, int(os.environ.get("RNG_BENCH_INFLIGHT", "2"))))
    for i in range(max(1, min(args.warmup, 4))):
        step(100 + i * 100_000)
    ctx.sync()
    if dist:
        dist.barrier()
    ctx.sync()
    t0 = time.perf_counter()
    futs = [step_pool.submit(step, 10_000_000 + rank * 100_000_000 + i * 100_000)
            for i in range(args.steps)]
    outs = [f.result() for f in futs]
    ctx.sync()
    if dist:
        import torch
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    else:
        elapsed = time.perf_counter() - t0
    if rank == 0 and args.dump_outputs:
        for name, a in outs[-1].items():
            dump_u64(args.dump_outputs, name, a)
    if rank == 0:
        out = {
            "metric": "settlement_bundles_per_s",
            "value": round(args.steps * args.jobs * n_gpus / elapsed, 3),
            "unit": "bundles/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1000.0 * elapsed / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic",
            "config": {
                "workload": "production proof bundle: 1 settlement (n=4096) + 2 "
                            "intent-and-balance validity (n=16384) + 2 output-"
                            "balance validity (n=8192) + 4 cross-domain link "
                            "proofs (native_proof_manager.rs:554-590); one step "
                            "= `jobs` bundles, same-position proofs cohorted",
                "bundles_per_step": args.jobs,
            },
        }
        print(json.dumps(out), flush=True)
    # join worker threads BEFORE interpreter teardown so their TLS HIP
    # scratch frees while the runtime is still alive
    link_pool.shutdown(wait=True)
    step_pool.shutdown(wait=True)
    if dist:
        dist.destroy_process_group()


def msm_shard_mode(args, plib, orc, dist, rank, local_rank, n_gpus):
    """BASELINE configs[4]: 2^20-point MSM base-split across ranks; exchange =
    all-gather of per-rank G1 partials (EC add is not an RCCL reduce op) +
    host fold.  Strong scaling (total work fixed)."""
    import ctypes as ct
    from renegade_amd.dist import shard_bounds, combine_shard_results
    lib = plib.lib
    lib.rng_g1_add_affine.argtypes = [U64P, U64P, U64P]
    n = 1 << MSM_LOG2N
    ptau, bases8, scalars = None, None, None
    power = 12
    ptau = orc.srs_generate_ptau(power, seed=42)
    g1, _, _ = orc.srs_parse(ptau, (1 << power) + 2)
    npts = g1.shape[0]
    reps = (n + npts - 1) // npts
    bases8 = np.ascontiguousarray(
        np.tile(np.ascontiguousarray(g1[:, :8]), (reps, 1))[:n])
    rng = np.random.default_rng(777)
    scalars = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    scalars[:, 3] &= (1 << 61) - 1
    ctx = plib.init(ptau, (1 << power) + 2)
    world = max(1, n_gpus if dist else 1)
    lo, hi = shard_bounds(n, world, rank)
    db = ctx.dbuf_from(np.ascontiguousarray(bases8[lo:hi]).reshape(-1))
    ds = ctx.dbuf_from(np.ascontiguousarray(scalars[lo:hi]).reshape(-1))

    def add_fn(a, b):
        out = np.zeros(9, dtype=np.uint64)
        lib.rng_g1_add_affine(ptr(a), ptr(b), ptr(out))
        return out

    def step():
        part = ctx.msm_dev(db, ds, hi - lo, window_c=0)
        if dist:
            return combine_shard_results(dist, part, add_fn)
        return part

    for _ in range(args.warmup):
        out = step()
    if dist:
        dist.barrier()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    ctx.sync()
    if dist:
        import torch
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    else:
        elapsed = time.perf_counter() - t0
    if rank == 0 and args.dump_outputs:
        dump_u64(args.dump_outputs, "msm_result", res)
    if rank == 0:
        bytes_alg = n * (MSM_WINDOW_C * 64 + 2 * 32)
        value = bytes_alg * args.steps / elapsed / 1e9
        # verify vs oracle once (bounded n -> do a spot equality across modes)
        result = {
            "metric": "BN254 G1 MSM 2^20 base-split across ranks (algorithmic GB/s)",
            "value": round(value, 2),
            "unit": "GB/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "u256",
            "data": "synthetic",
            "config": {"workload": "msm_2^20_base_split", "points": n,
                       "per_rank_points": hi - lo,
                       "exchange": "all_gather(72B G1 record) + host EC fold",
                       "parallelism": f"base-split x{n_gpus}"},
            "roofline": None,
            "cpu_baseline": None,
        }
        print(json.dumps(result), flush=True)
    if dist:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the "
                         "cohort-vs-single parity checks, the MSM/NTT kernel legs "
                         "(roofline, extra) and the cpu_baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs "
                         "(proof words as float64 32-bit halves) to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the cpu_baseline")
    ap.add_argument("--jobs", type=int, default=48,
                    help="cohort size: proofs advanced in lockstep per step "
                         "(the reference proves from a rayon pool; measured "
                         "optimum 48 with 4 cohorts in flight)")
    ap.add_argument("--no-kernel-legs", action="store_true",
                    help="with --full: skip the MSM/NTT kernel side-measurements")
    ap.add_argument("--mode", choices=["proofs", "msm-shard", "bundle"],
                    default="proofs",
                    help="msm-shard = BASELINE configs[4]: one 2^20 MSM base-split "
                         "across ranks, RCCL all-gather of partials + host EC fold; "
                         "bundle = full production bundle (1 settlement + 4 validity "
                         "proofs + 4 link proofs) per step")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world == 1:
        # invoked directly with --gpus N: self-launch one rank per GPU so the
        # printed value can never be a single rank's work multiplied by N
        # 
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               f"--nproc-per-node={args.gpus}", "--standalone",
               "--local-addr", "127.0.0.1", str(REPO / "bench.py")] + sys.argv[1:]
        log(f"bench: self-launching torchrun for --gpus {args.gpus}")
        sys.exit(subprocess.run(cmd).returncode)
    n_gpus = world if world > 1 else args.gpus

    from renegade_amd import load_prover
    from tests.orc_bindings import OracleLib
    if not (REPO / "oracle" / "liborc.so").exists():
        subprocess.run(["make", "-C", str(REPO / "oracle")], check=True)
    orc = OracleLib(str(REPO / "oracle" / "liborc.so"))
    plib = load_prover()
    plib.require_gpu()
    try:
        plib.set_device(local_rank)
    except Exception:
        plib.set_device(0)  # over-subscribed smoke runs on fewer GPUs
    lib = plib.lib
    lib.rng_preprocess.restype = ctypes.c_void_p
    lib.rng_preprocess.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.rng_prove.argtypes = [ctypes.c_void_p, ctypes.c_void_p, U64P, U64P,
                              ctypes.c_uint64, U64P, U64P]

    dist = None
    if world > 1:
        import torch
        import torch.distributed as td
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("RNG_DIST_BACKEND", "nccl")
        td.init_process_group(backend=backend, rank=rank, world_size=world)
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
        dist = td

    if args.mode == "msm-shard":
        return msm_shard_mode(args, plib, orc, dist, rank, local_rank, n_gpus)
    if args.mode == "bundle":
        return bundle_mode(args, plib, orc, dist, rank, local_rank, n_gpus)

    # --- setup: circuit tables + SRS + PK ---
    n, npub, sel, sigma, wires, pubs = build_settlement_tables(lib)
    power = max(4, int(n).bit_length())
    ptau = orc.srs_generate_ptau(power, seed=42)
    max_degree = (1 << power) + 2
    ctx = plib.init(ptau, max_degree)
    desc = Desc(n, npub, ptr(sel), ptr(sigma), 0, None)
    pk = lib.rng_preprocess(ctx.h, ctypes.byref(desc))
    assert pk, "rng_preprocess failed"
    lib.rng_prove_cohort.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_uint64, U64P, U64P, U64P, U64P, U64P]
    proof = np.zeros(157, dtype=np.uint64)

    def prove_one(seed, buf=proof):
        rc = lib.rng_prove(ctx.h, ctypes.c_void_p(pk), ptr(wires), ptr(pubs),
                           ctypes.c_uint64(seed), ptr(buf), None)
        assert rc == 0, f"rng_prove rc={rc}"

    # one STEP = one COHORT of `jobs` proofs advanced in lockstep with fused
    # per-round MSMs (rng_prove_cohort) — the batched shape of the
    # reference's proof-job pool (native_proof_manager.rs:143-148).  A few
    # cohorts stay in flight on separate threads/streams so host phases of
    # one overlap GPU phases of another; value stays robust at any --steps.
    k = args.jobs
    wires_all = np.tile(wires, k)
    pubs_all = np.tile(pubs, k)

    def step(seed_base, buf):
        seeds = (seed_base + np.arange(k, dtype=np.uint64)).astype(np.uint64)
        rc = lib.rng_prove_cohort(ctx.h, ctypes.c_void_p(pk), k, ptr(wires_all),
                                  ptr(pubs_all), ptr(seeds), ptr(buf), None)
        assert rc == 0, f"rng_prove_cohort rc={rc}"

    # first cohort on the calling thread, before the pool threads exist.  It
    # is part of the warmup, not only the subject of the check below: the
    # headline has always been measured after it, and without it the timed
    # steps run measurably slower (about 1100-1500 against 1600-1650
    # proofs/s in interleaved runs on one MI355X).
    cbuf0 = np.zeros(157 * k, dtype=np.uint64)
    step(12345, cbuf0)
    if args.full:
        # determinism + cohort-vs-single parity spot check
        prove_one(12345)
        assert np.array_equal(cbuf0[:157], proof), "cohort[0] differs from single proof"
        prove_one(12345 + k - 1)
        assert np.array_equal(cbuf0[157 * (k - 1):], proof), \
            "cohort[k-1] differs from single proof"

    from concurrent.futures import ThreadPoolExecutor
    inflight = max(1, int(os.environ.get("RNG_BENCH_INFLIGHT", "4")))
    pool = ThreadPoolExecutor(max_workers=inflight)
    bufs = [np.zeros(157 * k, dtype=np.uint64) for _ in range(inflight)]
    # the last timed step writes a buffer of its own: the shared ones may be
    # rewritten by a neighbouring step still in flight, and this one is what
    # --dump-outputs stores
    last_buf = np.zeros(157 * k, dtype=np.uint64)

    def buf_for(i):
        return last_buf if i == args.steps - 1 else bufs[i % inflight]

    for w in range(max(1, min(args.warmup, 8))):
        list(pool.map(lambda j: step(500 + (w * inflight + j) * 10 * k, bufs[j]),
                      range(inflight)))
    ctx.sync()

    total_proofs = args.steps * k
    if dist:
        dist.barrier()
    ctx.sync()
    t0 = time.perf_counter()
    futs = [pool.submit(step, 10_000 + rank * 10_000_000 + i * 10 * k,
                        buf_for(i))
            for i in range(args.steps)]
    for f in futs:
        f.result()
    ctx.sync()
    elapsed = time.perf_counter() - t0
    if args.full:
        # concurrency correctness: a cohort proof produced under the thread pool
        # must be bit-identical to the same seed proved alone
        last0 = args.steps - 1 - ((args.steps - 1) % inflight)
        prove_one(10_000 + rank * 10_000_000 + last0 * 10 * k)
        assert np.array_equal(proof, buf_for(last0)[:157]), \
            "pooled cohort differs from serial"
    if dist:
        import torch
        # NCCL collectives operate on device tensors
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    proofs_per_s = total_proofs * n_gpus / elapsed

    if rank == 0 and args.dump_outputs:
        dump_u64(args.dump_outputs, "proofs", last_buf.reshape(k, 157))

    # --- kernel legs (rank 0): MSM 2^20 roofline + NTT 2^22 ---
    roofline = None
    ntt_extra = None
    msm_extra = None
    if rank == 0 and args.full and not args.no_kernel_legs:
        g1, _, _ = orc.srs_parse(ptau, max_degree)
        npts = g1.shape[0]
        nb = 1 << MSM_LOG2N
        reps = (nb + npts - 1) // npts
        bases8 = np.ascontiguousarray(
            np.tile(np.ascontiguousarray(g1[:, :8]), (reps, 1))[:nb].reshape(-1))
        rng = np.random.default_rng(12345)
        scalars = rng.integers(0, 1 << 64, size=4 * nb, dtype=np.uint64)
        scalars[3::4] &= (1 << 61) - 1
        dbases = ctx.dbuf_from(bases8)
        dscalars = ctx.dbuf_from(scalars)
        for _ in range(2):
            ctx.msm_dev(dbases, dscalars, nb, window_c=MSM_WINDOW_C)
        t1 = time.perf_counter()
        kt = []
        for _ in range(5):
            ctx.msm_dev(dbases, dscalars, nb, window_c=MSM_WINDOW_C)
            kt.append(plib.msm_last_times())
        msm_ms = (time.perf_counter() - t1) / 5 * 1e3
        avg_bucket_ms = float(np.mean([k["bucket_reduce"] for k in kt]))
        bucket_bytes = MSM_WINDOW_C * (64 + 8) * nb
        achieved = bucket_bytes / (avg_bucket_ms / 1e3) / 1e9
        traffic = None
        pmc_path = REPO / "profiles" / "pmc_traffic.json"
        if pmc_path.exists():
            pmc = json.load(open(pmc_path))
            traffic = pmc.get("fetch_size_reported_bytes_per_launch")
        roofline = {
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": traffic,
            "traffic_note": "FETCH_SIZE reported bytes/launch from committed PMC "
                            "profile (profiles/pmc_traffic.json; gfx950 counter "
                            "caveats in DESIGN.md)" if traffic else None,
            "kernel": "k_msm_bucket_reduce (msm 2^20 leg)",
            "kernel_ms": round(avg_bucket_ms, 3),
        }
        msm_extra = {
            "msm_2^20_ms": round(msm_ms, 3),
            "alg_gbs": round(nb * (MSM_WINDOW_C * 64 + 64) / (msm_ms / 1e3) / 1e9, 1),
            "breakdown_ms": {k: round(float(np.mean([t[k] for t in kt])), 3)
                             for k in kt[0]},
        }
        ctx.dbuf_free(dbases)
        ctx.dbuf_free(dscalars)

        m = 1 << 22
        nd = np.random.default_rng(5).integers(0, 1 << 61, size=4 * m, dtype=np.uint64)
        da = ctx.dbuf_from(nd)
        db = ctx.dbuf_alloc(nd.nbytes)
        for _ in range(2):
            ctx.ntt_dev_oop(da, db, m)
            ctx.ntt_dev_oop(db, da, m, inverse=True)
        ctx.sync()
        t1 = time.perf_counter()
        for _ in range(5):
            ctx.ntt_dev_oop(da, db, m)
            ctx.ntt_dev_oop(db, da, m, inverse=True)
        ctx.sync()
        rt_ms = (time.perf_counter() - t1) / 5 * 1e3
        back = np.empty_like(nd)
        ctx.dbuf_download(da, back)
        assert np.array_equal(back, nd), "NTT round-trip mismatch in bench"
        ntt_extra = {
            "roundtrip_ms": round(rt_ms, 3),
            "alg_gbs": round(2 * 2 * 2 * 32 * m / (rt_ms / 1e3) / 1e9, 1),
            "pass_ms": {k: round(v, 3) for k, v in plib.ntt_last_times().items()},
        }
        ctx.dbuf_free(da)
        ctx.dbuf_free(db)

    if rank == 0:
        cores = os.cpu_count()
        cb = None
        if args.full and not args.no_cpu_baseline:
            g1, _, _ = orc.srs_parse(ptau, max_degree)
            srs_records = np.ascontiguousarray(g1).reshape(-1)
            cb = cpu_baseline_proofs(orc, n, npub, sel, sigma, wires, pubs, srs_records,
                                     max_degree, cores)
        result = {
            "metric": "VALID MATCH MPC proofs/sec (Intent And Balance Private Settlement)",
            "value": round(proofs_per_s, 3),
            "unit": "proofs/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u256",
            "data": "synthetic",
            "config": {
                "workload": "intent_and_balance_private_settlement_proof",
                "domain_n": int(n),
                "num_public": int(npub),
                "srs_power": power,
                "prover_mode": "cohort (lockstep rounds, fused per-round MSMs)",
                "proofs_per_step": args.jobs,
                "total_proofs": total_proofs * n_gpus,
                "parallelism": f"x{n_gpus} gpus, cohort={args.jobs}, "
                               f"{inflight} in flight",
            },
            "roofline": roofline,
            "cpu_baseline": cb,
            "extra": {"msm_2^20": msm_extra, "ntt_2^22": ntt_extra},
        }
        print(json.dumps(result), flush=True)

    pool.shutdown(wait=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
    sys.stdout.flush()
    sys.stderr.flush()
    # The JSON is printed and all Python pools are joined.  Exit normally, so
    # that exit handlers (the interpreter's, a profiler's, any tool that
    # records what the process loaded) still run; an os._exit here used to
    # skip them all.  The library guards its destructors against a torn-down
    # HIP runtime (r01's rc=139).  Join the library's worker-pool threads
    # first so no finalizer can stall on them.
    try:
        import ctypes as _ct
        _ct.CDLL(str(REPO / "renegade_amd" / "librenegade_prover.so")).rng_shutdown_pool()
    except Exception:
        pass
