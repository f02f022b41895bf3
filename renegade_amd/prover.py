"""ctypes wrapper over librenegade_prover.so (the product C ABI).

Mirrors the reference's prover call surface for this path:
the names and argument meanings follow include/rng_prover.h, which cites the
reference interface each entry point replaces.
"""
import ctypes
import os
from pathlib import Path

import numpy as np

_U64P = ctypes.POINTER(ctypes.c_uint64)
_U8P = ctypes.POINTER(ctypes.c_uint8)

PROOF_U64S = 157


class ProverError(RuntimeError):
    pass


def _lib_path() -> Path:
    here = Path(__file__).resolve().parent
    return here / "librenegade_prover.so"


def load_prover():
    """Load the HIP prover library; raises loudly if absent or unbuilt."""
    p = _lib_path()
    if not p.exists():
        raise ProverError(
            f"HIP prover extension not found at {p}. Build it with "
            f"`python -c 'import __graft_entry__; __graft_entry__.build()'` — "
            f"there is no CPU fallback."
        )
    return ProverLib(str(p))


def _ptr(a):
    return a.ctypes.data_as(_U64P)


class ProverLib:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.rng_prover_init.restype = ctypes.c_void_p
        self.lib.rng_prover_init.argtypes = [_U8P, ctypes.c_size_t, ctypes.c_uint64]
        self.lib.rng_ctx_free.argtypes = [ctypes.c_void_p]
        self.lib.rng_version.restype = ctypes.c_char_p
        self.lib.rng_dbuf_alloc.restype = ctypes.c_void_p
        self.lib.rng_dbuf_alloc.argtypes = [ctypes.c_size_t]
        self.lib.rng_dbuf_free.argtypes = [ctypes.c_void_p]
        self.lib.rng_dbuf_upload.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        self.lib.rng_dbuf_download.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        self.lib.rng_ntt_fr.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_uint64,
                                        ctypes.c_uint64, ctypes.c_int]
        self.lib.rng_ntt_fr_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
        self.lib.rng_ntt_fr_dev_oop.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.c_uint64, ctypes.c_int]
        self.lib.rng_msm_g1.argtypes = [ctypes.c_void_p, _U64P, _U64P, ctypes.c_uint64,
                                        _U64P, ctypes.c_int]
        self.lib.rng_msm_g1_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_uint64, _U64P,
                                            ctypes.c_int]
        self.lib.rng_msm_srs_batch.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_uint64,
                                               ctypes.c_uint32, ctypes.c_int,
                                               ctypes.c_int, _U64P]
        self.lib.rng_commit_lagrange.argtypes = [ctypes.c_void_p, ctypes.c_uint64, _U64P,
                                                 _U64P, ctypes.c_uint32, ctypes.c_int,
                                                 _U64P]
        self.lib.rng_perm_product.argtypes = [ctypes.c_void_p, _U64P, _U64P, _U64P, _U64P,
                                              ctypes.c_uint64, ctypes.c_uint64, _U64P]
        self.lib.rng_perm_product_pk.argtypes = [ctypes.c_void_p, ctypes.c_void_p, _U64P,
                                                 _U64P, ctypes.c_uint64, ctypes.c_int,
                                                 _U64P]
        self.lib.rng_poly_horner.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                             _U64P, ctypes.c_int, _U64P]
        self.lib.rng_open_pk.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                         _U64P, _U64P, _U64P, ctypes.c_int, _U64P]
        self.lib.rng_quotient_pk.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint64, _U64P, _U64P, _U64P,
                                             ctypes.c_int, _U64P, _U64P]
        self.lib.rng_srs_dev_bases.restype = ctypes.c_void_p
        self.lib.rng_srs_dev_bases.argtypes = [ctypes.c_void_p, _U64P]

    @property
    def version(self) -> str:
        return self.lib.rng_version().decode()

    def set_device(self, dev: int):
        rc = self.lib.rng_set_device(dev)
        if rc != 0:
            raise ProverError(f"rng_set_device({dev}) failed rc={rc}")

    def msm_last_times(self):
        out = (ctypes.c_double * 5)()
        self.lib.rng_msm_last_times(out)
        return {"digits": out[0], "sort": out[1], "bucket_reduce": out[2],
                "window_chunks": out[3], "final": out[4]}

    def ntt_last_times(self):
        out = (ctypes.c_double * 2)()
        self.lib.rng_ntt_last_times(out)
        return {"pass1": out[0], "pass2": out[1]}

    @property
    def gpu_available(self) -> bool:
        return bool(self.lib.rng_gpu_available())

    def require_gpu(self):
        if not self.gpu_available:
            raise ProverError("no AMD GPU visible — the product path requires MI355X")

    # ---- context ----
    def init(self, srs_ptau: bytes, max_degree: int) -> "ProverCtx":
        buf = (ctypes.c_uint8 * len(srs_ptau)).from_buffer_copy(srs_ptau)
        h = self.lib.rng_prover_init(buf, len(srs_ptau), max_degree)
        if not h:
            raise ProverError("rng_prover_init failed (bad SRS?)")
        return ProverCtx(self, h)


class ProverCtx:
    def __init__(self, plib: ProverLib, handle):
        self._plib = plib
        self.lib = plib.lib
        self.h = handle

    def close(self):
        if self.h:
            self.lib.rng_ctx_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise ProverError(f"{what} failed rc={rc}")

    # ---- primitives ----
    def ntt(self, data: np.ndarray, n: int, batch: int = 1, inverse: bool = False):
        """In-place NTT on a host uint64 array of 4*n*batch limbs."""
        assert data.dtype == np.uint64 and data.size == 4 * n * batch
        self._check(self.lib.rng_ntt_fr(self.h, _ptr(data), n, batch,
                                        1 if inverse else 0), "rng_ntt_fr")

    def msm(self, bases: np.ndarray, scalars: np.ndarray, n: int, window_c: int = 0):
        """bases: 8*n u64 (x,y Montgomery); scalars: 4*n u64 canonical.
        Returns 9-u64 affine record."""
        assert bases.dtype == np.uint64 and bases.size == 8 * n
        assert scalars.dtype == np.uint64 and scalars.size == 4 * n
        out = np.zeros(9, dtype=np.uint64)
        self._check(self.lib.rng_msm_g1(self.h, _ptr(bases), _ptr(scalars), n, _ptr(out),
                                        window_c), "rng_msm_g1")
        return out

    MSM_AUTO, MSM_FIXED_BASE, MSM_WINDOWED, MSM_LOOKUP = 0, 1, 2, 3

    def msm_srs_batch(self, scalars: np.ndarray, n: int, batch: int = 1,
                      window_c: int = 0, mode: int = 0):
        """`batch` polynomials of n canonical scalars each (4*n*batch u64)
        against the first n SRS points, through the prover's own commitment
        MSM.  mode: MSM_AUTO / MSM_FIXED_BASE / MSM_WINDOWED / MSM_LOOKUP.  Returns a
        (batch, 9) array of affine records."""
        assert scalars.dtype == np.uint64 and scalars.size == 4 * n * batch
        scalars = np.ascontiguousarray(scalars).reshape(-1)
        out = np.zeros(9 * batch, dtype=np.uint64)
        self._check(self.lib.rng_msm_srs_batch(self.h, _ptr(scalars), n, batch, window_c,
                                               mode, _ptr(out)), "rng_msm_srs_batch")
        return out.reshape(batch, 9)

    def commit_lagrange(self, evals: np.ndarray, n: int, batch: int = 1, blinders=None,
                        window_c: int = 0):
        """The prover's round-1 commitment on the Lagrange path: `batch`
        evaluation vectors of n canonical scalars each (4*n*batch u64) and,
        optionally, two canonical blinders per vector (8*batch u64).
        Returns a (batch, 9) array of affine records."""
        assert evals.dtype == np.uint64 and evals.size == 4 * n * batch
        evals = np.ascontiguousarray(evals).reshape(-1)
        bptr = None
        if blinders is not None:
            assert blinders.dtype == np.uint64 and blinders.size == 8 * batch
            blinders = np.ascontiguousarray(blinders).reshape(-1)
            bptr = _ptr(blinders)
        out = np.zeros(9 * batch, dtype=np.uint64)
        self._check(self.lib.rng_commit_lagrange(self.h, n, _ptr(evals), bptr, batch,
                                                 window_c, _ptr(out)),
                    "rng_commit_lagrange")
        return out.reshape(batch, 9)

    Z_AUTO, Z_DEVICE, Z_HOST = 0, 1, 2

    def perm_product(self, wires: np.ndarray, sigma_evals: np.ndarray, k5: np.ndarray,
                     beta_gamma: np.ndarray, n: int, batch: int = 1):
        """Permutation grand product z on the GPU.  Montgomery limbs: wires
        batch*5*n Fr (column-major per proof), sigma_evals 5*n Fr, k5 5 Fr,
        beta_gamma batch*(beta, gamma).  Returns a (batch, n, 4) array."""
        for a, fr in ((wires, 5 * n * batch), (sigma_evals, 5 * n), (k5, 5),
                      (beta_gamma, 2 * batch)):
            assert a.dtype == np.uint64 and a.size == 4 * fr
        args = [np.ascontiguousarray(a).reshape(-1)
                for a in (wires, sigma_evals, k5, beta_gamma)]
        out = np.zeros(4 * n * batch, dtype=np.uint64)
        self._check(self.lib.rng_perm_product(self.h, *map(_ptr, args), n, batch,
                                              _ptr(out)), "rng_perm_product")
        return out.reshape(batch, n, 4)

    def perm_product_pk(self, pk, wires: np.ndarray, beta_gamma: np.ndarray, n: int,
                        batch: int = 1, mode: int = 0):
        """The prover's own round-2 call against proving key `pk` (a
        rng_preprocess handle of domain size n).  mode: Z_AUTO / Z_DEVICE /
        Z_HOST.  Returns a (batch, n, 4) array."""
        assert wires.dtype == np.uint64 and wires.size == 4 * 5 * n * batch
        assert beta_gamma.dtype == np.uint64 and beta_gamma.size == 8 * batch
        wires = np.ascontiguousarray(wires).reshape(-1)
        beta_gamma = np.ascontiguousarray(beta_gamma).reshape(-1)
        out = np.zeros(4 * n * batch, dtype=np.uint64)
        self._check(self.lib.rng_perm_product_pk(self.h, ctypes.c_void_p(pk), _ptr(wires),
                                                 _ptr(beta_gamma), batch, mode,
                                                 _ptr(out)), "rng_perm_product_pk")
        return out.reshape(batch, n, 4)

    HORNER_EVAL, HORNER_DIVIDE = 0, 1

    def poly_horner(self, polys: np.ndarray, points: np.ndarray, length: int,
                    group: int = 1, batch: int = 1, shared: bool = False,
                    mode: int = 0):
        """Batched Horner scan on the GPU.  Montgomery limbs: polys
        batch*group*length Fr (group*length when shared), points batch Fr.
        HORNER_EVAL returns the evaluations, (batch, group, 4); HORNER_DIVIDE
        the quotients by (X - point), (batch, group, length - 1, 4)."""
        assert polys.dtype == np.uint64 and points.dtype == np.uint64
        assert polys.size == 4 * length * group * (1 if shared else batch)
        assert points.size == 4 * batch
        polys = np.ascontiguousarray(polys).reshape(-1)
        points = np.ascontiguousarray(points).reshape(-1)
        per_seq = 1 if mode == self.HORNER_EVAL else length - 1
        out = np.zeros(4 * batch * group * per_seq, dtype=np.uint64)
        self._check(self.lib.rng_poly_horner(self.h, _ptr(polys), length, group, batch,
                                             1 if shared else 0, _ptr(points), mode,
                                             _ptr(out)), "rng_poly_horner")
        if mode == self.HORNER_EVAL:
            return out.reshape(batch, group, 4)
        return out.reshape(batch, group, length - 1, 4)

    OPEN_AUTO, OPEN_DEVICE, OPEN_HOST = 0, 1, 2

    def open_pk(self, pk, polys: np.ndarray, points: np.ndarray, scalars: np.ndarray,
                n: int, k: int = 1, mode: int = 0):
        """The prover's own call for the batched opening against proving key
        `pk` (domain size n): polys k*11*(n+3) Fr (wires 0..4, z, chunks 0..4,
        zero-padded), points k*(zeta, zeta*w), scalars k*29 in the order of
        open_scalars.  mode: OPEN_AUTO / OPEN_DEVICE / OPEN_HOST.  Returns
        (k, 2, n + 2, 4): W_zeta and W_zeta_w of each proof."""
        for a, fr in ((polys, 11 * (n + 3) * k), (points, 2 * k), (scalars, 29 * k)):
            assert a.dtype == np.uint64 and a.size == 4 * fr
        args = [np.ascontiguousarray(a).reshape(-1) for a in (polys, points, scalars)]
        out = np.zeros(4 * 2 * (n + 2) * k, dtype=np.uint64)
        self._check(self.lib.rng_open_pk(self.h, ctypes.c_void_p(pk), k, *map(_ptr, args),
                                         mode, _ptr(out)), "rng_open_pk")
        return out.reshape(k, 2, n + 2, 4)

    QUOT_AUTO, QUOT_OUT_OF_PLACE, QUOT_IN_PLACE = 0, 1, 2

    def quotient_pk(self, pk, polys: np.ndarray, challenges: np.ndarray, n: int,
                    k: int = 1, blinders=None, mode: int = 0):
        """The prover's own round-3 call against proving key `pk` (domain
        size n): polys k*7*(n+3) Fr (wires 0..4, z, PI, zero-padded),
        challenges k*(beta, gamma, alpha), blinders k*4 chunk blinders or
        None for zeros.  mode: QUOT_AUTO / QUOT_OUT_OF_PLACE / QUOT_IN_PLACE
        (the two coset-extension arms).  Returns (chunks, quot): the blinded
        chunks, (k, 5, n + 3, 4), and every quotient coefficient before the
        split, (k, 8n, 4)."""
        for a, fr in ((polys, 7 * (n + 3) * k), (challenges, 3 * k)):
            assert a.dtype == np.uint64 and a.size == 4 * fr
        polys = np.ascontiguousarray(polys).reshape(-1)
        challenges = np.ascontiguousarray(challenges).reshape(-1)
        bptr = None
        if blinders is not None:
            assert blinders.dtype == np.uint64 and blinders.size == 4 * 4 * k
            blinders = np.ascontiguousarray(blinders).reshape(-1)
            bptr = _ptr(blinders)
        chunks = np.zeros(4 * 5 * (n + 3) * k, dtype=np.uint64)
        quot = np.zeros(4 * 8 * n * k, dtype=np.uint64)
        self._check(self.lib.rng_quotient_pk(self.h, ctypes.c_void_p(pk), k, _ptr(polys),
                                             _ptr(challenges), bptr, mode, _ptr(chunks),
                                             _ptr(quot)), "rng_quotient_pk")
        return chunks.reshape(k, 5, n + 3, 4), quot.reshape(k, 8 * n, 4)

    # ---- device-resident helpers (benchmarking) ----
    def dbuf_from(self, host: np.ndarray):
        nbytes = host.nbytes
        d = self.lib.rng_dbuf_alloc(nbytes)
        if not d:
            raise ProverError("rng_dbuf_alloc failed")
        self._check(self.lib.rng_dbuf_upload(d, host.ctypes.data_as(ctypes.c_void_p),
                                             nbytes), "upload")
        return d

    def dbuf_alloc(self, nbytes: int):
        d = self.lib.rng_dbuf_alloc(nbytes)
        if not d:
            raise ProverError("rng_dbuf_alloc failed")
        return d

    def dbuf_download(self, d, host: np.ndarray):
        self._check(self.lib.rng_dbuf_download(d, host.ctypes.data_as(ctypes.c_void_p),
                                               host.nbytes), "download")

    def dbuf_free(self, d):
        self.lib.rng_dbuf_free(d)

    def ntt_dev(self, d, n, batch=1, inverse=False):
        self._check(self.lib.rng_ntt_fr_dev(self.h, d, n, batch, 1 if inverse else 0),
                    "rng_ntt_fr_dev")

    def ntt_dev_oop(self, din, dout, n, batch=1, inverse=False):
        self._check(self.lib.rng_ntt_fr_dev_oop(self.h, din, dout, n, batch,
                                                1 if inverse else 0), "rng_ntt_fr_dev_oop")

    def msm_dev(self, dbases, dscalars, n, window_c=0):
        out = np.zeros(9, dtype=np.uint64)
        self._check(self.lib.rng_msm_g1_dev(self.h, dbases, dscalars, n, _ptr(out),
                                            window_c), "rng_msm_g1_dev")
        return out

    def sync(self):
        self._check(self.lib.rng_device_sync(), "rng_device_sync")
