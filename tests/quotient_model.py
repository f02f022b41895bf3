"""Round 3 of the prover (the quotient stage behind rng_quotient_pk) on plain
Python ints: canonical residues mod r, no Montgomery form, no device tables.

For one proof, with g the coset generator, w_m the 8n-th root of unity and
x_t = g w_m^t for t < m = 8n:
  1. selector, sigma and L1 coefficients = inverse DFT over H of their
     evaluations (sigma evaluations are K5[slot // n] * w_n^(slot % n), L1 is
     the interpolant of e_0);
  2. every polynomial is evaluated at every x_t;
  3. num(t) = gate(t) + alpha [z f - z_shift g] + alpha^2 (z - 1) L1, the
     formula at the head of plonk_kernels.hip, selector order = enum Sel of
     plonk_circuit.hpp, z_shift = z(x_{(t+8) mod m}) = z(w_n x_t);
  4. q(t) = num(t) / (x_t^n - 1);
  5. quotient coefficients = inverse DFT of q over the m points, times g^-j;
  6. chunk i = coefficients i(n+2) .. (i+1)(n+2)-1, [0] -= b_{i-1} for i > 0,
     [n+2] += b_i for i < 4, length n+3.

Two routes for the transforms, the same pointwise arithmetic:
  NAIVE  every transform an O(N^2) sum or a Horner evaluation per point, all
         in Python ints: nothing but pow and % is trusted;
  ORC    the oracle's orc_ntt (pinned against bignums in test_oracle_core.py)
         for the DFTs, Python ints for everything else.
route_for(n) gives NAIVE up to n = 16; the tests assert that both routes
agree there, which anchors the larger sizes.
"""
import numpy as np

from tests import py_ref as ref

R = ref.R
G = 5                                   # FR_GENERATOR (include/bn254_params.h)
K5 = [pow(7, j, R) for j in range(5)]   # coset_ks (plonk_circuit.hpp)
NAIVE, ORC = "naive", "orc"
NAIVE_MAX_N = 16
# enum Sel (plonk_circuit.hpp)
LC0, LC1, LC2, LC3, MUL0, MUL1, HASH0, HASH1, HASH2, HASH3, SEL_O, SEL_C, ECC = range(13)
NUM_SEL = 13


def route_for(n):
    return NAIVE if n <= NAIVE_MAX_N else ORC


def horner(coeffs, x):
    s = 0
    for c in reversed(coeffs):
        s = (c + x * s) % R
    return s


def _pack(vals):
    buf = b"".join((v * ref.R256 % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).copy()


def _unpack(a):
    b = a.tobytes()
    rinv = pow(ref.R256, -1, R)
    return [int.from_bytes(b[i:i + 32], "little") * rinv % R for i in range(0, len(b), 32)]


class Transforms:
    """DFTs over the subgroup of size N and its coset g H, by one route."""

    def __init__(self, route, orc=None):
        assert route in (NAIVE, ORC)
        assert route == NAIVE or orc is not None
        self.route, self.orc = route, orc

    def _orc_ntt(self, vals, inverse):
        data = _pack(vals)
        self.orc.ntt(data, len(vals), inverse=inverse)
        return _unpack(data)

    def interpolate(self, evals):
        """evaluations over H_N (natural order) -> N coefficients"""
        N = len(evals)
        if self.route == ORC:
            return self._orc_ntt(evals, True)
        winv = pow(ref.fr_root_of_unity(N), -1, R)
        ninv = pow(N, -1, R)
        out = []
        for j in range(N):
            step, x, s = pow(winv, j, R), 1, 0
            for e in evals:
                s = (s + e * x) % R
                x = x * step % R
            out.append(s * ninv % R)
        return out

    def coset_evaluate(self, coeffs, N):
        """coefficients (any length <= N) -> values at g w_N^t, t < N"""
        assert len(coeffs) <= N
        if self.route == ORC:
            scaled, gj = [], 1
            for c in coeffs:
                scaled.append(c * gj % R)
                gj = gj * G % R
            return self._orc_ntt(scaled + [0] * (N - len(coeffs)), False)
        w = ref.fr_root_of_unity(N)
        out, x = [], G
        for _ in range(N):
            out.append(horner(coeffs, x))
            x = x * w % R
        return out

    def coset_interpolate(self, evals):
        """values at g w_N^t -> N coefficients"""
        c = self.interpolate(evals)
        ginv = pow(G, -1, R)
        out, gj = [], 1
        for v in c:
            out.append(v * gj % R)
            gj = gj * ginv % R
        return out


def sigma_evals(sigma_idx, n):
    w = ref.fr_root_of_unity(n)
    wp = [pow(w, t, R) for t in range(n)]
    return [K5[int(s) // n] * wp[int(s) % n] % R for s in sigma_idx]


class Key:
    """What rng_preprocess derives for round 3, from the same inputs:
    sel = 13 columns of n evaluations, sigma_idx = 5n slot indices."""

    def __init__(self, tf, n, sel, sigma_idx):
        assert len(sel) == NUM_SEL and all(len(c) == n for c in sel)
        assert len(sigma_idx) == 5 * n
        self.tf, self.n, self.m = tf, n, 8 * n
        m = self.m
        sig = sigma_evals(sigma_idx, n)
        self.sel_coef = [tf.interpolate(list(c)) for c in sel]
        self.sig_coef = [tf.interpolate(sig[j * n:(j + 1) * n]) for j in range(5)]
        self.l1_coef = tf.interpolate([1] + [0] * (n - 1))
        self.sel_coset = [tf.coset_evaluate(c, m) for c in self.sel_coef]
        self.sig_coset = [tf.coset_evaluate(c, m) for c in self.sig_coef]
        self.l1_coset = tf.coset_evaluate(self.l1_coef, m)
        wm = ref.fr_root_of_unity(m)
        self.x = [G * pow(wm, t, R) % R for t in range(m)]
        self.zh_inv = [pow(pow(x, n, R) - 1, -1, R) for x in self.x]


def numerator(w, z, z_shift, pi, sel, sig, l1, x, beta, gamma, alpha):
    """num at one point, from the values of every polynomial there"""
    def p5(v):
        return pow(v, 5, R)
    gate = (sel[SEL_C] + pi
            + sel[LC0] * w[0] + sel[LC1] * w[1] + sel[LC2] * w[2] + sel[LC3] * w[3]
            + sel[MUL0] * w[0] * w[1] + sel[MUL1] * w[2] * w[3]
            + sel[HASH0] * p5(w[0]) + sel[HASH1] * p5(w[1])
            + sel[HASH2] * p5(w[2]) + sel[HASH3] * p5(w[3])
            + sel[ECC] * w[0] * w[1] * w[2] * w[3] * w[4]
            - sel[SEL_O] * w[4])
    f = g = 1
    for j in range(5):
        f = f * (w[j] + beta * K5[j] * x + gamma) % R
        g = g * (w[j] + beta * sig[j] + gamma) % R
    perm = alpha * (z * f - z_shift * g)
    l1term = alpha * alpha * (z - 1) * l1
    return (gate + perm + l1term) % R


def split_chunks(quot, n, blinders):
    b = list(blinders) if blinders is not None else [0] * 4
    chunks = []
    for i in range(5):
        c = quot[i * (n + 2):(i + 1) * (n + 2)] + [0]
        if i > 0:
            c[0] = (c[0] - b[i - 1]) % R
        if i < 4:
            c[n + 2] = (c[n + 2] + b[i]) % R
        chunks.append(c)
    return chunks


def quotient(key, polys, beta, gamma, alpha, blinders=None):
    """polys: 7 coefficient lists of n+3 (wires 0..4, z, PI).
    -> (5 chunks of n+3, the 8n quotient coefficients)"""
    n, m, tf = key.n, key.m, key.tf
    assert len(polys) == 7 and all(len(p) == n + 3 for p in polys)
    ev = [tf.coset_evaluate(p, m) for p in polys]
    q = []
    for t in range(m):
        num = numerator([ev[j][t] for j in range(5)], ev[5][t], ev[5][(t + 8) % m], ev[6][t],
                        [c[t] for c in key.sel_coset], [c[t] for c in key.sig_coset],
                        key.l1_coset[t], key.x[t], beta, gamma, alpha)
        q.append(num * key.zh_inv[t] % R)
    quot = tf.coset_interpolate(q)
    return split_chunks(quot, n, blinders), quot


# ------------------------------------------- the identity at a single point

def eval_from_evals(evals, zeta):
    """Value at zeta of the interpolant of `evals` over H_n, by the
    barycentric formula on Python ints (no transform)."""
    n = len(evals)
    w = ref.fr_root_of_unity(n)
    s, wi = 0, 1
    for e in evals:
        if e:
            s = (s + e * wi % R * pow(zeta - wi, -1, R)) % R
        wi = wi * w % R
    return s * (pow(zeta, n, R) - 1) % R * pow(n, -1, R) % R


def numerator_at(n, sel, sigma_idx, polys, beta, gamma, alpha, zeta):
    """num(zeta) straight from the circuit's columns and the seven
    coefficient polynomials: Horner and the barycentric formula only."""
    w = ref.fr_root_of_unity(n)
    sig = sigma_evals(sigma_idx, n)
    return numerator([horner(polys[j], zeta) for j in range(5)], horner(polys[5], zeta),
                     horner(polys[5], zeta * w % R), horner(polys[6], zeta),
                     [eval_from_evals(c, zeta) for c in sel],
                     [eval_from_evals(sig[j * n:(j + 1) * n], zeta) for j in range(5)],
                     eval_from_evals([1] + [0] * (n - 1), zeta), zeta, beta, gamma, alpha)


def chunks_at(chunks, n, zeta):
    """sum_i chunk_i(zeta) zeta^(i(n+2))"""
    return sum(horner(c, zeta) * pow(zeta, i * (n + 2), R) for i, c in enumerate(chunks)) % R


def blind_wire(coeffs, n, b0, b1):
    """k_blind_wires_batch: n coefficients -> n+3 with [0] -= b0, [1] -= b1,
    [n] += b0, [n+1] += b1"""
    v = list(coeffs) + [0, 0, 0]
    v[0], v[1] = (v[0] - b0) % R, (v[1] - b1) % R
    v[n], v[n + 1] = (v[n] + b0) % R, (v[n + 1] + b1) % R
    return v


def blind_z(coeffs, n, b2, b3, b4):
    """k_blind_z_batch: [0] -= b4, [1] -= b3, [2] -= b2, [n] += b4,
    [n+1] += b3, [n+2] += b2"""
    v = list(coeffs) + [0, 0, 0]
    for j, b in enumerate((b4, b3, b2)):
        v[j] = (v[j] - b) % R
        v[n + j] = (v[n + j] + b) % R
    return v
