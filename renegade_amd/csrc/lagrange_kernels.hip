// PRODUCT PATH — Lagrange-basis commitments for the round-1 wire polynomials
// ("Lagrange basis over compacted digits").
//
// The commitment of a wire polynomial is the same group element whether it
// is computed from the n+2 blinded coefficients against [tau^j] or from the
// n wire EVALUATIONS against [L_i(tau)] plus the two blinders against
// [tau^n] - [tau^0] and [tau^(n+1)] - [tau^1].  The evaluations are sparse
// where the coefficients are dense, so this file provides
//  1. the bases: an inverse radix-2 NTT over G1 of the first n SRS points
//     (k_g1_ntt_*), the 1/n scaling, the two blinding bases and the
//     normalisation to G1Aff (k_g1_normalize);
//  2. compacted digit extraction (k_msm_digit_count / k_msm_digits_compact):
//     only the non-zero signed digits are written, with the key/val packing
//     of k_msm_digits_fixed, so every later MSM stage runs on the real
//     entry count;
//  3. k_lagrange_scalars: canonical evaluations + blinders at stride n+2.
#include <hip/hip_runtime.h>
#include "gpu_curve.hpp"
#include "msm_digits.hpp"

namespace rng {

struct Canon4 {  // one canonical scalar passed by value
    uint64_t l[4];
};

// s * p by double-and-add from the top set bit; s canonical LE
__device__ inline G1Jac g1_mul_canon(const G1Jac& p, const uint64_t s[4]) {
    int top = -1;
    for (int i = 3; i >= 0 && top < 0; --i)
        if (s[i]) top = 64 * i + 63 - __clzll((long long)s[i]);
    G1Jac acc = G1Jac::identity();
    for (int bit = top; bit >= 0; --bit) {
        acc = acc.dbl();
        if ((s[bit >> 6] >> (bit & 63)) & 1) acc = acc.add(p);
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_g1_ntt_load(const G1Aff* srs, uint32_t n,
                                                     G1Jac* pts) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pts[i] = G1Jac::from_affine(srs[i]);
}

// One decimation-in-frequency pass of half-length h (h = n/2 first, 1 last;
// natural order in, bit-reversed order out after the last pass).  Butterfly
// t pairs i0 = blk*2h + j with i1 = i0 + h:
//   pts[i0] = a + b,  pts[i1] = (a - b) * winv^(j * n/(2h)).
// tw[e] = winv^e for e < n/2 (Montgomery).  A twiddle of 1 (j == 0, which
// covers the whole last pass) skips the multiplication.
__global__ __launch_bounds__(64) void k_g1_ntt_pass(G1Jac* pts, uint32_t n, uint32_t h,
                                                    const Fr* tw) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n / 2) return;
    uint32_t blk = t / h, j = t - blk * h;
    uint32_t i0 = blk * 2 * h + j, i1 = i0 + h;
    G1Jac a = pts[i0], b = pts[i1];
    pts[i0] = a.add(b);
    b.Y = b.Y.neg();
    G1Jac d = a.add(b);
    if (j != 0) {
        uint64_t s[4];
        tw[j * (n / (2 * h))].to_canonical(s);
        d = g1_mul_canon(d, s);
    }
    pts[i1] = d;
}

// out[i] = (1/n) * in[bitrev(i)] for i < n; out[n] = [tau^n] - [tau^0],
// out[n+1] = [tau^(n+1)] - [tau^1] (the blinding bases).  logn >= 1.
__global__ __launch_bounds__(64) void k_g1_ntt_finish(const G1Jac* in, const G1Aff* srs,
                                                      uint32_t n, uint32_t logn,
                                                      Canon4 ninv, G1Jac* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + 2) return;
    if (i >= n) {
        out[i] = G1Jac::from_affine(srs[i]).madd(srs[i - n], true);
        return;
    }
    uint32_t r = __brev(i) >> (32 - logn);
    out[i] = g1_mul_canon(in[r], ninv.l);
}

// Jacobian -> affine, LAG_NORM consecutive points per thread behind one
// field inversion.  G1Aff cannot hold infinity: any Z == 0 raises *bad and
// the host marks the domain unusable.
constexpr uint32_t LAG_NORM = 8;

__global__ __launch_bounds__(64) void k_g1_normalize(const G1Jac* pts, uint32_t N,
                                                     G1Aff* out, uint32_t* bad) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t lo = t * LAG_NORM;
    if (lo >= N) return;
    uint32_t cnt = N - lo < LAG_NORM ? N - lo : LAG_NORM;
    Fq pref[LAG_NORM];  // pref[j] = Z_0 * ... * Z_j
    Fq run = Fq::one();
    for (uint32_t j = 0; j < cnt; ++j) {
        Fq z = pts[lo + j].Z;
        if (z.is_zero()) {
            atomicOr(bad, 1u);
            return;
        }
        run = run.mul(z);
        pref[j] = run;
    }
    Fq inv = run.inverse();
    for (int j = (int)cnt - 1; j >= 0; --j) {
        G1Jac p = pts[lo + j];
        Fq zinv = j ? inv.mul(pref[j - 1]) : inv;
        inv = inv.mul(p.Z);
        Fq zinv2 = zinv.sqr();
        G1Aff a;
        a.x = p.X.mul(zinv2);
        a.y = p.Y.mul(zinv2.mul(zinv));
        out[lo + j] = a;
    }
}

// ---- compacted digits (fixed-base packing, non-zero digits only) ----

// the signed base-2^c digits of one scalar, as k_msm_digits_fixed derives
// them; f(w, mag, sign) is called for every NON-ZERO digit
template <typename F>
__device__ inline void msm_signed_digits(const uint64_t s[4], uint32_t c, uint32_t W, F f) {
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; ++w) {
        MsmDigit d = msm_recode_digit(s, c, w, carry);
        if (d.mag) f(w, d.mag, d.sign);
    }
}

// counts[idx] = non-zero digits of scalar idx (idx < total_scalars = n*B)
__global__ __launch_bounds__(256) void k_msm_digit_count(const uint64_t* scalars,
                                                         uint32_t total_scalars, uint32_t c,
                                                         uint32_t W, uint32_t* counts) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total_scalars) return;
    uint64_t s[4] = {scalars[4 * idx], scalars[4 * idx + 1], scalars[4 * idx + 2],
                     scalars[4 * idx + 3]};
    uint32_t cnt = 0;
    if (s[0] | s[1] | s[2] | s[3])
        msm_signed_digits(s, c, W, [&](uint32_t, uint32_t, uint32_t) { ++cnt; });
    counts[idx] = cnt;
}

// scatter after the exclusive scan of counts: key = poly << c | magnitude,
// val = sign << 31 | (w*N + i), exactly k_msm_digits_fixed's packing
__global__ __launch_bounds__(256) void k_msm_digits_compact(
    const uint64_t* scalars, uint32_t n, uint32_t c, uint32_t W, uint32_t B, uint32_t N,
    const uint32_t* offs, uint32_t* keys, uint32_t* vals) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * B) return;
    uint64_t s[4] = {scalars[4 * idx], scalars[4 * idx + 1], scalars[4 * idx + 2],
                     scalars[4 * idx + 3]};
    if (!(s[0] | s[1] | s[2] | s[3])) return;
    uint32_t b = idx / n, i = idx % n;
    uint32_t o = offs[idx];
    msm_signed_digits(s, c, W, [&](uint32_t w, uint32_t mag, uint32_t sign) {
        keys[o] = (b << c) | mag;
        vals[o] = (sign << 31) | (w * N + i);
        ++o;
    });
}

// non-zero scalars among `total` (the density figure behind the window rule)
__global__ __launch_bounds__(256) void k_count_nonzero_scalars(const uint64_t* scalars,
                                                               uint32_t total,
                                                               uint32_t* out) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    bool nz = false;
    if (idx < total)
        nz = (scalars[4 * idx] | scalars[4 * idx + 1] | scalars[4 * idx + 2] |
              scalars[4 * idx + 3]) != 0;
    uint32_t cnt = (uint32_t)__popcll(__ballot(nz));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(out, cnt);
}

// canonical scalars of B polys at stride n+2: the n evaluations (Montgomery
// in), then the poly's two blinders (zero where blinders == nullptr)
__global__ __launch_bounds__(256) void k_lagrange_scalars(const Fr* evals,
                                                          const Fr* blinders, uint32_t n,
                                                          uint64_t total /* B*(n+2) */,
                                                          uint64_t* out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    uint64_t g = i / (n + 2);
    uint32_t j = (uint32_t)(i - g * (n + 2));
    Fr v = j < n ? evals[g * n + j] : (blinders ? blinders[2 * g + (j - n)] : Fr::zero());
    v.to_canonical(out + 4 * i);
}

}  // namespace rng
