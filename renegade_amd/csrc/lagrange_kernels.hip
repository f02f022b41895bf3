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
//  3. k_lagrange_scalars: canonical evaluations + blinders at stride n+2;
//  4. k_msm_entry_lookup_sum: the commitment as a plain signed sum over the
//     compacted entries, each gathering its digit multiple from a lookup
//     table over the bases (k_msm_lookup_table over the domain's window
//     table), with k_msm_digit_count_density feeding it the entry offsets
//     and the density figure in one pass.
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

// the block's sum of one flag per lane, added to *out by ONE atomic (every
// lane of the 256-lane block calls this)
__device__ inline void block_count_add(bool flag, uint32_t* out) {
    __shared__ uint32_t wave_cnt[4];
    const uint32_t cnt = (uint32_t)__popcll(__ballot(flag));
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t sum = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (sum) atomicAdd(out, sum);
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

// k_msm_digit_count for the lookup sum over compacted entries: also writes
// counts[total_scalars] = 0, so the exclusive scan over total_scalars + 1
// words ends in the entry total and every poly's range has an upper end, and
// adds the non-zero SCALARS (the density figure) to *nonzero, one atomic per
// block.  The grid covers total_scalars + 1 lanes.
__global__ __launch_bounds__(256) void k_msm_digit_count_density(
    const uint64_t* scalars, uint32_t total_scalars, uint32_t c, uint32_t W, uint32_t* counts,
    uint32_t* nonzero) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t cnt = 0;
    if (idx < total_scalars) {
        uint64_t s[4] = {scalars[4 * idx], scalars[4 * idx + 1], scalars[4 * idx + 2],
                         scalars[4 * idx + 3]};
        if (s[0] | s[1] | s[2] | s[3])
            msm_signed_digits(s, c, W, [&](uint32_t, uint32_t, uint32_t) { ++cnt; });
    }
    if (idx <= total_scalars) counts[idx] = cnt;
    // a non-zero scalar has a non-zero digit
    block_count_add(cnt != 0, nonzero);
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
        keys[o] = msm_entry_key(b, mag, c);
        vals[o] = msm_entry_val(w, N, i, sign);
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
    block_count_add(nz, out);
}

// ---- lookup sum over compacted entries ----
// table: L[((w*N + i) << (c-1)) + d-1] = d * 2^(c*w) * base_i over the N
// bases of a domain (k_msm_lookup_table over the domain's window table).
// keys/vals: the entries k_msm_digits_compact wrote; scalars lie poly-major,
// so poly b owns the entries offs[b*N] .. offs[(b+1)*N] (offs has B*N + 1
// words, the last one the entry total) and nothing is sorted.
//
// grid (S, B), 256 lanes: the lanes of block (x, b) stride over poly b's
// range from x*256 + lane in steps of S*256, add the looked-up points into
// one Jacobian each, and the block folds them through LDS into
// partials[b*S + x].  Lanes past the range hold the identity and stay out
// of the fold; a block past the range only writes the identity.  No lane
// reads an entry outside [lo, hi).
__global__ __launch_bounds__(256) void k_msm_entry_lookup_sum(
    const uint32_t* keys, const uint32_t* vals, const uint32_t* offs, uint32_t N, uint32_t c,
    const G1Aff* table, G1Jac* partials) {
    __shared__ G1Jac red[256];
    const uint32_t b = blockIdx.y;
    const uint32_t lo = offs[(uint64_t)b * N], hi = offs[(uint64_t)(b + 1) * N];
    const uint32_t first = blockIdx.x * 256;  // S <= 2^16: no overflow
    G1Jac* out = partials + (uint64_t)b * gridDim.x + blockIdx.x;
    if (first >= hi - lo) {  // block-uniform
        if (threadIdx.x == 0) *out = G1Jac::identity();
        return;
    }
    const uint32_t active = hi - lo - first < 256 ? hi - lo - first : 256;
    const uint64_t step = (uint64_t)gridDim.x * 256;
    G1Jac acc = G1Jac::identity();
    for (uint64_t e = (uint64_t)lo + first + threadIdx.x; e < hi; e += step) {
        const uint32_t key = keys[e], val = vals[e];
        const G1Aff p = table[msm_lookup_index(key, val, c)];
        acc = acc.madd(p, msm_entry_sign(val) != 0);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t stride = 128; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride && threadIdx.x + stride < active)
            red[threadIdx.x] = red[threadIdx.x].add(red[threadIdx.x + stride]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
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
