// PRODUCT PATH — MI355X-native Pippenger MSM over BN254 G1.
//
// Replaces: arkworks ark-ec VariableBaseMSM as consumed through the
// reference's KZG commitments (BASELINE config #2).
//
// Structure (sort-based, designed for gfx950; B polynomials batch through
// one pipeline via key group g = poly*W + window):
//  1. k_msm_digits: signed windowed digit decomposition (c in {8,13,16} so
//     the TOP window stays populated — see msm_auto_c), one
//     (key = group<<16 | magnitude, val = sign<<31 | point index) pair per
//     nonzero digit; zero digits get the dynamic sentinel (G<<16).
//  2. rocPRIM device radix sort over the live key bits only (3 passes) —
//     groups every bucket's points together; no atomics or EC critical
//     sections anywhere.
//  3. segment heads via flag+select; long segments split into capped
//     sub-segments (k_msm_seg_lengths / k_msm_make_subs), reduced
//     longest-first one lane each with Jacobian mixed adds
//     (k_msm_bucket_reduce), then merged per bucket longest-first
//     (k_msm_seg_merge).
//  4. k_msm_window_chunks: per (window, chunk) suffix running sums ->
//     (sum, weighted-sum) partials; chunk size adapts to keep >=32k lanes.
//  5. k_msm_window_combine: per-window fold of the chunk partials
//     (sub-block count adapts); the final Horner across windows runs on
//     the HOST (a 1-lane dependent EC chain is far faster on a host core).
//
// Fixed-base mode (every commitment against the context's SRS):
// the bases never change, so k_msm_fixed_table precomputes
// T[w*N + i] = 2^(c*w) * P_i once per window size c.  k_msm_digits_fixed
// then writes key = poly<<c | magnitude and val = sign<<31 | (w*N + i): all
// W digits of a polynomial share ONE bucket set (key group = poly), the
// sort covers c + ceil(log2(B+1)) bits, bucket_reduce gathers from the
// table, stages 4-5 see B groups instead of B*W, and the host Horner fold
// disappears.  c comes from msm_fixed_c (cost-based; no top-window rule).
// The variable-base pipeline above is unchanged and still serves
// caller-supplied bases (rng_msm_g1*), RNG_MSM_FIXED=0 and window sizes with
// no table.
//
// Direct-lookup mode (dense SRS commitments): one step further,
// k_msm_lookup_table stores every digit multiple
// L[((w*N + i) << (c-1)) + d-1] = d * 2^(c*w) * P_i, d = 1..2^(c-1), built
// from T for the same c, and k_msm_lookup_sum adds the n*W looked-up points
// of a polynomial with their signs: no keys, no sort, no buckets, no
// aggregation, one partial per 256-lane block, folded on the host.  The add
// count is the bucket pipeline's n*W(c); the cost is W*N*2^(c-1)*64 B of
// device memory behind a byte budget (msm_lookup_table in prover_api.hip),
// c in {8, 9, 10}.  Every fixed-base path cuts a scalar with the one
// msm_recode_digit of msm_digits.hpp.  The compacted Lagrange round, a
// context whose table does not fit, and RNG_MSM_LOOKUP=0 keep the buckets.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include "gpu_curve.hpp"
#include "msm_digits.hpp"

namespace rng {

// zero digits get the sentinel key (G << 16) — one past the last real
// group, so it sorts after every real (group<<16|mag) key while keeping the
// radix sort to 16 + ceil(log2(G+1)) bits (3 passes instead of 4 for every
// workload here)
__host__ __device__ inline uint32_t msm_sentinel(uint32_t G) { return G << 16; }
constexpr uint32_t MSM_CHUNK = 16;            // buckets per window-sum thread

// window size by problem size.  Besides balancing bucket-phase work
// (~ n*W(c)) against aggregation (~ W(c)*2^(c-1)), c must keep the TOP
// window well-populated: with 254-bit scalars the top window holds only
// 254-(W-1)*c significant bits, and when that is small every scalar's top
// digit lands in a handful of buckets — giant segments whose serial merge
// chains dominate (measured 3x slowdown at c=9/11 vs c=8 for n=4096).
// Top-window distinct digits D(c) = 2^(254-(W-1)*c): c=8 -> 64, c=13 -> 128,
// c=16 -> 2^14; those three tiers are the sweet spots.
__host__ __device__ inline uint32_t msm_auto_c(uint64_t n) {
    if (n <= (1ull << 16)) return 8;
    if (n <= (1ull << 18)) return 13;
    return 16;
}

// ---- 1. digit decomposition ----
// scalars: canonical LE 4xu64. keys/vals: n*W entries, window-major
// (out[w*n + i]) so writes coalesce per window.
// B polys of n scalars each share one base array; digits of poly b window w
// go to key group g = b*W + w so one sort/reduce handles the whole batch.
__global__ __launch_bounds__(256) void k_msm_digits(const uint64_t* scalars, uint32_t n, uint32_t c,
                             uint32_t W, uint32_t B, uint32_t* keys, uint32_t* vals) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * B) return;
    uint32_t b = idx / n, i = idx % n;
    uint64_t s[4];
    s[0] = scalars[4 * idx];
    s[1] = scalars[4 * idx + 1];
    s[2] = scalars[4 * idx + 2];
    s[3] = scalars[4 * idx + 3];
    uint32_t carry = 0;
    uint32_t half = 1u << (c - 1);
    uint64_t cmask = (c == 64) ? ~0ull : ((1ull << c) - 1);
    for (uint32_t w = 0; w < W; ++w) {
        uint32_t bit0 = w * c;
        uint32_t limb = bit0 >> 6, off = bit0 & 63;
        uint64_t raw = s[limb] >> off;
        if (off + c > 64 && limb + 1 < 4) raw |= s[limb + 1] << (64 - off);
        raw = (raw & cmask) + carry;
        uint32_t mag, sign;
        if (raw >= half) {  // treat as negative digit raw - 2^c unless raw == half
            if (raw > half) {
                mag = (uint32_t)((1ull << c) - raw);
                sign = 1;
                carry = 1;
            } else {  // raw == half: use +half, no carry (mag fits 16 bits for c<=16)
                mag = half;
                sign = 0;
                carry = 0;
            }
        } else {
            mag = (uint32_t)raw;
            sign = 0;
            carry = 0;
        }
        uint64_t o = ((uint64_t)b * W + w) * n + i;
        keys[o] = mag == 0 ? msm_sentinel(B * W) : (((b * W + w) << 16) | mag);
        vals[o] = (sign << 31) | i;
    }
    // carry out of the top window must be zero for scalars < 2^(W*c-1)
}

// ---- 1-fixed. fixed-base mode (SRS commitments) ----
// The SRS never changes for the life of a context, so the window weights
// 2^(c*w) are folded into a precomputed table T[w*N + i] = 2^(c*w) * P_i.
// Every digit of a scalar then indexes its own table point and ALL W digits
// of a polynomial fall into ONE bucket set: key group = poly, W times fewer
// buckets, no per-window aggregation and no host Horner fold.

// window size on the fixed-base path, by per-poly point count n and batch B.
// There is no separate top window here (all windows share one bucket set),
// so the {8,13,16} "populated top window" rule of msm_auto_c does not apply
// and c is chosen by cost: n*W(c) mixed adds + ~2*2^(c-1) aggregation adds
// per poly.  What still matters is the bucket COUNT B*2^(c-1): a bucket
// holds n*W/2^(c-1) entries, and its sub-segment partials are merged by one
// lane, so few big buckets mean a long serial chain.  Measured on MI355X
// (DESIGN §4.1): c=10 wins the fused cohort rounds at the settlement size;
// small batches (single proofs, preprocessing, link proofs) and the large
// domains keep c=13, whose bucket count equals the windowed path's at c=8.
// At most three values, so at most three tables per context.
__host__ __device__ inline uint32_t msm_fixed_c(uint64_t n, uint32_t B) {
    if (n <= (1ull << 8)) return 8;
    if (B >= 16 && n < (1ull << 13)) return 10;
    return 13;
}

constexpr uint32_t MSM_FIXED_MAX_W = 32;  // W(c) = ceil(256/c) <= 32 for c >= 8

// table build: one thread per base walks its W windows (c Jacobian
// doublings each), parks (X, Y) in the table slot, then normalises all W
// points with ONE field inversion (Montgomery batch inversion over the
// thread's own Z values).  Bases have prime order, so no multiple is the
// identity and every Z is invertible.
__global__ __launch_bounds__(256) void k_msm_fixed_table(const G1Aff* bases, uint32_t N,
                                                         uint32_t c, uint32_t W,
                                                         G1Aff* table) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    Fq zs[MSM_FIXED_MAX_W], pref[MSM_FIXED_MAX_W];  // pref[j] = Z_0 * ... * Z_j
    G1Jac acc = G1Jac::from_affine(bases[i]);
    Fq run = Fq::one();
    for (uint32_t j = 0; j < W; ++j) {
        if (j)
            for (uint32_t k = 0; k < c; ++k) acc = acc.dbl();
        G1Aff parked;
        parked.x = acc.X;
        parked.y = acc.Y;
        table[(uint64_t)j * N + i] = parked;
        zs[j] = acc.Z;
        run = run.mul(acc.Z);
        pref[j] = run;
    }
    Fq inv = run.inverse();  // 1 / (Z_0 * ... * Z_{W-1})
    for (int j = (int)W - 1; j >= 0; --j) {
        Fq zinv = j ? inv.mul(pref[j - 1]) : inv;
        inv = inv.mul(zs[j]);
        Fq zinv2 = zinv.sqr();
        G1Aff p = table[(uint64_t)j * N + i];
        p.x = p.x.mul(zinv2);
        p.y = p.y.mul(zinv2.mul(zinv));
        table[(uint64_t)j * N + i] = p;
    }
}

// digits for the fixed-base mode: key = poly << c | magnitude (the magnitude
// reaches 2^(c-1) inclusive, so it needs c bits), val = sign << 31 | table
// index w*N + i.  Zero digits get the sentinel B << c.
__global__ __launch_bounds__(256) void k_msm_digits_fixed(const uint64_t* scalars,
                                                          uint32_t n, uint32_t c,
                                                          uint32_t W, uint32_t B,
                                                          uint32_t N, uint32_t* keys,
                                                          uint32_t* vals) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * B) return;
    uint32_t b = idx / n, i = idx % n;
    uint64_t s[4];
    s[0] = scalars[4 * idx];
    s[1] = scalars[4 * idx + 1];
    s[2] = scalars[4 * idx + 2];
    s[3] = scalars[4 * idx + 3];
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; ++w) {
        MsmDigit d = msm_recode_digit(s, c, w, carry);
        uint64_t o = ((uint64_t)b * W + w) * n + i;
        keys[o] = d.mag == 0 ? (B << c) : ((b << c) | d.mag);
        vals[o] = (d.sign << 31) | (w * N + i);
    }
    // carry out of the top window is zero: scalars < 2^254 <= 2^(W*c-1)
}

// ---- 3a. segment-head flags (for stream compaction) ----
__global__ void k_msm_head_flags(const uint32_t* keys, uint32_t total, uint32_t sentinel,
                                 uint8_t* flags) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    uint32_t key = keys[t];
    flags[t] = (key != sentinel && (t == 0 || keys[t - 1] != key)) ? 1 : 0;
}

// Segment walks are capped at MSM_MAX_SEG entries: skewed digit
// distributions (the top window of <2^253 scalars, duplicate scalars) create
// segments thousands of entries long, and a single lane walking one is the
// whole kernel's critical path.  Long segments are split into sub-segments
// reduced in parallel, then merged per segment.
constexpr uint32_t MSM_MAX_SEG = 128;

// choose the sub-segment cap so the reduce kernel has >= ~64K lanes in
// flight (256 CUs want >> 256 workgroups); smaller caps cost extra merge
// work, so keep within [8, MSM_MAX_SEG]
__host__ inline uint32_t msm_seg_cap(uint64_t total_entries) {
    uint64_t cap = total_entries / (1u << 16);
    if (cap < 8) cap = 8;  // scratch sizes subs as total/8 — keep min 8
    if (cap > MSM_MAX_SEG) cap = MSM_MAX_SEG;
    return (uint32_t)cap;
}

// Cap on the compacted (Lagrange) path.  Its entries are few and skewed: a
// settlement wire poly puts ~460 values equal to 1 into ONE bucket while the
// other buckets hold a handful each.  msm_seg_cap of the real count gives 8,
// and one k_msm_seg_merge lane then chains ~58 Jacobian adds; a cap of L
// costs about L mixed adds in the reduce lane plus len/L adds in the merge
// lane, minimal near sqrt(len) ~ 21-32 for that bucket.  Measured at the
// settlement cohort shape, caps 8..128: 32 is the fastest.
// Dense inputs on this path keep msm_seg_cap's larger value.
constexpr uint32_t MSM_COMPACT_SEG_CAP = 32;
__host__ inline uint32_t msm_compact_seg_cap(uint64_t entries) {
    uint32_t cap = msm_seg_cap(entries);
    return cap < MSM_COMPACT_SEG_CAP ? MSM_COMPACT_SEG_CAP : cap;
}

// ---- 3b. segment lengths + sub-segment counts ----
// heads are in increasing order (rocprim::select is stable); seg i spans
// [heads[i], heads[i+1] or first sentinel/total).
__global__ void k_msm_seg_lengths(const uint32_t* keys, const uint32_t* heads,
                                  const uint32_t* head_count, uint32_t total,
                                  uint32_t* lens, uint32_t* nsub, uint32_t seg_cap) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t hc = *head_count;
    if (t >= hc) return;
    uint32_t start = heads[t];
    uint32_t end = (t + 1 < hc) ? heads[t + 1] : total;
    // sentinel tail: the zero-digit entries sort after every real key, and
    // the last real segment's end must exclude them
    if (t + 1 == hc) {
        uint32_t key = keys[start];
        uint32_t e = start;
        while (e < total && keys[e] == key) ++e;
        end = e;
    }
    uint32_t len = end - start;
    lens[t] = len;
    nsub[t] = (len + seg_cap - 1) / seg_cap;
}

// ---- 3c. emit sub-segment records (after exclusive scan of nsub) ----
// subs: per sub-segment (start, len, head index)
__global__ void k_msm_make_subs(const uint32_t* heads, const uint32_t* lens,
                                const uint32_t* sub_off, const uint32_t* head_count,
                                uint32_t* sub_start, uint32_t* sub_len,
                                uint32_t seg_cap) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= *head_count) return;
    uint32_t start = heads[t], len = lens[t], off = sub_off[t];
    uint32_t k = 0;
    while (len > 0) {
        uint32_t l = len < seg_cap ? len : seg_cap;
        sub_start[off + k] = start;
        sub_len[off + k] = l;
        start += l;
        len -= l;
        ++k;
    }
}

// ---- 3d. sub-segment reduction: one thread per sub-segment (<= MAX_SEG) ----
__global__ __launch_bounds__(256) void k_msm_bucket_reduce(
    const uint32_t* vals, const uint32_t* sub_start, const uint32_t* sub_len,
    const uint32_t* sub_order /* sub ids sorted by length desc */,
    uint32_t sub_count, const G1Aff* bases, G1Jac* partials2) {
    uint32_t tt = blockIdx.x * blockDim.x + threadIdx.x;
    if (tt >= sub_count) return;
    uint32_t t = sub_order[tt];
    uint32_t start = sub_start[t], len = sub_len[t];
    // NOTE on ILP: a two-accumulator interleave was tried and reverted —
    // the v_mad_u64_u32 hazard s_nops it targets come from VCC carry
    // serialization, which BOTH chains share, so it only added an extra EC
    // add per sub-segment; the hazard slots are instead covered by running
    // 16 concurrent proof streams.
    G1Jac acc = G1Jac::identity();
    for (uint32_t j = start; j < start + len; ++j) {
        uint32_t v = vals[j];
        G1Aff p = bases[v & 0x7FFFFFFFu];
        acc = acc.madd(p, (v >> 31) != 0);
    }
    partials2[t] = acc;
}

// ---- 3e. merge sub-partials per segment -> bucket ----
// buckets: W * 2^(c-1) Jacobian points (zero-init = identity for untouched).
__global__ __launch_bounds__(256) void k_msm_seg_merge(
    const uint32_t* keys, const uint32_t* heads, const uint32_t* sub_off,
    const uint32_t* nsub, const uint32_t* head_order /* by nsub desc */,
    uint32_t head_count, const G1Jac* partials2,
    G1Jac* buckets, uint32_t c, uint32_t key_shift /* 16, or c in fixed-base mode */) {
    uint32_t tt = blockIdx.x * blockDim.x + threadIdx.x;
    if (tt >= head_count) return;
    uint32_t t = head_order[tt];
    uint32_t off = sub_off[t], ns = nsub[t];
    G1Jac acc = partials2[off];
    for (uint32_t k = 1; k < ns; ++k) acc = acc.add(partials2[off + k]);
    uint32_t key = keys[heads[t]];
    uint32_t w = key >> key_shift;
    uint32_t mag = key & ((1u << key_shift) - 1);  // 1 .. 2^(c-1)
    buckets[(uint64_t)w * (1u << (c - 1)) + (mag - 1)] = acc;
}

// ---- 4. per-window chunked suffix sums ----
// grid: W * (2^(c-1) / MSM_CHUNK) threads total; partials: per thread
// (T = plain sum, S = locally-weighted sum) -> 2 Jacobians.
__global__ __launch_bounds__(256) void k_msm_window_chunks(const G1Jac* buckets, uint32_t c, uint32_t W,
                                    uint32_t chunk_sz,
                                    G1Jac* partials /* 2 per thread: T, S */) {
    uint32_t nb = 1u << (c - 1);
    uint32_t chunks_per_w = nb / chunk_sz;
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= W * chunks_per_w) return;
    uint32_t w = t / chunks_per_w;
    uint32_t chunk = t % chunks_per_w;
    const G1Jac* b = buckets + (uint64_t)w * nb + (uint64_t)chunk * chunk_sz;
    // local digits are base + j, j = 1..chunk_sz, base = chunk*chunk_sz
    // suffix running sums over j descending: run = sum_{k>=j} S_k ; S += run
    G1Jac run = G1Jac::identity(), S = G1Jac::identity();
    for (int j = (int)chunk_sz - 1; j >= 0; --j) {
        run = run.add(b[j]);
        S = S.add(run);
    }
    partials[2 * t] = run;  // T = plain sum of chunk buckets
    partials[2 * t + 1] = S;  // sum_j (j_local) * bucket, j_local = 1..chunk_sz
}

// ---- 5a. window combine: grid = W * MSM_SUBB blocks; block (w, sb) folds a
// slice of window w's chunk partials (contribution = S + base*T with
// base = chunk*CHUNK), LDS tree reduce -> window_partials[w*SUBB + sb].
constexpr uint32_t MSM_SUBB = 16;

__global__ __launch_bounds__(64) void k_msm_window_combine(const G1Jac* partials,
                                                           uint32_t c,
                                                           uint32_t chunk_sz,
                                                           uint32_t subb,
                                                           G1Jac* window_partials) {
    __shared__ G1Jac red[64];
    uint32_t w = blockIdx.x / subb;
    uint32_t sb = blockIdx.x % subb;
    uint32_t nb = 1u << (c - 1);
    uint32_t chunks_per_w = nb / chunk_sz;
    uint32_t per_sb = (chunks_per_w + subb - 1) / subb;
    uint32_t lo = sb * per_sb;
    uint32_t hi = lo + per_sb < chunks_per_w ? lo + per_sb : chunks_per_w;
    G1Jac acc = G1Jac::identity();
    for (uint32_t chunk = lo + threadIdx.x; chunk < hi; chunk += blockDim.x) {
        uint32_t t = w * chunks_per_w + chunk;
        G1Jac T = partials[2 * t];
        G1Jac S = partials[2 * t + 1];
        uint32_t base = chunk * chunk_sz;
        G1Jac bT = G1Jac::identity();
        G1Jac addend = T;
        while (base) {
            if (base & 1) bT = bT.add(addend);
            addend = addend.dbl();
            base >>= 1;
        }
        acc = acc.add(S).add(bT);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride)
            red[threadIdx.x] = red[threadIdx.x].add(red[threadIdx.x + stride]);
        __syncthreads();
    }
    if (threadIdx.x == 0) window_partials[w * subb + sb] = red[0];
}

// ---- 5b. scan-based combine (large windows): block (w, sb) folds P =
// chunks_per_window/subb chunk partials with NO per-chunk scalar weighting.
// Decompose the weighted sum over the block's chunk range [lo, lo+P):
//   sum_c (S_c + cz*c*T_c) = sum S + cz*( lo*At + pl*sum_l l*A_l
//                                         + sum_l (B_l - A_l) )
// where lane l serially folds pl = P/64 chunks into A_l = sum T,
// B_l = sum (j+1)*T (suffix-running trick), At = sum_l A_l, and
// sum_l l*A_l comes from one LDS suffix scan.  The only scalar weights
// left are the power-of-two lo and cz (a few doublings once per block) —
// replaces the per-chunk binary-doubling chains of k_msm_window_combine,
// which rocprof showed at 1.74 ms of the 6.2 ms 2^20 MSM.
__global__ __launch_bounds__(64) void k_msm_window_combine2(
    const G1Jac* partials, uint32_t c, uint32_t chunk_sz, uint32_t subb,
    G1Jac* window_partials) {
    __shared__ G1Jac sA[64], sB[64], sS[64];
    uint32_t w = blockIdx.x / subb;
    uint32_t sb = blockIdx.x % subb;
    uint32_t nb = 1u << (c - 1);
    uint32_t chunks_per_w = nb / chunk_sz;
    uint32_t P = chunks_per_w / subb;  // caller guarantees P >= 64
    uint32_t pl = P / 64;
    uint32_t lo = sb * P;
    uint32_t l = threadIdx.x;
    const G1Jac* base = partials + 2 * ((uint64_t)w * chunks_per_w + lo + l * pl);
    G1Jac A = G1Jac::identity(), B = G1Jac::identity(), S = G1Jac::identity();
    for (int j = (int)pl - 1; j >= 0; --j) {
        A = A.add(base[2 * j]);        // run += T_j
        B = B.add(A);                  // B = sum (j+1)*T_j
        S = S.add(base[2 * j + 1]);
    }
    // LDS suffix scan of A -> SufA_l = sum_{m>=l} A_m (ping-pong not needed:
    // Hillis-Steele with double buffer via barrier pairs)
    sA[l] = A;
    sB[l] = B;
    sS[l] = S;
    __syncthreads();
    for (uint32_t st = 1; st < 64; st <<= 1) {
        G1Jac v = sA[l];
        if (l + st < 64) v = v.add(sA[l + st]);
        __syncthreads();
        sA[l] = v;
        __syncthreads();
    }
    // At = SufA_0 (visible to all lanes); parallel trees for
    // lw = sum_{l>=1} SufA_l, Bt = sum B_l, St = sum S_l
    G1Jac At = sA[0];
    G1Jac tail = (l >= 1) ? sA[l] : G1Jac::identity();
    __syncthreads();
    sA[l] = tail;
    __syncthreads();
    for (uint32_t st = 32; st > 0; st >>= 1) {
        if (l < st) {
            sA[l] = sA[l].add(sA[l + st]);
            sB[l] = sB[l].add(sB[l + st]);
            sS[l] = sS[l].add(sS[l + st]);
        }
        __syncthreads();
    }
    if (l == 0) {
        G1Jac lw = sA[0], Bt = sB[0], St = sS[0];
        // weighted = lo*At + pl*lw + (Bt - At); lo has <=2 set bits
        G1Jac loAt = G1Jac::identity();
        {
            G1Jac addend = At;
            for (uint32_t rem = lo; rem; rem >>= 1) {
                if (rem & 1) loAt = loAt.add(addend);
                addend = addend.dbl();
            }
        }
        G1Jac plw = lw;
        for (uint32_t m = pl; m > 1; m >>= 1) plw = plw.dbl();
        G1Jac nAt = At;
        nAt.Y = nAt.Y.neg();  // Bt - At
        G1Jac weighted = loAt.add(plw).add(Bt).add(nAt);
        for (uint32_t m = chunk_sz; m > 1; m >>= 1) weighted = weighted.dbl();
        window_partials[blockIdx.x] = St.add(weighted);
    }
}

// (The final fold across windows — W*SUBB <= 512 Jacobians, ~1.5 KB — is
// done on the HOST: a single-lane dependent EC chain runs ~50x slower on a
// GPU SIMT lane than on a host core, and the data is tiny.)

// ---- direct-lookup fixed-base path ----
// The SRS is fixed for the life of a context, so the precomputation goes one
// step past the window table: every digit multiple of every table point,
//   L[((w*N + i) << (c-1)) + (d-1)] = d * 2^(c*w) * P_i,  d = 1 .. 2^(c-1),
// affine, 64 B each.  A commitment is then a plain signed sum of the n*W
// gathered points: nothing is sorted, bucketed or aggregated, and nothing is
// read back before the block partials.  Memory W*N*2^(c-1)*64 B, behind the
// budget of msm_lookup_table (prover_api.hip).

// entries normalised behind one field inversion; the two Fq arrays are what
// k_msm_fixed_table keeps per lane
constexpr uint32_t MSM_LOOKUP_BATCH = MSM_FIXED_MAX_W;
// window sizes with a lookup table; 2^(c-1) >= 128 is a multiple of the batch
constexpr uint32_t MSM_LOOKUP_MIN_C = 8, MSM_LOOKUP_MAX_C = 10;

// table build: one lane per row (w, i) of the window table `fixed` walks
// d = 1 .. 2^(c-1) by repeated mixed add of the row's point (d = 1 is the
// identity branch of madd, d = 2 its doubling branch), parks (X, Y) in the
// slot and normalises MSM_LOOKUP_BATCH entries at a time.  Bases have prime
// order r and d < r, so no multiple is the identity and every Z inverts.
__global__ __launch_bounds__(256) void k_msm_lookup_table(const G1Aff* fixed, uint64_t rows,
                                                          uint32_t c, G1Aff* table) {
    uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const uint32_t nd = 1u << (c - 1);
    const G1Aff P = fixed[r];
    G1Aff* row = table + (r << (c - 1));
    Fq zs[MSM_LOOKUP_BATCH], pref[MSM_LOOKUP_BATCH];  // pref[j] = Z_0 * ... * Z_j
    G1Jac acc = G1Jac::identity();
    for (uint32_t d0 = 0; d0 < nd; d0 += MSM_LOOKUP_BATCH) {
        Fq run = Fq::one();
        for (uint32_t j = 0; j < MSM_LOOKUP_BATCH; ++j) {
            acc = acc.madd(P);  // (d0 + j + 1) * P
            G1Aff parked;
            parked.x = acc.X;
            parked.y = acc.Y;
            row[d0 + j] = parked;
            zs[j] = acc.Z;
            run = run.mul(acc.Z);
            pref[j] = run;
        }
        Fq inv = run.inverse();
        for (int j = (int)MSM_LOOKUP_BATCH - 1; j >= 0; --j) {
            Fq zinv = j ? inv.mul(pref[j - 1]) : inv;
            inv = inv.mul(zs[j]);
            Fq zinv2 = zinv.sqr();
            G1Aff p = row[d0 + j];
            p.x = p.x.mul(zinv2);
            p.y = p.y.mul(zinv2.mul(zinv));
            row[d0 + j] = p;
        }
    }
}

// the sum: grid (blocks per poly, B), 256 lanes; lane t of block x takes the
// scalars i = (x*per_lane + l)*256 + t, l < per_lane, of poly blockIdx.y
// (coalesced, never across polynomials), recodes each in registers and adds
// the looked-up multiples into one Jacobian.  The block folds its 256
// accumulators through LDS with the full add (equal and opposite operands
// meet here and in madd; both handle them) and writes ONE partial:
// partials[poly * gridDim.x + x].
__global__ __launch_bounds__(256) void k_msm_lookup_sum(const uint64_t* scalars, uint32_t n,
                                                        uint32_t c, uint32_t W, uint32_t N,
                                                        uint32_t per_lane, const G1Aff* table,
                                                        G1Jac* partials) {
    __shared__ G1Jac red[256];
    // the scalar being cut lives in the lane's own LDS row, not in registers:
    // with its 8 VGPRs live across madd the loop needs 176 VGPRs (2 waves per
    // SIMD), without them 167 (3 waves), and the recoding's limb index
    // becomes an address instead of a select chain
    __shared__ uint64_t sc[256][4];
    const uint32_t b = blockIdx.y;
    const uint32_t first = blockIdx.x * per_lane * 256 + threadIdx.x;
    uint64_t* s = sc[threadIdx.x];
    const uint64_t wstride = (uint64_t)N << (c - 1);  // entries per window
    G1Jac acc = G1Jac::identity();
    for (uint32_t l = 0; l < per_lane; ++l) {
        const uint32_t i = first + l * 256;
        if (i >= n) break;
        const uint64_t* sp = scalars + 4 * ((uint64_t)b * n + i);
        const uint64_t s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
        if (!(s0 | s1 | s2 | s3)) continue;
        s[0] = s0;
        s[1] = s1;
        s[2] = s2;
        s[3] = s3;
        const G1Aff* row = table + ((uint64_t)i << (c - 1));  // L[w = 0][i][.]
        uint32_t carry = 0;
        for (uint32_t w = 0; w < W; ++w, row += wstride) {
            const MsmDigit d = msm_recode_digit(s, c, w, carry);
            if (d.mag == 0) continue;
            const G1Aff p = row[d.mag - 1];
            acc = acc.madd(p, d.sign != 0);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t stride = 128; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride)
            red[threadIdx.x] = red[threadIdx.x].add(red[threadIdx.x + stride]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[(uint64_t)b * gridDim.x + blockIdx.x] = red[0];
}

// ---- helpers ----
__global__ void k_fr_to_canonical(const Fr* in, uint64_t* out, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    in[i].to_canonical(out + 4 * i);
}

}  // namespace rng
