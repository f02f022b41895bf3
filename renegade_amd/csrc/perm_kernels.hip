// PRODUCT PATH — PlonK permutation grand product z(X) on gfx950.
//
// For proof p and row t (w = the n-th root of unity, k_j the coset
// representatives, sigma the key's permutation evaluations):
//   num_p(t) = prod_{j<5} ( w_p[j][t] + beta_p k_j w^t      + gamma_p )
//   den_p(t) = prod_{j<5} ( w_p[j][t] + beta_p sigma[j][t]  + gamma_p )
//   z_p[0] = 1,  z_p[i] = prod_{t<i} num_p(t) / den_p(t)
// No per-row inversion: with P the inclusive prefix product of num, S the
// inclusive suffix product of den and Q = S_0,
//   z_i = P_{i-1} * S_i * Q^-1        (1 <= i < n),
// so the stage is a term kernel, a batched product scan over 2*batch
// sequences (sequence s < batch: num of proof s, scanned forward;
// s >= batch: den of proof s - batch, scanned backward), `batch` inversions
// of Q (host side, prover_api.hip) and a finalize kernel.  A zero
// denominator gives Q = 0, Q^-1 = 0 (Fermat) and z_i = 0 for i >= 1, the
// host loop's batch-inverse semantics; z_0 is written as the constant 1.
//
// Scan tiling: a workgroup of PERM_WG threads owns a tile of PERM_TILE =
// PERM_WG * PERM_EPT consecutive scan positions; thread t holds positions
// t*PERM_EPT .. t*PERM_EPT + PERM_EPT-1 in named registers (static indices
// only), runs them serially, the PERM_WG partials go through a
// Hillis-Steele scan in LDS, and the apply step multiplies the thread's
// exclusive prefix back in.  n <= PERM_TILE is one pass (k_perm_scan_apply
// without carry).  Longer sequences take three launches: k_perm_tile_reduce
// (tile totals), k_perm_tile_prefix (one workgroup per sequence scans its
// <= PERM_MAX_TILES totals) and k_perm_scan_apply with the tile's carry.
// No kernel waits on another workgroup; the dependent depth per sequence is
// about 3 * (PERM_EPT + log2 PERM_WG) multiplications for any n.
#include <hip/hip_runtime.h>
#include "gpu_field.hpp"

namespace rng {

constexpr uint32_t PERM_WG = 256;
constexpr uint32_t PERM_EPT = 4;
constexpr uint32_t PERM_TILE = PERM_WG * PERM_EPT;  // 1024
constexpr uint32_t PERM_MAX_N = 1u << 17;           // SRS cap
constexpr uint32_t PERM_MAX_TILES = PERM_MAX_N / PERM_TILE;  // 128
constexpr uint32_t PERM_MAX_BATCH = 128;

struct PermK5 {  // coset representatives (kernel arg)
    Fr k[5];
};

// One thread per (proof, row): num into nd[p*n + t], den into
// nd[(batch + p)*n + t].  wires = batch x 5 x n, sigma = 5 x n, wpow[t] = w^t,
// bg = batch x (beta, gamma).
__global__ __launch_bounds__(256) void k_perm_terms(
    const Fr* wires, const Fr* sigma, const Fr* wpow, const Fr* bg, PermK5 k5,
    Fr* nd, uint32_t n, uint32_t batch) {
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (uint64_t)batch * n) return;
    uint32_t p = (uint32_t)(tid / n);
    uint32_t t = (uint32_t)(tid - (uint64_t)p * n);
    Fr beta = bg[2 * p], gamma = bg[2 * p + 1];
    const Fr* w = wires + 5 * (uint64_t)p * n;
    Fr bx = beta.mul(wpow[t]);
    Fr num = Fr::one(), den = Fr::one();
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        Fr wg = w[(uint64_t)j * n + t].add(gamma);
        Fr f = wg.add(bx.mul(k5.k[j]));
        Fr g = wg.add(beta.mul(sigma[(uint64_t)j * n + t]));
        num = (j == 0) ? f : num.mul(f);
        den = (j == 0) ? g : den.mul(g);
    }
    nd[(uint64_t)p * n + t] = num;
    nd[((uint64_t)batch + p) * n + t] = den;
}

// scan position -> element index: forward for num, backward for den
__device__ __forceinline__ uint32_t perm_phys(uint32_t pos, uint32_t n, bool rev) {
    return rev ? n - 1 - pos : pos;
}

// inclusive Hillis-Steele product scan of PERM_WG values (one per thread)
// through two LDS buffers; returns this thread's inclusive value.  The
// buffers swap log2(PERM_WG) = 8 times, so sh[0] ends up holding every
// thread's inclusive value.
__device__ __forceinline__ Fr perm_wg_scan(Fr v, Fr (*sh)[PERM_WG]) {
    static_assert(PERM_WG == 256, "an even number of scan steps leaves the result in sh[0]");
    const uint32_t t = threadIdx.x;
    uint32_t cur = 0;
    sh[0][t] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < PERM_WG; d <<= 1) {
        if (t >= d) v = sh[cur][t - d].mul(v);
        sh[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    return v;
}

// product of one tile: grid = nseq * tiles blocks, tile_tot[block]
__global__ __launch_bounds__(PERM_WG) void k_perm_tile_reduce(
    const Fr* nd, Fr* tile_tot, uint32_t n, uint32_t tiles, uint32_t batch) {
    __shared__ Fr sh[PERM_WG];
    const uint32_t seq = blockIdx.x / tiles, tile = blockIdx.x - seq * tiles;
    const bool rev = seq >= batch;
    const Fr* src = nd + (uint64_t)seq * n;
    const uint32_t pos0 = tile * PERM_TILE + threadIdx.x * PERM_EPT;
    Fr acc = Fr::one();
#pragma unroll
    for (uint32_t e = 0; e < PERM_EPT; ++e) {
        uint32_t pos = pos0 + e;
        if (pos < n) {
            Fr v = src[perm_phys(pos, n, rev)];
            acc = (e == 0) ? v : acc.mul(v);
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (uint32_t d = PERM_WG / 2; d >= 1; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] = sh[threadIdx.x].mul(sh[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_tot[blockIdx.x] = sh[0];
}

// one workgroup per sequence: exclusive scan of its tile totals into
// tile_pre, sequence total into totals[seq].  tiles <= PERM_MAX_TILES <= PERM_WG.
__global__ __launch_bounds__(PERM_WG) void k_perm_tile_prefix(
    const Fr* tile_tot, Fr* tile_pre, Fr* totals, uint32_t tiles) {
    __shared__ Fr sh[2][PERM_WG];
    const uint32_t seq = blockIdx.x, t = threadIdx.x;
    Fr v = (t < tiles) ? tile_tot[(uint64_t)seq * tiles + t] : Fr::one();
    Fr inc = perm_wg_scan(v, sh);
    if (t < tiles) tile_pre[(uint64_t)seq * tiles + t] = (t == 0) ? Fr::one() : sh[0][t - 1];
    if (t == tiles - 1) totals[seq] = inc;
}

// in-place inclusive scan of one tile.  CARRY: multiply in the tile's
// exclusive prefix from k_perm_tile_prefix (multi-tile sequences); without
// it the sequence is the single tile and its total goes to totals[seq].
template <bool CARRY>
__global__ __launch_bounds__(PERM_WG) void k_perm_scan_apply(
    Fr* nd, const Fr* tile_pre, Fr* totals, uint32_t n, uint32_t tiles, uint32_t batch) {
    __shared__ Fr sh[2][PERM_WG];
    const uint32_t seq = blockIdx.x / tiles, tile = blockIdx.x - seq * tiles;
    const bool rev = seq >= batch;
    Fr* seqp = nd + (uint64_t)seq * n;
    const uint32_t t = threadIdx.x;
    const uint32_t pos0 = tile * PERM_TILE + t * PERM_EPT;
    static_assert(PERM_EPT == 4, "named registers below");
    Fr v0 = Fr::one(), v1 = Fr::one(), v2 = Fr::one(), v3 = Fr::one();
    if (pos0 + 0 < n) v0 = seqp[perm_phys(pos0 + 0, n, rev)];
    if (pos0 + 1 < n) v1 = seqp[perm_phys(pos0 + 1, n, rev)];
    if (pos0 + 2 < n) v2 = seqp[perm_phys(pos0 + 2, n, rev)];
    if (pos0 + 3 < n) v3 = seqp[perm_phys(pos0 + 3, n, rev)];
    v1 = v0.mul(v1);
    v2 = v1.mul(v2);
    v3 = v2.mul(v3);
    Fr inc = perm_wg_scan(v3, sh);
    // exclusive prefix of this thread = inclusive value of thread t-1
    Fr ex = (t == 0) ? Fr::one() : sh[0][t - 1];
    bool has_ex = t != 0;
    if (CARRY) {
        Fr c = tile_pre[blockIdx.x];
        ex = has_ex ? ex.mul(c) : c;
        has_ex = true;
    }
    if (has_ex) {
        v0 = ex.mul(v0);
        v1 = ex.mul(v1);
        v2 = ex.mul(v2);
        v3 = ex.mul(v3);
    }
    if (pos0 + 0 < n) seqp[perm_phys(pos0 + 0, n, rev)] = v0;
    if (pos0 + 1 < n) seqp[perm_phys(pos0 + 1, n, rev)] = v1;
    if (pos0 + 2 < n) seqp[perm_phys(pos0 + 2, n, rev)] = v2;
    if (pos0 + 3 < n) seqp[perm_phys(pos0 + 3, n, rev)] = v3;
    if (!CARRY && t == PERM_WG - 1) totals[seq] = inc;
}

// z_p[0] = 1, z_p[i] = P_{i-1} * S_i * Q^-1.  nd holds the scanned
// sequences (P of proof p at nd[p*n], S at nd[(batch+p)*n]).
__global__ __launch_bounds__(256) void k_perm_finalize(const Fr* nd, const Fr* qinv,
                                                       Fr* z, uint32_t n,
                                                       uint32_t batch) {
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (uint64_t)batch * n) return;
    uint32_t p = (uint32_t)(tid / n);
    uint32_t i = (uint32_t)(tid - (uint64_t)p * n);
    Fr out = Fr::one();
    if (i != 0) {
        Fr pre = nd[(uint64_t)p * n + i - 1];
        Fr suf = nd[((uint64_t)batch + p) * n + i];
        out = pre.mul(suf).mul(qinv[p]);
    }
    z[tid] = out;
}

}  // namespace rng
