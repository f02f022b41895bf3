// PRODUCT PATH — PlonK rounds 4 and 5 on gfx950: evaluations at zeta, the
// batched opening polynomial and the two opening quotients.
//
// One primitive, the batched Horner scan.  For coefficients c[0..len) and a
// point x let S[i] = sum_{j>=i} c[j] x^(j-i), i.e. S[i] = c[i] + x S[i+1].
//   S[0]              = c(x)                       (reduce mode)
//   S[1] .. S[len-1]  = c(X) / (X - x), remainder dropped   (scan mode)
// which are hpoly_eval and hpoly_div_linear of plonk_host.hpp.  No inverse
// of x appears anywhere, so x = 0 and x = 1 are ordinary points.
//
// Tiling (as perm_kernels.hip): a workgroup of OPEN_WG threads owns a tile
// of OPEN_TILE = OPEN_WG * OPEN_EPT consecutive positions; thread t holds
// positions 4t .. 4t+3 of the tile in named registers, folds them with a
// 3-mul Horner into h_t = S restricted to its own four coefficients, and a
// Hillis-Steele suffix pass in LDS turns h into S at every thread's first
// position: step s adds x^(4*2^s) times the value 2^s threads up, the
// multiplier is uniform and squared between steps.  Coefficients at or above
// len read as zero, which changes no S.  A sequence longer than one tile
// takes three launches: k_open_horner_tile<false,false> (tile totals),
// k_open_tile_prefix (one workgroup per sequence: the same suffix pass over
// the totals with multiplier x^OPEN_TILE; total j becomes the carry
// S[(j+1)*OPEN_TILE] of tile j, S[0] the evaluation) and
// k_open_horner_tile<true,true>, which folds x^4 * carry into the last
// thread's h before the pass.  No kernel waits on another workgroup.
//
// Sequences are addressed as batch x group: item b has one point, shared by
// its `group` polynomials, which are per item or (item_stride = 0) shared
// by all items.
#include <hip/hip_runtime.h>
#include "gpu_field.hpp"

namespace rng {

constexpr uint32_t OPEN_WG = 256;
constexpr uint32_t OPEN_EPT = 4;
constexpr uint32_t OPEN_TILE = OPEN_WG * OPEN_EPT;           // 1024
constexpr uint32_t OPEN_MAX_N = 1u << 17;                    // SRS cap
constexpr uint32_t OPEN_MAX_LEN = OPEN_MAX_N + 3;            // z and chunk length at the cap
constexpr uint32_t OPEN_MAX_TILES = (OPEN_MAX_LEN + OPEN_TILE - 1) / OPEN_TILE;  // 129
constexpr uint32_t OPEN_MAX_SEQ = 640;                       // batch * group per call
constexpr uint32_t OPEN_MAX_BATCH = 128;                     // proofs per stage call
constexpr uint32_t OPEN_TERMS = 29;                          // polynomials in C (open_scalars)
static_assert(OPEN_MAX_TILES <= OPEN_WG, "k_open_tile_prefix holds one total per thread");
static_assert(OPEN_MAX_SEQ >= 5 * OPEN_MAX_BATCH, "the wire evaluations of a full cohort");

struct OpenSeqs {  // one batched call (kernel arg); strides in Fr
    const Fr* src;
    uint64_t item_stride, poly_stride;  // sequence (b, g) at src + b*item_stride + g*poly_stride
    const Fr* pts;
    uint32_t pt_stride;                 // point of item b at pts[b*pt_stride]
    uint32_t len, group, tiles;
    Fr* out;                            // scan mode: (b, g) at out + b*out_item_stride + g*out_poly_stride
    uint64_t out_item_stride, out_poly_stride;
};

// suffix pass over OPEN_WG values (one per thread): returns
// sum_{u >= t} v_u m^(u-t).  The buffers swap log2(OPEN_WG) = 8 times, so
// sh[0] ends up holding every thread's result.
__device__ __forceinline__ Fr open_wg_suffix(Fr v, Fr m, Fr (*sh)[OPEN_WG]) {
    static_assert(OPEN_WG == 256, "an even number of steps leaves the result in sh[0]");
    const uint32_t t = threadIdx.x;
    uint32_t cur = 0;
    sh[0][t] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < OPEN_WG; d <<= 1) {
        if (t + d < OPEN_WG) v = v.add(m.mul(sh[cur][t + d]));
        sh[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
        m = m.sqr();
    }
    return v;
}

// One tile of one sequence; grid = nseq * tiles blocks.
//   <false,false>: tile_io[block] = the tile's own total (for a single tile:
//                  the evaluation, block == sequence)
//   <false,true> : scan of a single-tile sequence
//   <true,true>  : scan with the carry tile_io[block] from k_open_tile_prefix
template <bool CARRY, bool SCAN>
__global__ __launch_bounds__(OPEN_WG) void k_open_horner_tile(OpenSeqs q, Fr* tile_io) {
    __shared__ Fr sh[2][OPEN_WG];
    const uint32_t seq = blockIdx.x / q.tiles, tile = blockIdx.x - seq * q.tiles;
    const uint32_t b = seq / q.group, g = seq - b * q.group;
    const Fr* c = q.src + b * q.item_stride + g * q.poly_stride;
    const Fr x = q.pts[(uint64_t)b * q.pt_stride];
    const uint32_t t = threadIdx.x;
    const uint32_t pos0 = tile * OPEN_TILE + t * OPEN_EPT;
    static_assert(OPEN_EPT == 4, "named registers below");
    Fr c0 = Fr::zero(), c1 = Fr::zero(), c2 = Fr::zero(), c3 = Fr::zero();
    if (pos0 + 0 < q.len) c0 = c[pos0 + 0];
    if (pos0 + 1 < q.len) c1 = c[pos0 + 1];
    if (pos0 + 2 < q.len) c2 = c[pos0 + 2];
    if (pos0 + 3 < q.len) c3 = c[pos0 + 3];
    const Fr x4 = x.sqr().sqr();
    Fr h = c0.add(x.mul(c1.add(x.mul(c2.add(x.mul(c3))))));
    Fr carry = Fr::zero();  // S at the first position after the tile
    if (CARRY) {
        carry = tile_io[blockIdx.x];
        if (t == OPEN_WG - 1) h = h.add(x4.mul(carry));
    }
    const Fr s0 = open_wg_suffix(h, x4, sh);  // S[pos0]
    if (!SCAN) {
        if (t == 0) tile_io[blockIdx.x] = s0;
        return;
    }
    const Fr up = (t == OPEN_WG - 1) ? carry : sh[0][t + 1];  // S[pos0 + 4]
    const Fr s3 = c3.add(x.mul(up));
    const Fr s2 = c2.add(x.mul(s3));
    const Fr s1 = c1.add(x.mul(s2));
    // quotient coefficient i - 1 is S[i], 1 <= i < len
    Fr* o = q.out + b * q.out_item_stride + g * q.out_poly_stride;
    if (pos0 >= 1 && pos0 < q.len) o[pos0 - 1] = s0;
    if (pos0 + 1 < q.len) o[pos0] = s1;
    if (pos0 + 2 < q.len) o[pos0 + 1] = s2;
    if (pos0 + 3 < q.len) o[pos0 + 2] = s3;
}

// One workgroup per sequence folds its tile totals with Horner in
// x^OPEN_TILE.  In place: total j is replaced by tile j's carry (zero for
// the last tile); the evaluation goes to evals[seq] when evals is given.
__global__ __launch_bounds__(OPEN_WG) void k_open_tile_prefix(
    const Fr* pts, uint32_t pt_stride, uint32_t group, uint32_t tiles, Fr* tile_io,
    Fr* evals) {
    __shared__ Fr sh[2][OPEN_WG];
    const uint32_t seq = blockIdx.x, t = threadIdx.x;
    Fr y = pts[(uint64_t)(seq / group) * pt_stride];
    static_assert(OPEN_TILE == 1024, "ten squarings below");
    for (int i = 0; i < 10; ++i) y = y.sqr();
    Fr v = (t < tiles) ? tile_io[(uint64_t)seq * tiles + t] : Fr::zero();
    const Fr s = open_wg_suffix(v, y, sh);
    if (t < tiles)
        tile_io[(uint64_t)seq * tiles + t] = (t + 1 < tiles) ? sh[0][t + 1] : Fr::zero();
    if (t == 0 && evals) evals[seq] = s;
}

struct OpenPolys {  // where the 29 polynomials of open_scalars live (kernel arg)
    const Fr* key;      // 18 x n: 13 selectors, 5 sigma (coefficients)
    const Fr* wz;       // proof p at wz + p*wz_item: wires 0..4 and z at stride n+3
    uint64_t wz_item;
    const Fr* chunks;   // proof p at chunks + p*ch_item: 5 chunks at stride n+3
    uint64_t ch_item;
};

// C_p[i] = sum_t s_p[t] P_t[i] in the order of open_scalars
// (plonk_rounds.hpp); a polynomial contributes below its own length only.
// grid = (ceil((n+3)/256), k); the scalars of a proof are uniform in a block.
__global__ __launch_bounds__(256) void k_open_lincomb(OpenPolys P, const Fr* scal, Fr* C,
                                                      uint32_t n) {
    const uint32_t p = blockIdx.y;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)n + 3;
    if (i >= stride) return;
    const Fr* s = scal + (uint64_t)OPEN_TERMS * p;
    const Fr* wz = P.wz + p * P.wz_item;
    const Fr* ch = P.chunks + p * P.ch_item;
    Fr acc = s[23].mul(wz[5 * stride + i]);  // z: n + 3
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) acc = acc.add(s[24 + t].mul(ch[t * stride + i]));
    if (i < n + 2) {
#pragma unroll
        for (uint32_t t = 0; t < 5; ++t) acc = acc.add(s[18 + t].mul(wz[t * stride + i]));
        acc = acc.add(s[28].mul(ch[4 * stride + i]));
    }
    if (i < n) {
#pragma unroll
        for (uint32_t t = 0; t < 18; ++t)
            acc = acc.add(s[t].mul(P.key[(uint64_t)t * n + i]));
    }
    C[p * stride + i] = acc;
}

}  // namespace rng
