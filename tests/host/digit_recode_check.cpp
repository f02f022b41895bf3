// Host-only check of msm_recode_digit (renegade_amd/csrc/msm_digits.hpp), the
// signed-digit recoding every fixed-base MSM path shares.  For each window
// size c in 8..13 and each scalar s (the edge scalars of the lookup tests
// plus random ones below r), walking w = 0 .. W-1 with W = ceil(256/c):
//   * every magnitude is at most 2^(c-1), every sign 0 or 1 (raw == 2^c,
//     all ones plus a carry, is the zero digit with sign 1 and a carry);
//   * raw == 2^(c-1) stays +2^(c-1) with no carry, raw > 2^(c-1) goes
//     negative with a carry;
//   * sum_w sign*mag*2^(c*w) == s, computed in 320-bit two's complement;
//   * the carry out of the top window is zero.
// Plain C++: no HIP header, no device.  Exit status 0 on agreement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../renegade_amd/csrc/msm_digits.hpp"

using rng::MsmDigit;
using rng::msm_recode_digit;

// BN254 scalar field modulus r, LE limbs
static const uint64_t R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull,
                              0xb85045b68181585dull, 0x30644e72e131a029ull};

struct U256 {
    uint64_t l[4];
};

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static bool less_than_r(const U256& a) {
    for (int i = 3; i >= 0; --i)
        if (a.l[i] != R[i]) return a.l[i] < R[i];
    return false;
}

static U256 sub_small(const uint64_t a[4], uint64_t k) {
    U256 r;
    uint64_t borrow = k;
    for (int i = 0; i < 4; ++i) {
        r.l[i] = a[i] - borrow;
        borrow = a[i] < borrow ? 1 : 0;
    }
    return r;
}

static U256 pow2(unsigned bit) {
    U256 r = {{0, 0, 0, 0}};
    r.l[bit >> 6] = 1ull << (bit & 63);
    return r;
}

static U256 pow2_minus_1(unsigned bits) {  // bits <= 255
    U256 r = {{0, 0, 0, 0}};
    for (unsigned b = 0; b < bits; ++b) r.l[b >> 6] |= 1ull << (b & 63);
    return r;
}

static U256 small(uint64_t v) { return U256{{v, 0, 0, 0}}; }

static U256 or_shifted(U256 a, uint64_t v, unsigned bit) {  // a | v << bit, v < 2^32
    a.l[bit >> 6] |= v << (bit & 63);
    if ((bit & 63) > 32 && (bit >> 6) + 1 < 4) a.l[(bit >> 6) + 1] |= v >> (64 - (bit & 63));
    return a;
}

// acc (5 limbs, two's complement) += sign * mag << bit
static void add_digit(uint64_t acc[5], uint32_t mag, uint32_t sign, unsigned bit) {
    uint64_t term[5] = {0, 0, 0, 0, 0};
    unsigned limb = bit >> 6, off = bit & 63;
    term[limb] = (uint64_t)mag << off;
    if (off && limb + 1 < 5) term[limb + 1] = off > 32 ? (uint64_t)mag >> (64 - off) : 0;
    unsigned __int128 carry = 0;
    if (sign) {  // two's complement negation
        for (int i = 0; i < 5; ++i) term[i] = ~term[i];
        carry = 1;
    }
    for (int i = 0; i < 5; ++i) {
        unsigned __int128 t = (unsigned __int128)acc[i] + term[i] + carry;
        acc[i] = (uint64_t)t;
        carry = t >> 64;
    }
}

static int g_fail = 0;
static void fail(const char* what, uint32_t c, uint32_t w, const U256& s) {
    if (g_fail++ < 10)
        fprintf(stderr, "FAIL %s: c=%u w=%u s=%016lx%016lx%016lx%016lx\n", what, c, w,
                (unsigned long)s.l[3], (unsigned long)s.l[2], (unsigned long)s.l[1],
                (unsigned long)s.l[0]);
}

static void check_scalar(const U256& s, uint32_t c) {
    const uint32_t W = (256 + c - 1) / c;
    const uint32_t half = 1u << (c - 1);
    uint64_t acc[5] = {0, 0, 0, 0, 0};
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; ++w) {
        // the raw window value, cut here independently of the function
        uint64_t raw = 0;
        for (uint32_t k = 0; k < c; ++k) {
            uint32_t bit = w * c + k;
            if (bit < 256 && ((s.l[bit >> 6] >> (bit & 63)) & 1)) raw |= 1ull << k;
        }
        raw += carry;
        const MsmDigit d = msm_recode_digit(s.l, c, w, carry);
        if (d.mag > half || d.sign > 1) fail("range", c, w, s);
        if (raw > half) {
            if (!(d.sign == 1 && carry == 1 && d.mag == (1u << c) - raw)) fail("negative", c, w, s);
        } else {
            if (!(d.sign == 0 && carry == 0 && d.mag == raw)) fail("positive", c, w, s);
        }
        add_digit(acc, d.mag, d.sign, w * c);
    }
    if (carry != 0) fail("carry out of the top window", c, W, s);
    if (acc[0] != s.l[0] || acc[1] != s.l[1] || acc[2] != s.l[2] || acc[3] != s.l[3] ||
        acc[4] != 0)
        fail("digit sum", c, W, s);
}

int main() {
    size_t checked = 0;
    for (uint32_t c = 8; c <= 13; ++c) {
        const uint32_t half = 1u << (c - 1);
        const uint32_t W = (256 + c - 1) / c;
        std::vector<U256> ss;
        ss.push_back(small(0));
        ss.push_back(small(1));
        ss.push_back(small(2));
        ss.push_back(small(half));      // digit exactly 2^(c-1)
        ss.push_back(small(half + 1));  // negative with carry
        ss.push_back(small(half - 1));
        ss.push_back(small((1u << c) + half));
        ss.push_back(sub_small(R, 1));
        ss.push_back(sub_small(R, 2));
        ss.push_back(pow2_minus_1(253));                // all ones
        ss.push_back(pow2_minus_1(c * (253 / c)));      // every digit 2^c - 1
        ss.push_back(pow2_minus_1(128));
        for (uint32_t w = 0; w < W; ++w) {  // a single 1, half and half + 1 in every window
            if (w * c + c > 253) break;
            ss.push_back(pow2(w * c));
            ss.push_back(or_shifted(small(0), half, w * c));
            ss.push_back(or_shifted(small(0), half + 1, w * c));
            ss.push_back(or_shifted(pow2_minus_1(w * c), half, w * c));  // carry arrives at half-1.. edge
            ss.push_back(or_shifted(pow2_minus_1(w * c), half - 1, w * c));
        }
        for (int k = 0; k < 20000; ++k) {
            U256 s = {{next_u64(), next_u64(), next_u64(), next_u64() >> 2}};
            if (less_than_r(s)) ss.push_back(s);
        }
        for (const U256& s : ss) {
            if (!less_than_r(s)) {
                fail("test scalar not below r", c, 0, s);
                continue;
            }
            check_scalar(s, c);
            ++checked;
        }
    }
    if (g_fail) {
        fprintf(stderr, "digit_recode_check: %d failures\n", g_fail);
        return 1;
    }
    printf("digit_recode_check ok: %zu (scalar, c) pairs\n", checked);
    return 0;
}
