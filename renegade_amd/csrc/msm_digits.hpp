// Signed base-2^c digit recoding of one canonical scalar, shared by every
// fixed-base MSM path (the sorted bucket pipeline, its compacted variant and
// the direct-lookup sum) and by the host check tests/host/digit_recode_check.cpp.
// Plain C++: usable from host code with no HIP header.
//
//   s = sum_w sign_w * mag_w * 2^(c*w),   0 <= mag_w <= 2^(c-1)
//
// Window w holds raw = bits [c*w, c*w + c) of s plus the carry out of window
// w-1.  raw > 2^(c-1) becomes the negative digit raw - 2^c with a carry into
// the next window; raw == 2^(c-1) stays +2^(c-1) with no carry.  For
// s < 2^254 <= 2^(W*c-1), W = ceil(256/c), the carry out of the top window
// is zero.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MSM_DIGIT_HD __host__ __device__
#else
#define MSM_DIGIT_HD
#endif

namespace rng {

struct MsmDigit {
    uint32_t mag;   // 0 .. 2^(c-1)
    uint32_t sign;  // 1 = negative
};

// digit w of scalar s (canonical, 4 LE limbs) at window size c (1 <= c <= 31).
// `carry` is the carry into window w (0 for w = 0) and leaves as the carry
// into window w+1, so the caller walks w = 0, 1, .. in order.
MSM_DIGIT_HD inline MsmDigit msm_recode_digit(const uint64_t s[4], uint32_t c, uint32_t w,
                                              uint32_t& carry) {
    const uint32_t half = 1u << (c - 1);
    const uint64_t cmask = (1ull << c) - 1;
    const uint32_t bit0 = w * c;
    const uint32_t limb = bit0 >> 6, off = bit0 & 63;
    uint64_t raw = limb < 4 ? s[limb] >> off : 0;
    if (off + c > 64 && limb + 1 < 4) raw |= s[limb + 1] << (64 - off);
    raw = (raw & cmask) + carry;
    MsmDigit d;
    if (raw > half) {  // negative digit raw - 2^c, carry into the next window
        d.mag = (uint32_t)((1ull << c) - raw);
        d.sign = 1;
        carry = 1;
    } else {  // raw == half stays +half, no carry
        d.mag = (uint32_t)raw;
        d.sign = 0;
        carry = 0;
    }
    return d;
}

// ---- compacted entries of the fixed-base paths ----
// A non-zero digit travels as two words (k_msm_digits_fixed's packing):
//   key = poly << c | mag          (1 <= mag <= 2^(c-1) needs c bits)
//   val = sign << 31 | (w*N + i)   (row of the window table, N bases)
// so the packing needs W*N < 2^31 rows.

MSM_DIGIT_HD inline uint32_t msm_entry_key(uint32_t poly, uint32_t mag, uint32_t c) {
    return (poly << c) | mag;
}
MSM_DIGIT_HD inline uint32_t msm_entry_val(uint32_t w, uint32_t N, uint32_t i, uint32_t sign) {
    return (sign << 31) | (w * N + i);
}
MSM_DIGIT_HD inline uint32_t msm_entry_mag(uint32_t key, uint32_t c) {
    return key & ((1u << c) - 1);
}
MSM_DIGIT_HD inline uint32_t msm_entry_row(uint32_t val) { return val & 0x7fffffffu; }
MSM_DIGIT_HD inline uint32_t msm_entry_sign(uint32_t val) { return val >> 31; }

// rows of the window table over N bases at window size c
MSM_DIGIT_HD inline uint64_t msm_table_rows(uint64_t N, uint32_t c) {
    return (uint64_t)((256 + c - 1) / c) * N;
}
// the row must leave bit 31 of val to the sign
MSM_DIGIT_HD inline bool msm_entry_rows_fit(uint64_t N, uint32_t c) {
    return msm_table_rows(N, c) < (1ull << 31);
}

// where the entry's point d * 2^(c*w) * base_i lies in the lookup table
//   L[((w*N + i) << (c-1)) + d-1];
// 64-bit: the product passes 2^32 long before the row count passes 2^31
MSM_DIGIT_HD inline uint64_t msm_lookup_index(uint32_t key, uint32_t val, uint32_t c) {
    return ((uint64_t)msm_entry_row(val) << (c - 1)) + (msm_entry_mag(key, c) - 1);
}

}  // namespace rng
