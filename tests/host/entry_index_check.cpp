// Host-only check of the compacted-entry packing and the lookup-table index
// (renegade_amd/csrc/msm_digits.hpp) that k_msm_digits_compact writes and
// k_msm_entry_lookup_sum reads.  For window sizes c = 8..10 and domains
// n = 2 .. 32768 (N = n + 2 bases):
//   * (poly, w, i, mag, sign) -> (key, val) -> (row, mag, sign) round trips
//     for every corner of the ranges and for random tuples;
//   * msm_lookup_index(key, val, c) == ((w*N + i) << (c-1)) + mag - 1 in
//     64-bit arithmetic, stays below rows << (c-1), and the last entry of the
//     last row is the table's last slot;
//   * distinct (row, mag) give distinct indices (row-major, 2^(c-1) per row);
//   * the row guard: n = 32768, c = 10 has 852 020 rows and fits, its index
//     passes 2^28 (a byte offset past 2^32, hence the 64-bit index), and a
//     base count whose rows reach 2^31 is refused, one below is accepted.
// Plain C++: no HIP header, no device.  Exit status 0 on agreement.
#include <cstdint>
#include <cstdio>

#include "../../renegade_amd/csrc/msm_digits.hpp"

using namespace rng;

static uint64_t g_state = 0x2545f4914f6cdd1dull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static int g_fail = 0;
static void fail(const char* what, uint32_t c, uint64_t N, uint32_t w, uint32_t i, uint32_t mag) {
    if (g_fail++ < 10)
        fprintf(stderr, "FAIL %s: c=%u N=%lu w=%u i=%u mag=%u\n", what, c, (unsigned long)N, w,
                i, mag);
}

static size_t g_checked = 0;
static void check_entry(uint32_t c, uint32_t N, uint32_t poly, uint32_t w, uint32_t i,
                        uint32_t mag, uint32_t sign) {
    const uint32_t key = msm_entry_key(poly, mag, c);
    const uint32_t val = msm_entry_val(w, N, i, sign);
    if (msm_entry_mag(key, c) != mag || (key >> c) != poly) fail("key", c, N, w, i, mag);
    if (msm_entry_row(val) != w * N + i || msm_entry_sign(val) != sign)
        fail("val", c, N, w, i, mag);
    const uint64_t want = (((uint64_t)w * N + i) << (c - 1)) + (mag - 1);
    const uint64_t got = msm_lookup_index(key, val, c);
    if (got != want) fail("index", c, N, w, i, mag);
    if (got >= (msm_table_rows(N, c) << (c - 1))) fail("index past the table", c, N, w, i, mag);
    // row-major: the slot recovers (row, mag)
    if ((got >> (c - 1)) != (uint64_t)w * N + i || (got & ((1u << (c - 1)) - 1)) != mag - 1)
        fail("slot", c, N, w, i, mag);
    ++g_checked;
}

int main() {
    for (uint32_t c = 8; c <= 10; ++c) {
        const uint32_t W = (256 + c - 1) / c, half = 1u << (c - 1);
        for (uint32_t n = 2; n <= 32768; n <<= 1) {
            const uint32_t N = n + 2;
            if (!msm_entry_rows_fit(N, c)) fail("rows_fit", c, N, 0, 0, 0);
            if (msm_table_rows(N, c) != (uint64_t)W * N) fail("rows", c, N, 0, 0, 0);
            // polys: the key keeps c bits for the magnitude, 32 - c for the poly
            const uint32_t polys[3] = {0, 239, (1u << (32 - c)) - 1};
            const uint32_t ws[3] = {0, W / 2, W - 1};
            const uint32_t is[4] = {0, 1, n, N - 1};
            const uint32_t mags[4] = {1, 2, half - 1, half};
            for (uint32_t poly : polys)
                for (uint32_t w : ws)
                    for (uint32_t i : is)
                        for (uint32_t mag : mags)
                            for (uint32_t sign = 0; sign < 2; ++sign)
                                check_entry(c, N, poly, w, i, mag, sign);
            for (int k = 0; k < 2000; ++k) {
                const uint64_t r = next_u64();
                check_entry(c, N, (uint32_t)(r >> 40) % 65535u, (uint32_t)(r >> 8) % W,
                            (uint32_t)(r >> 16) % N, 1 + (uint32_t)(r >> 32) % half,
                            (uint32_t)r & 1);
            }
            // the last entry of the last row is the last slot of the table
            const uint64_t last = msm_lookup_index(msm_entry_key(0, half, c),
                                                   msm_entry_val(W - 1, N, N - 1, 1), c);
            if (last + 1 != (msm_table_rows(N, c) << (c - 1))) fail("last slot", c, N, W, N, half);
        }
    }
    // n = 32768, c = 10: 26 * 32770 rows, far below 2^31, but the slot index
    // passes 2^28 and a 64-byte slot's byte offset passes 2^32
    {
        const uint32_t c = 10, N = 32770, W = 26;
        if (msm_table_rows(N, c) != 852020ull || !msm_entry_rows_fit(N, c))
            fail("guard at n=32768", c, N, 0, 0, 0);
        const uint64_t last = msm_lookup_index(msm_entry_key(0, 512, c),
                                               msm_entry_val(W - 1, N, N - 1, 0), c);
        if (last != 852020ull * 512 - 1 || last < (1ull << 28) || last * 64 < (1ull << 32))
            fail("index at n=32768", c, N, W - 1, N - 1, 512);
    }
    // the guard itself: rows = W*N must stay below 2^31 (bit 31 is the sign)
    for (uint32_t c = 8; c <= 10; ++c) {
        const uint64_t W = (256 + c - 1) / c;
        const uint64_t n_bad = ((1ull << 31) + W - 1) / W;  // smallest N with W*N >= 2^31
        if (msm_entry_rows_fit(n_bad, c)) fail("guard accepts 2^31 rows", c, n_bad, 0, 0, 0);
        if (!msm_entry_rows_fit(n_bad - 1, c)) fail("guard refuses", c, n_bad - 1, 0, 0, 0);
        // the largest accepted row keeps the sign bit free
        const uint64_t top = W * (n_bad - 1) - 1;
        if (top >> 31) fail("row reaches the sign bit", c, n_bad - 1, 0, 0, 0);
        const uint32_t val = (1u << 31) | (uint32_t)top;
        if (msm_entry_row(val) != top || msm_entry_sign(val) != 1)
            fail("top row", c, n_bad - 1, 0, 0, 0);
        if (msm_lookup_index(msm_entry_key(0, 1, c), val, c) != top << (c - 1))
            fail("top row index", c, n_bad - 1, 0, 0, 0);
    }
    if (g_fail) {
        fprintf(stderr, "entry_index_check: %d failures\n", g_fail);
        return 1;
    }
    printf("entry_index_check ok: %zu entries\n", g_checked);
    return 0;
}
