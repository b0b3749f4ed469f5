// pack12_check.cpp — the d12 layout of es_pack12.hpp on the host, under AddressSanitizer + UBSan (make check-pack12):
// exact round trips through the group functions the kernels use and through the byte functions, every position of a
// group at the edge values with complemented neighbours, the lengths around a group, and no byte written outside
// ceil(3 n / 2).  Stand-alone, no GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../es_pack12.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, "\n");                   \
        }                                                 \
    } while (0)

// a group through pack8 / unpack8 and, bit for bit, through the byte functions
static void check_group(const uint32_t (&d)[8], const char* what) {
    uint32_t w[3], back[8];
    p12_pack8(d, w);
    p12_unpack8(w, back);
    for (int j = 0; j < 8; ++j) CHECK(back[j] == d[j], "%s: doc %d 0x%X -> 0x%X", what, j, d[j], back[j]);
    uint8_t bytes[12], by_put[12];
    std::memset(by_put, 0, sizeof by_put);
    for (int k = 0; k < 3; ++k)
        for (int q = 0; q < 4; ++q) bytes[4 * k + q] = (uint8_t)(w[k] >> (8 * q));
    for (int j = 0; j < 8; ++j) {
        CHECK(p12_get(bytes, j) == d[j], "%s: byte view of doc %d", what, j);
        p12_put(by_put, j, d[j]);
    }
    CHECK(std::memcmp(bytes, by_put, 12) == 0, "%s: words and bytes disagree", what);
    // the windows: doc 2 i at kP12Even, doc 2 i + 1 at kP12Odd
    for (int i = 0; i < 4; ++i) {
        const uint32_t x = p12_window(w[0], w[1], w[2], i);
        CHECK(((x >> kP12Even) & kP12Mask) == d[2 * i] && ((x >> kP12Odd) & kP12Mask) == d[2 * i + 1], "%s: window %d", what, i);
    }
}

// n docs through p12_pack / p12_unpack inside guard bytes: the round trip is exact and the guards stay
static void check_length(size_t n, std::mt19937& rng) {
    const size_t nb = p12_bytes_any(n), guard = 32;
    if (n % kP12Group == 0) CHECK(p12_bytes(n) == nb && nb == n * 3 / 2, "bytes of %zu docs", n);
    std::vector<uint16_t> src(n), back(n, 0xDEAD);
    for (size_t i = 0; i < n; ++i) src[i] = (uint16_t)(rng() & kP12Mask);
    for (uint8_t fill : {(uint8_t)0x00, (uint8_t)0xFF, (uint8_t)0xA5}) {
        // (exactly guard + nb + guard bytes on the heap: a write past them is the sanitizer's to report)
        std::vector<uint8_t> buf(guard + nb + guard, fill);
        p12_pack(src.data(), n, buf.data() + guard);
        for (size_t i = 0; i < guard; ++i)
            CHECK(buf[i] == fill && buf[guard + nb + i] == fill, "n %zu fill 0x%02X: a byte outside the %zu was written", n, fill, nb);
        p12_unpack(buf.data() + guard, n, back.data());
        for (size_t i = 0; i < n; ++i) CHECK(back[i] == src[i], "n %zu fill 0x%02X: doc %zu 0x%X -> 0x%X", n, fill, i, src[i], back[i]);
        for (size_t i = 0; i < n; ++i) CHECK(p12_get(buf.data() + guard, i) == src[i], "n %zu: byte view of doc %zu", n, i);
    }
    // a tight allocation of its own, so that a read or write one byte past the end is an error, not a guard hit
    std::vector<uint8_t> tight(nb);
    p12_pack(src.data(), n, tight.data());
    p12_unpack(tight.data(), n, back.data());
    for (size_t i = 0; i < n; ++i) CHECK(back[i] == src[i], "n %zu tight: doc %zu", n, i);
}

int main() {
    // every position with the edge values, the neighbours holding the complement
    const uint32_t edges[] = {0u, 1u, 0x7FFu, 0x800u, 0xFFFu};
    for (int pos = 0; pos < 8; ++pos)
        for (uint32_t e : edges) {
            uint32_t d[8];
            for (int j = 0; j < 8; ++j) d[j] = j == pos ? e : (~e & kP12Mask);
            char what[64];
            std::snprintf(what, sizeof what, "pos %d value 0x%X", pos, e);
            check_group(d, what);
        }
    std::mt19937 rng(20240612u);
    for (int g = 0; g < 10000; ++g) {
        uint32_t d[8];
        for (uint32_t& x : d) x = rng() & kP12Mask;
        check_group(d, "random group");
    }
    for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)8192}) check_length(n, rng);
    if (failures) {
        std::fprintf(stderr, "pack12_check: %d failures\n", failures);
        return 1;
    }
    std::printf("pack12_check ok: 40 edge groups, 10000 random groups, lengths 0 1 7 8 9 8192\n");
    return 0;
}
