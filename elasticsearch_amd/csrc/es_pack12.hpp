// es_pack12.hpp — the one statement of the d12 layout: a metric column's deltas over vmin at 12 bits each
// (DevColumn.d12), as Lucene's doc-values writer stores a column whose values span < 4096.
//
// Packed: 8 docs make a group of three little-endian dwords, doc j in bits [12 j, 12 j + 12) of the group's 96 --
//   w0 = d0 | d1 << 12 | d2 << 24,  w1 = d2 >> 8 | d3 << 4 | d4 << 16 | d5 << 28,  w2 = d5 >> 4 | d6 << 8 | d7 << 20
// so a thread's 8 docs are one 12-byte load, group g of a column lies at byte 12 g, and n docs (a multiple of 8) take
// 3 n / 2 bytes.  Read back as four windows, each holding two neighbours at bits 4 and 16:
//   x0 = w0 << 4,  x1 = (w1:w0) >> 20,  x2 = (w2:w1) >> 12,  x3 = w2 >> 4   (the other bits are other docs': mask them)
// -- the odd doc sits where a d16 word holds it, and neither funnel shift is a whole number of bytes (a byte shuffle
// would take its selector from a register, which the ranked kernel has none to spare for).
// Host and device: the recode kernel (esgpu_kernels.hip), the ranked kernel (esgpu_ranked.hip) and the host check
// (check/pack12_check.cpp) all go through these functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ES_P12_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ES_P12_HD inline
#endif

constexpr uint32_t kP12Group = 8;    // docs per group
constexpr uint32_t kP12Words = 3;    // dwords per group
constexpr uint32_t kP12Mask = 0xFFFu;

// bytes of n docs, n a multiple of kP12Group
ES_P12_HD size_t p12_bytes(size_t n) { return n / kP12Group * (kP12Words * 4); }

// 8 deltas (each < 4096) into a group's three words
ES_P12_HD void p12_pack8(const uint32_t (&d)[8], uint32_t (&w)[3]) {
    w[0] = d[0] | (d[1] << 12) | (d[2] << 24);
    w[1] = (d[2] >> 8) | (d[3] << 4) | (d[4] << 16) | (d[5] << 28);
    w[2] = (d[5] >> 4) | (d[6] << 8) | (d[7] << 20);
}
// window i (0..3) of a group: docs 2 i and 2 i + 1 at bits kP12Even and kP12Odd, other docs' bits around them
constexpr uint32_t kP12Even = 4, kP12Odd = 16;
ES_P12_HD uint32_t p12_window(uint32_t w0, uint32_t w1, uint32_t w2, int i) {
    return i == 0 ? w0 << 4 : i == 1 ? (w0 >> 20) | (w1 << 12) : i == 2 ? (w1 >> 12) | (w2 << 20) : w2 >> 4;
}
ES_P12_HD uint32_t p12_even(uint32_t x) { return (x >> kP12Even) & kP12Mask; }
ES_P12_HD uint32_t p12_odd(uint32_t x) { return (x >> kP12Odd) & kP12Mask; }
// a group's three words back into its 8 deltas
ES_P12_HD void p12_unpack8(const uint32_t (&w)[3], uint32_t (&d)[8]) {
    for (int i = 0; i < 4; ++i) {
        const uint32_t x = p12_window(w[0], w[1], w[2], i);
        d[2 * i] = p12_even(x);
        d[2 * i + 1] = p12_odd(x);
    }
}

// The same layout by bytes, for any number of docs: doc i starts at bit 12 i of the little-endian stream, so n docs take
// ceil(3 n / 2) bytes and no access reaches past them.  (Host-side: tails, checks.)
ES_P12_HD size_t p12_bytes_any(size_t n) { return (3 * n + 1) / 2; }
ES_P12_HD uint32_t p12_get(const uint8_t* b, size_t i) {
    const size_t o = 3 * (i / 2);
    return i & 1 ? (uint32_t)(b[o + 1] >> 4) | ((uint32_t)b[o + 2] << 4) : (uint32_t)b[o] | ((uint32_t)(b[o + 1] & 0x0Fu) << 8);
}
ES_P12_HD void p12_put(uint8_t* b, size_t i, uint32_t d) {
    const size_t o = 3 * (i / 2);
    if (i & 1) {
        b[o + 1] = (uint8_t)((b[o + 1] & 0x0Fu) | ((d & 0xFu) << 4));
        b[o + 2] = (uint8_t)(d >> 4);
    } else {
        b[o] = (uint8_t)d;
        b[o + 1] = (uint8_t)((b[o + 1] & 0xF0u) | ((d >> 8) & 0xFu));
    }
}
// n 16-bit deltas into the packed form and back: whole groups by words (as the kernels do), a tail by bytes
ES_P12_HD void p12_pack(const uint16_t* src, size_t n, uint8_t* out) {
    size_t i = 0;
    for (; i + kP12Group <= n; i += kP12Group) {
        uint32_t d[8], w[3];
        for (int j = 0; j < 8; ++j) d[j] = src[i + j];
        p12_pack8(d, w);
        for (int k = 0; k < 3; ++k)
            for (int q = 0; q < 4; ++q) out[i / 2 * 3 + 4 * k + q] = (uint8_t)(w[k] >> (8 * q));
    }
    if (i < n) out[p12_bytes_any(n) - 1] = 0;  // (an odd tail's last byte holds one nibble: the other is zero)
    for (; i < n; ++i) p12_put(out, i, src[i]);
}
ES_P12_HD void p12_unpack(const uint8_t* in, size_t n, uint16_t* dst) {
    size_t i = 0;
    for (; i + kP12Group <= n; i += kP12Group) {
        uint32_t d[8], w[3];
        for (int k = 0; k < 3; ++k) {
            const uint8_t* p = in + i / 2 * 3 + 4 * k;
            w[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
        p12_unpack8(w, d);
        for (int j = 0; j < 8; ++j) dst[i + j] = (uint16_t)d[j];
    }
    for (; i < n; ++i) dst[i] = (uint16_t)p12_get(in, i);
}
