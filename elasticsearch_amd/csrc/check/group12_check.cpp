// group12_check.cpp — the g12 layout of es_group12.hpp on the host, under AddressSanitizer + UBSan (make check-group12):
// the reference grouping of a block and the position-to-rank lookup against brute force -- every position's delta is a
// delta of a doc of the rank the lookup names, as a multiset per rank; the offsets are the counts of the lower groups;
// the lookup of 8 positions agrees with the lookup of one; the prefix byte counts; the group a lane of the grouped kernel
// loads for every prefix and position (g12_load_group: its own or group 0, inside the block).  Stand-alone, no GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../es_group12.hpp"

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

// one block of n docs: grouped by the reference, read back through the lookup for every K of `ks`
static void check_block(const std::vector<uint16_t>& rank, const std::vector<uint16_t>& d, const char* what) {
    const uint32_t n = (uint32_t)rank.size();
    // (tight heap allocations: a byte or an offset past them is the sanitizer's to report)
    std::vector<uint8_t> out(g12_block_bytes());
    std::vector<uint16_t> off(kG12OffStride, 0xDEAD);
    g12_group_block(rank.data(), d.data(), n, out.data(), off.data());
    // the offsets by brute force
    for (uint32_t r = 0; r <= kG12Groups; ++r) {
        uint32_t below = 0;
        for (uint32_t i = 0; i < n; ++i) below += g12_group(rank[i]) < r ? 1u : 0u;
        CHECK(off[r] == below, "%s: off[%u] = %u, %u docs below", what, r, off[r], below);
    }
    for (uint32_t r = kG12Offs; r < kG12OffStride; ++r) CHECK(off[r] == 0, "%s: padding offset %u", what, r);
    CHECK(off[0] == 0 && off[kG12Groups] <= kG12Block, "%s: ends", what);
    std::vector<uint16_t> back(kG12Block);
    p12_unpack(out.data(), kG12Block, back.data());
    const auto at = [&](uint32_t j) { return (uint32_t)off[j]; };
    for (uint32_t K : {1u, 2u, 5u, 10u, 64u, 65u, kG12Groups}) {
        // the deltas the lookup gives each rank below K, against the docs of that rank
        std::vector<std::vector<uint16_t>> got(K), want(K);
        for (uint32_t i = 0; i < n; ++i)
            if (rank[i] < K) want[rank[i]].push_back((uint16_t)(d[i] & kP12Mask));
        for (uint32_t p = 0; p < kG12Block; ++p) {
            const uint32_t r = g12_rank_at(p, K, at);
            CHECK(r <= K && (r == K) == (p >= off[K]), "%s: K %u position %u rank %u", what, K, p, r);
            if (r < K) got[r].push_back(back[p]);
        }
        for (uint32_t r = 0; r < K; ++r) {
            std::sort(got[r].begin(), got[r].end());
            std::sort(want[r].begin(), want[r].end());
            CHECK(got[r] == want[r], "%s: K %u rank %u: %zu deltas for %zu docs", what, K, r, got[r].size(), want[r].size());
        }
        // the 8-position form over every offset, and over those inside a span of 512 positions alone
        for (uint32_t p0 = 0; p0 < kG12Block; p0 += 8) {
            uint32_t r8[8], s8[8];
            g12_ranks8(p0, 0, K, at, r8);
            const uint32_t w = p0 & ~511u;
            uint32_t base = 0, upto = 0;
            for (uint32_t j = 1; j <= K; ++j) {
                base += off[j] <= w ? 1u : 0u;
                upto += off[j] < w + 512u ? 1u : 0u;
            }
            g12_ranks8(p0, base, upto, at, s8);
            for (uint32_t i = 0; i < 8; ++i) {
                const uint32_t want = g12_rank_at(p0 + i, K, at);
                CHECK(r8[i] == want && s8[i] == want, "%s: K %u ranks8 at %u: %u / %u, want %u", what, K, p0 + i, r8[i], s8[i], want);
            }
        }
    }
}

int main() {
    std::mt19937 rng(20240713u);
    const auto deltas = [&](uint32_t n) {
        std::vector<uint16_t> d(n);
        for (uint16_t& x : d) x = (uint16_t)(rng() & kP12Mask);
        return d;
    };
    int blocks = 0;
    // sizes around a packed group and the block; ranks skewed, uniform over many terms, and with missing ordinals
    for (uint32_t n : {0u, 1u, 7u, 8u, 9u, 8191u, 8192u}) {
        for (int kind = 0; kind < 4; ++kind) {
            std::vector<uint16_t> rank(n);
            for (uint16_t& r : rank) {
                const uint32_t u = rng();
                r = kind == 0   ? (uint16_t)(u % 5)
                    : kind == 1 ? (uint16_t)std::min<uint32_t>(999, (uint32_t)(1000.0 / (1 + u % 1000)) - 1)
                    : kind == 2 ? (uint16_t)(u % 300)
                                : (u % 7 == 0 ? (uint16_t)kG12Missing : (uint16_t)(u % 200));
            }
            char what[64];
            std::snprintf(what, sizeof what, "n %u kind %d", n, kind);
            check_block(rank, deltas(n), what);
            ++blocks;
        }
    }
    // degenerate blocks: one rank only, no collected doc, empty ranks in a row, runs of 1 and 2
    {
        std::vector<uint16_t> rank(kG12Block, 0);
        check_block(rank, deltas(kG12Block), "all rank 0");
        std::fill(rank.begin(), rank.end(), (uint16_t)kG12Missing);
        check_block(rank, deltas(kG12Block), "all missing");
        std::fill(rank.begin(), rank.end(), (uint16_t)kG12Groups);
        check_block(rank, deltas(kG12Block), "all rank 128");
        for (uint32_t i = 0; i < kG12Block; ++i) rank[i] = i < 3 ? (uint16_t)(i == 2 ? 4 : 0) : i < 6 ? (uint16_t)(i == 3 ? 1 : 7) : (uint16_t)9;
        check_block(rank, deltas(kG12Block), "short runs, empty ranks");
        blocks += 4;
    }
    CHECK(g12_prefix_bytes(0) == 0 && g12_prefix_bytes(1) == 12 && g12_prefix_bytes(8) == 12 && g12_prefix_bytes(9) == 24 &&
              g12_prefix_bytes(kG12Block) == g12_block_bytes() && g12_block_bytes() == 12288,
          "prefix bytes");
    CHECK(kG12OffBytes == 260 && kG12OffBytes % 4 == 0, "offset stride");
    // the group a lane of the grouped kernel loads (g12_load_group), for every prefix n and every p0 a thread holds: its
    // own group, which then lies below ceil8(n), or group 0 -- and its 12 bytes inside the block's data, read here from
    // a tight heap block
    {
        std::vector<uint8_t> data(g12_block_bytes(), 1);
        uint64_t own = 0, clamped = 0, sum = 0;
        for (uint32_t n = 0; n <= kG12Block; ++n) {
            for (uint32_t p0 = 0; p0 < kG12Block; p0 += kP12Group) {
                const uint32_t g = g12_load_group(p0, n);
                const size_t byte = (size_t)g * (kP12Words * 4);
                const bool is_own = g == p0 / kP12Group && (uint64_t)g * kP12Group < g12_ceil8(n);
                CHECK(is_own || g == 0, "load group: n %u p0 %u -> group %u", n, p0, g);
                CHECK(is_own == (p0 < n) || (g == 0 && p0 == 0), "load group: n %u p0 %u own %d", n, p0, (int)is_own);
                CHECK(byte + kP12Words * 4 <= g12_block_bytes() && byte + kP12Words * 4 <= std::max<size_t>(g12_prefix_bytes(n), kP12Words * 4),
                      "load group: n %u p0 %u reads bytes [%zu, +12)", n, p0, byte);
                for (uint32_t i = 0; i < kP12Words * 4; ++i) sum += data[byte + i];
                ++(is_own ? own : clamped);
            }
        }
        CHECK(sum == (own + clamped) * kP12Words * 4, "load group: bytes read");
        std::printf("group12_check: load group over n = 0..%u: %llu own, %llu clamped to group 0\n", kG12Block, (unsigned long long)own,
                    (unsigned long long)clamped);
    }
    if (failures) {
        std::fprintf(stderr, "group12_check: %d failures\n", failures);
        return 1;
    }
    std::printf("group12_check ok: %d blocks, every position's rank for K = 1 2 5 10 64 65 128\n", blocks);
    return 0;
}
