// Stand-alone check of rank_terms_by_count (es_term_rank.hpp), built with AddressSanitizer + UBSan by
// `make check-term-rank`: no GPU, no library.
#include "../es_term_rank.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static void run(const std::vector<uint64_t>& counts, const std::vector<uint32_t>& want_order) {
    const uint32_t T = (uint32_t)counts.size();
    std::vector<uint32_t> rank_of(T, ~0u), ord_of_rank(T, ~0u);
    rank_terms_by_count(counts.data(), T, rank_of.data(), ord_of_rank.data());
    for (uint32_t r = 0; r < T; ++r) {
        CHECK(ord_of_rank[r] < T);
        CHECK(rank_of[ord_of_rank[r]] == r);  // inverse permutations
        if (r + 1 < T) {
            const uint32_t a = ord_of_rank[r], b = ord_of_rank[r + 1];
            CHECK(counts[a] > counts[b] || (counts[a] == counts[b] && a < b));  // count desc, then ordinal asc
        }
    }
    if (!want_order.empty()) CHECK(ord_of_rank == want_order);
}

int main() {
    run({7}, {0});                                   // T = 1
    run({0}, {0});                                   // ... with no doc
    run({}, {});                                     // no term at all
    run({3, 9, 3, 9, 1}, {1, 3, 0, 2, 4});           // ties: the smaller ordinal first
    run({0, 0, 5, 0}, {2, 0, 1, 3});                 // zeros keep ordinal order behind the terms with docs
    run({4, 4, 4, 4}, {0, 1, 2, 3});                 // every count tied
    run({1, 2, 3, 4}, {3, 2, 1, 0});                 // ascending counts
    run({~0ull, 1ull << 40, ~0ull}, {0, 2, 1});      // counts past 32 bits
    // three equal counts behind 27 distinct larger ones: the tied terms take the last ranks in ordinal order
    {
        std::vector<uint64_t> c(30);
        for (uint32_t t = 0; t < 30; ++t) c[t] = 1000 - t;
        c[20] = c[4] = c[11] = 500;
        std::vector<uint32_t> rank_of(30), ord(30);
        rank_terms_by_count(c.data(), 30, rank_of.data(), ord.data());
        CHECK(rank_of[4] == 27 && rank_of[11] == 28 && rank_of[20] == 29);
        run(c, {});
    }
    // randomised, small alphabets of counts so that ties are everywhere
    uint64_t x = 88172645463325252ull;
    auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int it = 0; it < 200; ++it) {
        const uint32_t T = 1 + (uint32_t)(next() % 700);
        std::vector<uint64_t> c(T);
        for (uint64_t& v : c) v = next() % (1 + it % 9);
        run(c, {});
    }
    if (failures) {
        std::fprintf(stderr, "term_rank_check: %d failure(s)\n", failures);
        return 1;
    }
    std::puts("term_rank_check: ok");
    return 0;
}
