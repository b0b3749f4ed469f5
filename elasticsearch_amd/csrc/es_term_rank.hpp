// Frequency ranks of a segment's terms (host only, no dependencies: csrc/check/term_rank_check.cpp runs it stand-alone).
//
// A segment's per-ordinal doc counts are immutable (Lucene's docFreq), so for an unfiltered terms aggregation ordered by
// count descending the shard's top terms are known before a doc is collected.  Rank 0 is the most frequent ordinal; equal
// counts rank the smaller ordinal first -- the order InternalOrder.COUNT_DESC gives (count descending, then the term
// ascending; ordinals number the terms in ascending order), which is what the build's top-k uses for
// ESGPU_ORDER_COUNT_DESC.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>

// counts[T] -> rank_of[T] (ordinal -> rank) and ord_of_rank[T] (rank -> ordinal), inverse permutations of [0, T)
inline void rank_terms_by_count(const uint64_t* counts, uint32_t T, uint32_t* rank_of, uint32_t* ord_of_rank) {
    std::iota(ord_of_rank, ord_of_rank + T, 0u);
    std::stable_sort(ord_of_rank, ord_of_rank + T, [&](uint32_t a, uint32_t b) { return counts[a] > counts[b]; });
    for (uint32_t r = 0; r < T; ++r) rank_of[ord_of_rank[r]] = r;
}
