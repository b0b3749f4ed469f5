// esgpu_bool_bits.hpp — the bool query's doc bitset (esgpu_bool_bits.hip): parameters and launcher.
#pragma once
#include "es_filter_masks.hpp"
#include "esgpu_kernels.hpp"

namespace esgpu {

// The leaf columns as the filters collect describes them (FilterCol; `table`: [n_cols][kFilterStride], the leaf as the
// slot, build_leaf_masks) and the combinator over a doc's leaf mask.
struct BoolBitsParams {
    FilterCol col[kFilterCols];
    uint64_t ex_mask[kFilterCols];  // a double column: the exists leaves on it (a NaN is a value: only a clear present bit clears them)
    uint32_t n_cols;
    uint32_t n_docs;
    uint32_t n_rounds;              // set by the launcher: n_pad / kRgRound
    uint64_t all_mask;              // the bits of the leaves whose field the segment has (a leaf on a missing field holds for no doc)
    const uint64_t* accept;         // the caller's accept bits; null = all docs
    const uint64_t* table;
    uint64_t* out;                  // n_pad / 64 words, every one written
    BoolComb comb;
};
void launch_bool_bits(BoolBitsParams p, uint32_t n_pad, int cus, hipStream_t s);

}  // namespace esgpu
