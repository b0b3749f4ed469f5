// esgpu_bool_bits.hip — the doc bitset of a bool query (BoolQueryBuilder.doToQuery, Lucene's BooleanQuery matching
// rules): one pass over the distinct leaf columns of one owner's clauses, one bit per doc out.
//
// Every leaf (term, range, terms, exists) is one bit of a u64.  Per leaf column the host cuts the key line at the bounds
// of the leaves on it (es_filter_masks.hpp, build_leaf_masks: a leaf accepts a union of intervals), so a doc's leaf mask
// on a column is one table entry, found by the branch-free search over the cuts in LDS (fl_column, shared with the
// filters collect), and the doc's leaf mask is the AND over the columns -- a leaf has a clause only on its own column and
// is all ones on the others.  The combinator (BoolComb: required, prohibited, optional leaves, groups, m) is then
// evaluated per doc on that mask: a handful of ANDs and one popcount, whatever the number of leaves.
//
// exists on a double column: fl_column hands a NaN the column's no-value mask, as it does for a doc without a value, and
// a NaN is a value.  The no-value mask of such a column carries the exists leaves' bits, and the kernel clears them for
// the docs whose present bit is clear (ex_mask).
//
// Output: a thread holds the 4 bits of its 4 consecutive docs, 16 adjacent lanes one 64-bit word.  The nibbles are
// combined across the lanes (8 lanes to a 32-bit half by three xor-shuffles, the high half fetched by a fourth) and lane
// 0 of the 16 stores the word once, already ANDed with the accept word and the tail mask of n_docs.  No atomics, no LDS
// for the output.  Rounds past n_docs store zero words: the collect kernels read the bitset over whole zone blocks.
// Bytes per doc: the leaf columns at the width read (4 for ordinals, 8 otherwise), 1/8 for the accept bits, 1/8 written.
#include "esgpu_bool_bits.hpp"
#include "esgpu_mask_docs.hpp"

namespace esgpu {

__global__ __launch_bounds__(kRgWG) void bool_bits_kernel(BoolBitsParams P) {
    __shared__ FlTab S;
#pragma unroll
    for (uint32_t c = 0; c < kFilterCols; ++c) {
        if (c >= P.n_cols) break;
        const uint64_t* tab = P.table + (size_t)c * kFilterStride;
        const uint32_t n = P.col[c].n_cuts;
        for (uint32_t i = threadIdx.x; i < n; i += kRgWG) S.cuts[c][i] = (long long)tab[i];
        for (uint32_t i = threadIdx.x; i <= n; i += kRgWG) S.masks[c][i] = tab[kRangeCuts + i];
        if (threadIdx.x == 0) {
            S.no_value[c] = tab[2 * kRangeCuts + 1];
            S.col[c] = P.col[c];
        }
    }
    __syncthreads();

    const uint32_t sub = threadIdx.x & 15u;  // the thread's nibble of its 16 lanes' word
    for (uint32_t r = blockIdx.x; r < P.n_rounds; r += gridDim.x) {  // (uniform)
        const uint32_t base = r * kRgRound;
        uint32_t hit = 0;  // bit j: doc j matches the query
        if (base < P.n_docs) {
            unsigned long long m[kRgDocs];
#pragma unroll
            for (uint32_t j = 0; j < kRgDocs; ++j) m[j] = ~0ull;
#pragma unroll 1
            for (uint32_t c = 0; c < P.n_cols; ++c) {
                fl_column(S, c, S.col[c], base, m);
                const unsigned long long ex = P.ex_mask[c];
                if (ex && S.col[c].present) {  // (uniform) exists on a sparse double column: the present bit decides
#pragma unroll
                    for (uint32_t q = 0; q < kRgQuads; ++q) {
                        const uint32_t pr = bits4(S.col[c].present, base + q * kRgQuad + threadIdx.x * 4);
#pragma unroll
                        for (uint32_t t = 0; t < 4; ++t) m[4 * q + t] &= ((pr >> t) & 1u) ? ~0ull : ~ex;
                    }
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < kRgDocs; ++j) hit |= (bool_comb_match(P.comb, m[j] & P.all_mask) ? 1u : 0u) << j;
        }
#pragma unroll
        for (uint32_t q = 0; q < kRgQuads; ++q) {
            uint32_t v = ((hit >> (4 * q)) & 0xFu) << (4 * (sub & 7u));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            v |= __shfl_xor(v, 4);
            const uint32_t hi = __shfl_xor(v, 8);  // lanes 0..7 of the 16: the half of lanes 8..15
            if (sub == 0) {
                const uint32_t w = (base + q * kRgQuad) / 64 + (threadIdx.x >> 4);  // < n_rounds * kRgRound / 64: inside `out`
                const uint32_t doc0 = w * 64;
                unsigned long long word = (unsigned long long)v | ((unsigned long long)hi << 32);
                if (doc0 >= P.n_docs) word = 0ull;
                else if (P.n_docs - doc0 < 64) word &= (1ull << (P.n_docs - doc0)) - 1ull;
                if (word && P.accept) word &= P.accept[w];
                P.out[w] = word;
            }
        }
    }
}

static int bool_bits_occupancy() {
    static const int occ = [] {
        int n = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bool_bits_kernel, kRgWG, 0);
        return e == hipSuccess && n > 0 ? n : 1;
    }();
    return occ;
}

// out: n_pad / 64 words (n_pad: n_docs rounded up to whole zone blocks); the columns, present bitsets and accept bits
// are readable over n_pad docs
void launch_bool_bits(BoolBitsParams P, uint32_t n_pad, int cus, hipStream_t st) {
    static_assert(kBlockDocs % kRgRound == 0, "a zone block is a whole number of rounds");
    P.n_rounds = n_pad / kRgRound;
    if (P.n_rounds == 0) return;
    const uint32_t slots = (uint32_t)std::max(1, cus) * (uint32_t)bool_bits_occupancy();
    hipLaunchKernelGGL(bool_bits_kernel, dim3(std::min(P.n_rounds, slots)), dim3(kRgWG), 0, st, P);
}

}  // namespace esgpu
