// esgpu_filters.hip — the filters aggregation's collect (path 12, FiltersAggregator.java:78-110): one pass over the
// distinct clause columns and one metric field into the [R] cells of a pipeline's ordinary grid.
//
// A doc goes into every bucket whose filter it matches, so -- as in the range collect -- the bucket dimension is a u64
// mask per doc.  A filter is a conjunction of term / range clauses; each clause is an interval of keys on its column
// (es_filter_masks.hpp), and the host cuts every clause column's key line at the bounds of the clauses on it
// (FiltersParams).  A doc's mask on one column is the table entry of its value's elementary interval, found by the
// branch-free binary search over the cuts in LDS (rg_lookup) -- no loop over the filters or the clauses per doc -- or the
// column's no-value mask (a clear present bit, the missing ordinal, NaN: the filters without a clause there).  The doc's
// mask is the AND over the columns, taken one column after another so that only the 8 masks stay live; a doc that is
// accepted and matches no filter gets the other bucket's bit.  Values are compared as signed 64-bit keys: ordinals and
// longs as they are, doubles through the order-preserving image of their bits (rg_key).
//
// The tables and a clause column's lookup (FlTab, fl_column): esgpu_mask_docs.hpp, shared with the keyed form
// (esgpu_mask_hist.hip); accumulation and flush: esgpu_range_cells.hpp, shared with the range collect too.  The staging
// and the round below are also there as fl_stage / fl_docs for the keyed kernel; this kernel keeps them written out --
// called through those functions its counts-only and avg instantiations took 74 VGPRs instead of 68 / 72 and lost a
// wave per SIMD (DESIGN §5 "Path 13").
#include "esgpu_mask_docs.hpp"

namespace esgpu {

struct FlLds {
    FlTab tab;
    RgCells cells;
};

template <int MET>
__global__ __launch_bounds__(kRgWG) void filters_kernel(FiltersParams P) {
    __shared__ FlLds S;
    const uint32_t R = P.R;
#pragma unroll
    for (uint32_t c = 0; c < kFilterCols; ++c) {
        if (c >= P.n_cols) break;
        const uint64_t* tab = P.table + (size_t)c * kFilterStride;
        const uint32_t n = P.col[c].n_cuts;
        for (uint32_t i = threadIdx.x; i < n; i += kRgWG) S.tab.cuts[c][i] = (long long)tab[i];
        for (uint32_t i = threadIdx.x; i <= n; i += kRgWG) S.tab.masks[c][i] = tab[kRangeCuts + i];
        if (threadIdx.x == 0) {
            S.tab.no_value[c] = tab[2 * kRangeCuts + 1];
            S.tab.col[c] = P.col[c];
        }
    }
    rg_cells_init(S.cells);
    __syncthreads();

    const uint32_t b_begin = blockIdx.x * P.blocks_per_wg;
    const uint32_t b_end = min(b_begin + P.blocks_per_wg, P.n_blocks);
    const bool lane0 = (threadIdx.x & 63) == 0;
    const bool vcnt = MET > 0 && P.vcnt_mode != 0;
    const unsigned long long other = P.other_bit >= 0 ? 1ull << P.other_bit : 0ull;

    for (uint32_t base = b_begin * kBlockDocs; base < b_end * kBlockDocs; base += kRgRound) {
        if (base >= P.n_docs) break;  // (uniform: the rest of the last block is padding)
        unsigned long long m[kRgDocs];
        double x[kRgDocs];
        uint32_t mp = 0;  // bit j: doc j has a metric value
        uint32_t ok = 0;  // bit j: doc j is inside the segment and accepted
#pragma unroll
        for (uint32_t q = 0; q < kRgQuads; ++q) {
            const uint32_t doc0 = base + q * kRgQuad + threadIdx.x * 4;
            uint32_t o = 0xFu;
            if (P.accept) o &= bits4(P.accept, doc0);
            const uint32_t left = doc0 < P.n_docs ? P.n_docs - doc0 : 0u;
            if (left < 4) o &= (1u << left) - 1u;
            ok |= o << (4 * q);
        }
#pragma unroll
        for (uint32_t j = 0; j < kRgDocs; ++j) m[j] = P.all_mask;
#pragma unroll 1
        for (uint32_t c = 0; c < P.n_cols; ++c) fl_column(S.tab, c, S.tab.col[c], base, m);
#pragma unroll
        for (uint32_t j = 0; j < kRgDocs; ++j) {
            const bool in = (ok >> j) & 1u;
            m[j] = in ? (m[j] ? m[j] : other) : 0ull;
        }
        if constexpr (MET > 0) {
#pragma unroll
            for (uint32_t q = 0; q < kRgQuads; ++q) {
                const uint32_t doc0 = base + q * kRgQuad + threadIdx.x * 4;
                long long mvv[4];
                load_i64x4((const int64_t*)P.mv, doc0, (int64_t*)mvv);
#pragma unroll
                for (uint32_t t = 0; t < 4; ++t)
                    x[4 * q + t] = P.mv_f64 ? bits_dbl((unsigned long long)mvv[t]) : (double)mvv[t];
                mp |= (P.mv_present ? bits4(P.mv_present, doc0) : 0xFu) << (4 * q);
            }
        }
        rg_accumulate<MET>(S.cells, m, x, mp, vcnt, lane0);
    }
    __syncthreads();
    rg_flush<MET>(S.cells, P, R, vcnt);
}

void launch_filters(const FiltersParams& p, int met, uint32_t grid, hipStream_t st) {
    switch (met) {
        case 0: hipLaunchKernelGGL((filters_kernel<0>), dim3(grid), dim3(kRgWG), 0, st, p); break;
        case 1: hipLaunchKernelGGL((filters_kernel<1>), dim3(grid), dim3(kRgWG), 0, st, p); break;
        case 2: hipLaunchKernelGGL((filters_kernel<2>), dim3(grid), dim3(kRgWG), 0, st, p); break;
        default: hipLaunchKernelGGL((filters_kernel<3>), dim3(grid), dim3(kRgWG), 0, st, p); break;
    }
}

int filters_occupancy(int met) {
    int n = 0;
    const hipError_t e = met == 0   ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, filters_kernel<0>, kRgWG, 0)
                         : met == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, filters_kernel<1>, kRgWG, 0)
                         : met == 2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, filters_kernel<2>, kRgWG, 0)
                                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, filters_kernel<3>, kRgWG, 0);
    return e == hipSuccess && n > 0 ? n : 1;
}

}  // namespace esgpu
