// esgpu_range.hip — the range aggregation's collect (path 11, RangeAggregator.java:128-190): one pass over the range
// field and one metric field into the [R] cells of a pipeline's ordinary grid.
//
// A doc may fall into several ranges, so the bucket dimension is a u64 mask per doc instead of a cell index.  The host
// cuts the number line at the ranges' distinct finite bounds (RangeParams): a value's mask is the table entry of its
// elementary interval, found by a binary search over the cuts in LDS -- no loop over the ranges per value -- and a doc's
// mask is the OR over its values (a multi-valued doc counts once per range).  Values are compared as signed 64-bit keys:
// a long column against long cuts (the host made each the least long whose double reaches the bound), a double column
// through the order-preserving image of its bits (rg_key; NaN and +Infinity belong to no range).
//
// The tables and the single-valued round: esgpu_mask_docs.hpp (shared with the keyed form, esgpu_mask_hist.hip);
// accumulation and flush: esgpu_range_cells.hpp (shared with the filters collect too).
#include "esgpu_mask_docs.hpp"

namespace esgpu {

struct RgLds {
    RgTab tab;
    RgCells cells;
};

template <int MET, bool MULTI>
__global__ __launch_bounds__(kRgWG) void range_kernel(RangeParams P) {
    __shared__ RgLds S;
    const uint32_t n = P.n_cuts, R = P.R;
    rg_stage(S.tab, P.table, n);
    rg_cells_init(S.cells);
    __syncthreads();
    uint32_t step0 = 0;
    if (n) step0 = 1u << (31 - __clz((int)n));

    const uint32_t b_begin = blockIdx.x * P.blocks_per_wg;
    const uint32_t b_end = min(b_begin + P.blocks_per_wg, P.n_blocks);
    const bool lane0 = (threadIdx.x & 63) == 0;
    const bool vcnt = MET > 0 && P.vcnt_mode != 0;

    for (uint32_t base = b_begin * kBlockDocs; base < b_end * kBlockDocs; base += kRgRound) {
        if (base >= P.n_docs) break;  // (uniform: the rest of the last block is padding)
        unsigned long long m[kRgDocs];
        double x[kRgDocs];
        uint32_t mp = 0;  // bit j: doc j has a metric value
        if constexpr (!MULTI) {
            rg_docs<MET>(S.tab, P, n, step0, base, m, x, mp);
        } else {
            // multi-valued range field (CSR): one doc per lane and sweep, its values in a loop
#pragma unroll
            for (uint32_t j = 0; j < kRgDocs; ++j) {
                const uint32_t d = base + j * kRgWG + threadIdx.x;
                m[j] = 0ull;
                if constexpr (MET > 0) x[j] = 0.0;
                if (d >= P.n_docs) continue;
                if (P.accept && !((P.accept[d >> 6] >> (d & 63)) & 1ull)) continue;
                const unsigned long long* vals = (const unsigned long long*)P.rv;
                const uint64_t o1 = P.rv_off[d + 1];
                unsigned long long acc = 0ull;
                for (uint64_t o = P.rv_off[d]; o < o1; ++o)
                    acc |= P.rv_f64 ? rg_value_mask<true>(S.tab, n, step0, vals[o]) : rg_value_mask<false>(S.tab, n, step0, vals[o]);
                m[j] = acc;
                if constexpr (MET > 0) {
                    const long long raw = ((const long long*)P.mv)[d];
                    x[j] = P.mv_f64 ? bits_dbl((unsigned long long)raw) : (double)raw;
                    if (!P.mv_present || ((P.mv_present[d >> 6] >> (d & 63)) & 1ull)) mp |= 1u << j;
                }
            }
        }
        rg_accumulate<MET>(S.cells, m, x, mp, vcnt, lane0);
    }
    __syncthreads();
    rg_flush<MET>(S.cells, P, R, vcnt);
}

template <int MET>
static void launch_rg(const RangeParams& p, uint32_t grid, hipStream_t st) {
    if (p.rv_off) hipLaunchKernelGGL((range_kernel<MET, true>), dim3(grid), dim3(kRgWG), 0, st, p);
    else hipLaunchKernelGGL((range_kernel<MET, false>), dim3(grid), dim3(kRgWG), 0, st, p);
}
void launch_range(const RangeParams& p, int met, uint32_t grid, hipStream_t st) {
    switch (met) {
        case 0: launch_rg<0>(p, grid, st); break;
        case 1: launch_rg<1>(p, grid, st); break;
        case 2: launch_rg<2>(p, grid, st); break;
        default: launch_rg<3>(p, grid, st); break;
    }
}

template <int MET>
static hipError_t occ_rg(int* n, bool multi) {
    return multi ? hipOccupancyMaxActiveBlocksPerMultiprocessor(n, range_kernel<MET, true>, kRgWG, 0)
                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(n, range_kernel<MET, false>, kRgWG, 0);
}
int range_occupancy(int met, bool multi) {
    int n = 0;
    const hipError_t e = met == 0 ? occ_rg<0>(&n, multi) : met == 1 ? occ_rg<1>(&n, multi) : met == 2 ? occ_rg<2>(&n, multi)
                                                                                            : occ_rg<3>(&n, multi);
    return e == hipSuccess && n > 0 ? n : 1;
}

}  // namespace esgpu
