// esgpu_range_cells.hpp — what the range collect (esgpu_range.hip, path 11), the filters collect (esgpu_filters.hip,
// path 12) and their keyed form (esgpu_mask_hist.hip, path 13) share: a doc's buckets are a u64 mask, a thread holds 8
// docs (masks and metric values) in registers, and from the masks on the kernels accumulate alike.  For every bucket
// present in the wave the wave reduces first -- ballots for the counts, wave_sum_f64 / wave_min_u64 / wave_max_u64 for
// the metric (rg_reduce) -- and lane 0 updates the workgroup's LDS cell of that bucket once.  The cells reach the grid
// in one flush per workgroup (path 13: per key the workgroup meets), one atomic per non-empty cell and array
// (compensated where the pipeline's double-double rule is on).  No global atomic and no LDS atomic per doc.
#pragma once
#include "esgpu_collect.hpp"

namespace esgpu {

constexpr int kRgWG = 256;
constexpr uint32_t kRgQuad = kRgWG * 4;        // docs of one 16-byte-per-lane sweep of the workgroup (two loads per column)
constexpr uint32_t kRgQuads = 2;               // sweeps per reduction round
constexpr uint32_t kRgDocs = 4 * kRgQuads;     // docs per thread per round
constexpr uint32_t kRgRound = kRgQuad * kRgQuads;
static_assert(kBlockDocs % kRgRound == 0, "a zone block is a whole number of rounds");

// a workgroup's cells, one per bucket
struct RgCells {
    unsigned long long cnt[kRangeMax], vcnt[kRangeMax];
    double sum[kRangeMax];
    unsigned long long mn[kRangeMax], mx[kRangeMax];
    double sq[kRangeMax];
};

__device__ __forceinline__ void rg_cells_init(RgCells& C) {
    for (uint32_t i = threadIdx.x; i < kRangeMax; i += kRgWG) {
        C.cnt[i] = 0;
        C.vcnt[i] = 0;
        C.sum[i] = 0.0;
        C.mn[i] = kMinInit;
        C.mx[i] = kMaxInit;
        C.sq[i] = 0.0;
    }
}

// the signed key doubles compare by (-0.0 just below +0.0)
__device__ __forceinline__ long long rg_key(unsigned long long bits) {
    const long long b = (long long)bits;
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFll);
}

// mask of a key: masks[k], k = the number of cuts <= key (the largest k in [0, n] with cuts[k - 1] <= key); step0 = the
// largest power of two <= n (0 for n = 0)
__device__ __forceinline__ unsigned long long rg_lookup(const long long* cuts, const unsigned long long* masks, uint32_t n,
                                                        uint32_t step0, long long key) {
    uint32_t k = 0;
    for (uint32_t step = step0; step; step >>= 1) {
        const uint32_t t = k + step;
        if (t <= n && cuts[t - 1] <= key) k = t;
    }
    return masks[k];
}

__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// a wave's part of one bucket in one round
struct RgPart {
    uint32_t c, vc;
    double s, sq;
    unsigned long long mn, mx;
};

// bucket r over the wave's docs of one round: m[j] the buckets of doc j, x[j] its metric value, bit j of mp: it has one.
// (What rg_accumulate below does per bucket, for the keyed kernel's straight-to-grid parts; rg_accumulate keeps its own
// copy of the loop -- calling this from it cost range_kernel's stats instantiation 5 VGPRs and a wave per SIMD.)
template <int MET>
__device__ __forceinline__ RgPart rg_reduce(const unsigned long long (&m)[kRgDocs], const double (&x)[kRgDocs], uint32_t mp,
                                            bool vcnt, uint32_t r) {
    uint32_t c = 0, vc = 0;
    double s = 0.0, sq = 0.0;
    unsigned long long mn = kMinInit, mx = kMaxInit;
#pragma unroll
    for (uint32_t j = 0; j < kRgDocs; ++j) {
        const bool in = (m[j] >> r) & 1ull;
        c += __popcll(__ballot(in));
        if constexpr (MET > 0) {
            const bool has = in && ((mp >> j) & 1u);
            if (vcnt) vc += __popcll(__ballot(has));
            s += has ? x[j] : 0.0;
            if constexpr (MET >= 2) {
                const bool nan = x[j] != x[j];
                const unsigned long long e = sortable(x[j]);
                const unsigned long long emn = nan ? 0ull : e, emx = nan ? ~0ull : e;
                if (has && emn < mn) mn = emn;
                if (has && emx > mx) mx = emx;
            }
            if constexpr (MET >= 3) sq += has ? x[j] * x[j] : 0.0;  // (sumOfSqr += value * value, no FMA)
        }
    }
    if constexpr (MET > 0) {
        s = wave_sum_f64(s);
        if constexpr (MET >= 2) {
            mn = wave_min_u64(mn);
            mx = wave_max_u64(mx);
        }
        if constexpr (MET >= 3) sq = wave_sum_f64(sq);
    }
    return RgPart{c, vc, s, sq, mn, mx};
}

// one round's docs into the workgroup's cells: m[j] the buckets of doc j, x[j] its metric value, bit j of mp: it has one
template <int MET>
__device__ __forceinline__ void rg_accumulate(RgCells& C, const unsigned long long (&m)[kRgDocs], const double (&x)[kRgDocs],
                                              uint32_t mp, bool vcnt, bool lane0) {
    unsigned long long any = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < kRgDocs; ++j) any |= m[j];
    any = wave_or_u64(any);
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)any), hi = __builtin_amdgcn_readfirstlane((uint32_t)(any >> 32));
    // one pass per bucket present in the wave (uniform)
    while (lo | hi) {
        uint32_t r;
        if (lo) { r = __builtin_ctz(lo); lo &= lo - 1u; }
        else { r = 32u + __builtin_ctz(hi); hi &= hi - 1u; }
        uint32_t c = 0, vc = 0;
        double s = 0.0, sq = 0.0;
        unsigned long long mn = kMinInit, mx = kMaxInit;
#pragma unroll
        for (uint32_t j = 0; j < kRgDocs; ++j) {
            const bool in = (m[j] >> r) & 1ull;
            c += __popcll(__ballot(in));
            if constexpr (MET > 0) {
                const bool has = in && ((mp >> j) & 1u);
                if (vcnt) vc += __popcll(__ballot(has));
                s += has ? x[j] : 0.0;
                if constexpr (MET >= 2) {
                    const bool nan = x[j] != x[j];
                    const unsigned long long e = sortable(x[j]);
                    const unsigned long long emn = nan ? 0ull : e, emx = nan ? ~0ull : e;
                    if (has && emn < mn) mn = emn;
                    if (has && emx > mx) mx = emx;
                }
                if constexpr (MET >= 3) sq += has ? x[j] * x[j] : 0.0;  // (sumOfSqr += value * value, no FMA)
            }
        }
        if constexpr (MET > 0) {
            s = wave_sum_f64(s);
            if constexpr (MET >= 2) {
                mn = wave_min_u64(mn);
                mx = wave_max_u64(mx);
            }
            if constexpr (MET >= 3) sq = wave_sum_f64(sq);
        }
        if (lane0) {
            atomicAdd(&C.cnt[r], (unsigned long long)c);
            if constexpr (MET > 0) {
                if (vcnt) atomicAdd(&C.vcnt[r], (unsigned long long)vc);
                atomicAdd(&C.sum[r], s);
                if constexpr (MET >= 2) {
                    atomicMin(&C.mn[r], mn);
                    atomicMax(&C.mx[r], mx);
                }
                if constexpr (MET >= 3) atomicAdd(&C.sq[r], sq);
            }
        }
    }
}

// one cell's part into grid cell g (P.g_*): one atomic per array
template <int MET, class PARAMS>
__device__ __forceinline__ void rg_to_grid(const PARAMS& P, size_t g, unsigned long long cnt, unsigned long long vc, double sum,
                                           unsigned long long mn, unsigned long long mx, double sq, bool vcnt) {
    atomicAdd(&P.g_cnt[g], cnt);
    if constexpr (MET > 0) {
        const bool some = !vcnt || vc != 0;  // (docs of the bucket, none with a metric value: nothing to add)
        if (vcnt && some) atomicAdd(&P.g_vcnt[g], vc);
        if (some) {
            dd_atomic_add(&P.g_sum[g], P.g_sum_lo ? P.g_sum_lo + g : nullptr, sum);
            if constexpr (MET >= 2) {
                if (mn != kMinInit) atomicMin(&P.g_min[g], mn);
                if (mx != kMaxInit) atomicMax(&P.g_max[g], mx);
            }
            if constexpr (MET >= 3) dd_atomic_add(&P.g_sq[g], P.g_sq_lo ? P.g_sq_lo + g : nullptr, sq);
        }
    }
}

// the workgroup's cells into row `row` of the grid (R cells a row): one atomic per non-empty cell and array; after a
// __syncthreads
template <int MET, class PARAMS>
__device__ __forceinline__ void rg_flush(const RgCells& C, const PARAMS& P, uint32_t R, bool vcnt, size_t row = 0) {
    const uint32_t r = threadIdx.x;
    if (r < R && C.cnt[r] != 0) rg_to_grid<MET>(P, row * R + r, C.cnt[r], C.vcnt[r], C.sum[r], C.mn[r], C.mx[r], C.sq[r], vcnt);
}

}  // namespace esgpu
