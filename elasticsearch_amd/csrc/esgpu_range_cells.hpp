// esgpu_range_cells.hpp — what the range collect (esgpu_range.hip, path 11) and the filters collect (esgpu_filters.hip,
// path 12) share: a doc's buckets are a u64 mask, a thread holds 8 docs (masks and metric values) in registers, and from
// the masks on both kernels accumulate alike.  For every bucket present in the wave the wave reduces first -- ballots
// for the counts, wave_sum_f64 / wave_min_u64 / wave_max_u64 for the metric -- and lane 0 updates the workgroup's LDS
// cell of that bucket once.  The cells reach the grid in one flush per workgroup, one atomic per non-empty cell and
// array (compensated where the pipeline's double-double rule is on).  No global atomic and no LDS atomic per doc.
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

// the workgroup's cells into the grid (P.g_*): one atomic per non-empty cell and array; after a __syncthreads
template <int MET, class PARAMS>
__device__ __forceinline__ void rg_flush(const RgCells& C, const PARAMS& P, uint32_t R, bool vcnt) {
    const uint32_t r = threadIdx.x;
    if (r < R && C.cnt[r] != 0) {
        atomicAdd(&P.g_cnt[r], C.cnt[r]);
        if constexpr (MET > 0) {
            const bool some = !vcnt || C.vcnt[r] != 0;  // (docs of the bucket, none with a metric value: nothing to add)
            if (vcnt && some) atomicAdd(&P.g_vcnt[r], C.vcnt[r]);
            if (some) {
                dd_atomic_add(&P.g_sum[r], P.g_sum_lo ? P.g_sum_lo + r : nullptr, C.sum[r]);
                if constexpr (MET >= 2) {
                    if (C.mn[r] != kMinInit) atomicMin(&P.g_min[r], C.mn[r]);
                    if (C.mx[r] != kMaxInit) atomicMax(&P.g_max[r], C.mx[r]);
                }
                if constexpr (MET >= 3) dd_atomic_add(&P.g_sq[r], P.g_sq_lo ? P.g_sq_lo + r : nullptr, C.sq[r]);
            }
        }
    }
}

}  // namespace esgpu
