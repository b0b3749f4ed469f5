// esgpu_mask_hist.hip — a date_histogram under a range or a filters aggregation (collect path 13): one pass over the
// mask's columns, one metric field and -- where a zone block spans several keys -- the timestamps, into the [H][R] cells
// of a pipeline's ordinary grid (row = histogram key, column = bucket).
//
// A doc's buckets are the u64 mask of the range collect (path 11) or the filters collect (path 12), made by the same
// code (esgpu_mask_docs.hpp).  The key dimension comes from the timestamp column's zone maps, rounded once per segment
// into grid rows (HistKeys.zkey, launch_zone_keys):
//   - the workgroup's LDS cells stand for a window of kMhSlots consecutive grid rows at a time.  When a block's rows do
//     not lie inside the window (uniform across the workgroup) the cells are flushed to their rows, start again, and the
//     window moves to the block's first row.
//   - a block whose range rounds to one key reads no timestamp.  Its docs are accumulated exactly as paths 11 / 12 do,
//     into the cells of its row.  On time-ordered data this is nearly every block.
//   - a block that spans several keys reads its timestamps (16-byte loads, like the other columns) and rounds them -- a
//     32-bit magic division relative to the block's first key where the block's span allows, the 64-bit division or the
//     table search otherwise.  Each wave then walks the distinct rows among its docs in ascending order (a wave-wide
//     minimum per step, so the walk is as long as the wave has keys: two or three on jittered data, hundreds on unordered
//     data), masks the docs' bucket words to the row's, and reduces as above; lane 0 adds the wave's part to the row's
//     LDS cells when the row is in the window (jittered data: a block's two or three keys always are) and straight to
//     the grid cell otherwise -- one global atomic per wave, row, bucket and array, none per doc.  There is no third
//     path and so no threshold between two.
//   - a doc of a bucket without a timestamp (a clear present bit, a block or a segment without values) counts in the
//     bucket's doc count (g_ocnt) and in no row; every other doc counts in both.
#include "esgpu_mask_docs.hpp"

namespace esgpu {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;
constexpr uint32_t kMhSlots = 4;  // grid rows the LDS cells stand for at a time (12 KB of cells)

// the source of the masks: its LDS tables, what staging leaves in registers, and one round's docs
template <class PARAMS>
struct MhSrc;
template <>
struct MhSrc<RangeParams> {
    using Tab = RgTab;
    struct Regs { uint32_t n, step0; };
    static __device__ __forceinline__ Regs stage(Tab& T, const RangeParams& P) {
        rg_stage(T, P.table, P.n_cuts);
        uint32_t step0 = 0;
        if (P.n_cuts) step0 = 1u << (31 - __clz((int)P.n_cuts));
        return Regs{P.n_cuts, step0};
    }
    template <int MET>
    static __device__ __forceinline__ void docs(const Tab& T, const RangeParams& P, const Regs& g, uint32_t base,
                                                unsigned long long (&m)[kRgDocs], double (&x)[kRgDocs], uint32_t& mp) {
        rg_docs<MET>(T, P, g.n, g.step0, base, m, x, mp);
    }
};
template <>
struct MhSrc<FiltersParams> {
    using Tab = FlTab;
    struct Regs { unsigned long long other; };
    static __device__ __forceinline__ Regs stage(Tab& T, const FiltersParams& P) {
        fl_stage(T, P);
        return Regs{P.other_bit >= 0 ? 1ull << P.other_bit : 0ull};
    }
    template <int MET>
    static __device__ __forceinline__ void docs(const Tab& T, const FiltersParams& P, const Regs& g, uint32_t base,
                                                unsigned long long (&m)[kRgDocs], double (&x)[kRgDocs], uint32_t& mp) {
        fl_docs<MET>(T, P, g.other, base, m, x, mp);
    }
};

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// grid row of a timestamp (key_index of the cell-grid collects over HistKeys); outside [0, H): kNoRow
__device__ __forceinline__ uint32_t mh_row(const HistKeys& K, int64_t v) {
    int64_t k;
    if (!K.kstart) {
        k = floor_div64(v - K.offset, K.interval) - K.key0;
    } else {
        if (K.nsteps == 0 || v < K.kstart[0]) return kNoRow;
        uint32_t lo = 0, hi = K.nsteps;  // kstart[lo] <= v < kstart[hi] (kstart[nsteps] = +inf)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (K.kstart[mid] <= v) lo = mid; else hi = mid;
        }
        k = K.kslot ? K.kslot[lo] : lo;
    }
    return (uint64_t)k < (uint64_t)K.H ? (uint32_t)k : kNoRow;
}

// the docs of one round into the buckets' doc counts alone (docs without a timestamp)
__device__ __forceinline__ void mh_count(unsigned long long* ocnt, const unsigned long long (&m)[kRgDocs], bool lane0) {
    unsigned long long any = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < kRgDocs; ++j) any |= m[j];
    any = wave_or_u64(any);
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)any), hi = __builtin_amdgcn_readfirstlane((uint32_t)(any >> 32));
    while (lo | hi) {
        uint32_t r;
        if (lo) { r = __builtin_ctz(lo); lo &= lo - 1u; }
        else { r = 32u + __builtin_ctz(hi); hi &= hi - 1u; }
        uint32_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRgDocs; ++j) c += __popcll(__ballot((m[j] >> r) & 1ull));
        if (lane0) atomicAdd(&ocnt[r], (unsigned long long)c);
    }
}

// one round's docs of one grid row straight into the grid: the wave's part of every bucket present, one atomic per array
template <int MET, class PARAMS>
__device__ __forceinline__ void mh_accumulate_row(const PARAMS& P, unsigned long long* ocnt, uint32_t R, uint32_t row,
                                                  const unsigned long long (&m)[kRgDocs], const double (&x)[kRgDocs], uint32_t mp,
                                                  bool vcnt, bool lane0) {
    unsigned long long any = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < kRgDocs; ++j) any |= m[j];
    any = wave_or_u64(any);
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)any), hi = __builtin_amdgcn_readfirstlane((uint32_t)(any >> 32));
    while (lo | hi) {
        uint32_t r;
        if (lo) { r = __builtin_ctz(lo); lo &= lo - 1u; }
        else { r = 32u + __builtin_ctz(hi); hi &= hi - 1u; }
        const RgPart w = rg_reduce<MET>(m, x, mp, vcnt, r);
        if (lane0 && r < R) {
            rg_to_grid<MET>(P, (size_t)row * R + r, w.c, w.vc, w.s, w.mn, w.mx, w.sq, vcnt);
            atomicAdd(&ocnt[r], (unsigned long long)w.c);
        }
    }
}

// the workgroup's cells into grid rows w0 .. w0 + kMhSlots - 1 (a slot that holds something stands for a row below H) and
// the buckets' doc counts, and empty again; between two __syncthreads
template <int MET, class PARAMS>
__device__ __forceinline__ void mh_flush(RgCells (&C)[kMhSlots], unsigned long long* ocnt, const PARAMS& P, uint32_t R, bool vcnt,
                                         uint32_t w0) {
    const uint32_t r = threadIdx.x;
#pragma unroll 1
    for (uint32_t s = 0; s < kMhSlots; ++s) {
        rg_flush<MET>(C[s], P, R, vcnt, (size_t)w0 + s);
        if (r < kRangeMax && C[s].cnt[r] != 0) {
            ocnt[r] += C[s].cnt[r];
            C[s].cnt[r] = 0;
            C[s].vcnt[r] = 0;
            C[s].sum[r] = 0.0;
            C[s].mn[r] = kMinInit;
            C[s].mx[r] = kMaxInit;
            C[s].sq[r] = 0.0;
        }
    }
}

template <int MET, class PARAMS>
__global__ __launch_bounds__(kRgWG) void mask_hist_kernel(PARAMS P, HistKeys K) {
    using Src = MhSrc<PARAMS>;
    __shared__ typename Src::Tab tab;
    __shared__ RgCells cells[kMhSlots];
    __shared__ unsigned long long ocnt[kRangeMax];
    const typename Src::Regs src = Src::stage(tab, P);
#pragma unroll 1
    for (uint32_t s = 0; s < kMhSlots; ++s) rg_cells_init(cells[s]);
    for (uint32_t i = threadIdx.x; i < kRangeMax; i += kRgWG) ocnt[i] = 0;
    __syncthreads();

    const uint32_t R = P.R;
    const uint32_t b_begin = blockIdx.x * P.blocks_per_wg;
    const uint32_t b_end = min(b_begin + P.blocks_per_wg, P.n_blocks);
    const bool lane0 = (threadIdx.x & 63) == 0;
    const bool vcnt = MET > 0 && P.vcnt_mode != 0;
    const zkey_pair_c* const zk = zkey_view(K.zkey);
    uint32_t w0 = kNoRow;  // the LDS cells stand for grid rows w0 .. w0 + kMhSlots - 1

    for (uint32_t blk = b_begin; blk < b_end; ++blk) {
        if (blk * kBlockDocs >= P.n_docs) break;  // (uniform: the rest of the last block is padding)
        int64_t kmn = 1, kmx = 0;  // the block's rows (uniform; a scalar load)
        if (K.hv) {
            const i64x2_t z = zk[__builtin_amdgcn_readfirstlane(blk)];
            kmn = z.x;
            kmx = z.y;
        }
        const bool nokey = kmn > kmx;
        const bool single = kmn == kmx && (uint64_t)kmn < (uint64_t)K.H;
        // the window moves to a block whose rows it does not hold (a block of more than kMhSlots rows: to its first ones)
        // (a flag, the flush under it, then a select.  Written as `if (move) { if (w0 != kNoRow) flush; w0 = kmn; }` --
        // the same program -- hipcc of ROCm 7.2.0 (AMD clang 22.0.0git, roc-7.2.0) at -O3 for gfx950 set the window's
        // register to kmn only on the path where w0 was unset and kept the old w0 on the path through the flush, in all
        // eight instantiations: the next single-key block then indexed the cells past their end.  This form compiles to
        // an s_cselect after the second barrier.  tests/test_gpu_mask_block_carry.py walks that path; with a later
        // toolchain the plain form may be tried against it again.)
        const bool move = !nokey && (uint64_t)kmn < (uint64_t)K.H &&
                          (w0 == kNoRow || kmn < (int64_t)w0 || kmx >= (int64_t)w0 + (int64_t)kMhSlots);
        if (move && w0 != kNoRow) {
            __syncthreads();
            mh_flush<MET>(cells, ocnt, P, R, vcnt, w0);
            __syncthreads();
        }
        w0 = move ? (uint32_t)kmn : w0;
        // several keys: the magic division holds while every timestamp of the block is within 2^32 of its first key
        const bool fast = !nokey && kmn >= 0 && K.keys32 != 0 && (uint64_t)(kmx - kmn) < (uint64_t)K.keys32;
        const int64_t vb = (K.key0 + kmn) * K.interval + K.offset;

        for (uint32_t base = blk * kBlockDocs; base < (blk + 1) * kBlockDocs; base += kRgRound) {
            if (base >= P.n_docs) break;
            unsigned long long m[kRgDocs];
            double x[kRgDocs];
            uint32_t mp = 0;  // bit j: doc j has a metric value
            Src::template docs<MET>(tab, P, src, base, m, x, mp);
            if (nokey || K.hv_present) {  // (uniform) the docs without a timestamp: into their buckets' doc counts only
                uint32_t hp = 0;
                if (!nokey) {
#pragma unroll
                    for (uint32_t q = 0; q < kRgQuads; ++q)
                        hp |= bits4(K.hv_present, base + q * kRgQuad + threadIdx.x * 4) << (4 * q);
                }
                unsigned long long mm[kRgDocs];
#pragma unroll
                for (uint32_t j = 0; j < kRgDocs; ++j) {
                    const bool has = (hp >> j) & 1u;
                    mm[j] = has ? 0ull : m[j];
                    m[j] = has ? m[j] : 0ull;
                }
                mh_count(ocnt, mm, lane0);
                if (nokey) continue;
            }
            if (single) {
                rg_accumulate<MET>(cells[(uint32_t)kmn - w0], m, x, mp, vcnt, lane0);
                continue;
            }
            uint32_t row[kRgDocs];
#pragma unroll
            for (uint32_t q = 0; q < kRgQuads; ++q) {
                long long v[4];
                load_i64x4(K.hv, base + q * kRgQuad + threadIdx.x * 4, (int64_t*)v);
#pragma unroll
                for (uint32_t t = 0; t < 4; ++t) {
                    uint32_t rw;
                    if (fast) {
                        rw = (uint32_t)kmn + magic_div((uint32_t)((uint64_t)v[t] - (uint64_t)vb), K.mg_m, K.mg_s1, K.mg_s2,
                                                       (uint32_t)K.interval);
                        if (rw >= K.H) rw = kNoRow;
                    } else {
                        rw = mh_row(K, v[t]);
                    }
                    row[4 * q + t] = m[4 * q + t] ? rw : kNoRow;  // (a doc in no bucket, or without a value: its word is garbage)
                }
            }
            // the wave's distinct rows, ascending (uniform)
            for (uint32_t lo = 0;;) {
                uint32_t nx = kNoRow;
#pragma unroll
                for (uint32_t j = 0; j < kRgDocs; ++j)
                    if (row[j] >= lo && row[j] < nx) nx = row[j];
                nx = __builtin_amdgcn_readfirstlane(wave_min_u32(nx));
                if (nx == kNoRow) break;
                unsigned long long mk[kRgDocs];
#pragma unroll
                for (uint32_t j = 0; j < kRgDocs; ++j) mk[j] = row[j] == nx ? m[j] : 0ull;
                if (w0 != kNoRow && nx - w0 < kMhSlots) rg_accumulate<MET>(cells[nx - w0], mk, x, mp, vcnt, lane0);
                else mh_accumulate_row<MET>(P, ocnt, R, nx, mk, x, mp, vcnt, lane0);
                lo = nx + 1;
            }
        }
    }
    __syncthreads();
    if (w0 != kNoRow) mh_flush<MET>(cells, ocnt, P, R, vcnt, w0);
    if (threadIdx.x < R && ocnt[threadIdx.x] != 0) atomicAdd(&K.g_ocnt[threadIdx.x], ocnt[threadIdx.x]);
}

template <class PARAMS>
static void launch_mh(const PARAMS& p, const HistKeys& k, int met, uint32_t grid, hipStream_t st) {
    switch (met) {
        case 0: hipLaunchKernelGGL((mask_hist_kernel<0, PARAMS>), dim3(grid), dim3(kRgWG), 0, st, p, k); break;
        case 1: hipLaunchKernelGGL((mask_hist_kernel<1, PARAMS>), dim3(grid), dim3(kRgWG), 0, st, p, k); break;
        case 2: hipLaunchKernelGGL((mask_hist_kernel<2, PARAMS>), dim3(grid), dim3(kRgWG), 0, st, p, k); break;
        default: hipLaunchKernelGGL((mask_hist_kernel<3, PARAMS>), dim3(grid), dim3(kRgWG), 0, st, p, k); break;
    }
}
void launch_mask_hist(const RangeParams& p, const HistKeys& k, int met, uint32_t grid, hipStream_t st) { launch_mh(p, k, met, grid, st); }
void launch_mask_hist(const FiltersParams& p, const HistKeys& k, int met, uint32_t grid, hipStream_t st) { launch_mh(p, k, met, grid, st); }

template <class PARAMS>
static int occ_mh(int met) {
    int n = 0;
    const hipError_t e = met == 0   ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mask_hist_kernel<0, PARAMS>, kRgWG, 0)
                         : met == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mask_hist_kernel<1, PARAMS>, kRgWG, 0)
                         : met == 2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mask_hist_kernel<2, PARAMS>, kRgWG, 0)
                                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mask_hist_kernel<3, PARAMS>, kRgWG, 0);
    return e == hipSuccess && n > 0 ? n : 1;
}
int mask_hist_occupancy(int met, bool filters) { return filters ? occ_mh<FiltersParams>(met) : occ_mh<RangeParams>(met); }

}  // namespace esgpu
