// esgpu_ranked_cells.hpp — what the two ranked-terms kernels (path 10) share: esgpu_ranked.hip, which streams a rank
// column and a metric column doc by doc, and esgpu_ranked_grouped.hip, which streams the collected prefix of
// rank-grouped zone blocks (es_group12.hpp).  Both keep collect_kernel's packed cells in LDS -- [W keys][K ranks]
// count << pk_shift | sum of deltas in lane-rotated copies cstride apart, one (min, max) delta pair per cell -- and
// share their carve (rk_cells), the flush of a window into the grid (rk_flush), the per-doc body for a block that is
// not a single key of the grid (rk_slow_quad), the parameter view (rk_again) and the columns' widths (rk_r4, rk_m8).
#pragma once
#include "es_pack12.hpp"
#include "esgpu_collect.hpp"

namespace esgpu {

#ifndef ESGPU_RK_WAVES  // waves per SIMD the register budget must allow (6: three 512-thread workgroups per CU)
#define ESGPU_RK_WAVES 6
#endif
#ifndef ESGPU_RK_NT  // the two streamed columns by non-temporal loads (0: plain loads, for A/B builds)
#define ESGPU_RK_NT 1
#endif
constexpr int kRkWG = 512;
// The kernel's parameters again, for the code off the fast path (the flush, the per-doc body): read through this view,
// a parameter is a scalar load where it is used.  Read through P, every parameter is loaded at the kernel's entry and
// stays in an SGPR across the block loop, and the ~45 of them pushed 26 scalars into VGPR lanes, written and read back
// in every block.  (RankedParams is the kernel's only argument: it starts the kernarg segment.  The empty asm keeps the
// compiler from recognising the pointer and hoisting the loads back to the entry.)
typedef const RankedParams __attribute__((address_space(4))) rk_params_c;
__device__ __forceinline__ rk_params_c* rk_again() {
    rk_params_c* q = (rk_params_c*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    return q;
}
// Two statements that hold the block loop's loads and waits where the source puts them (profiles/ranked_waits/isa.md).
// rk_pin: an empty statement the compiler moves no load across -- without it the reloads at the loop's bottom, which
// the prologue ends with as well, are merged and sunk to the loop's head, and the prologue's loads are reordered.
// rk_drain: a wait for every outstanding vector load, as the last statement of the per-doc body -- the wait insertion
// then knows that body's own loads have landed, and the single-key body that follows it on the static path is entered
// through a wait for its first buffer only, not through vmcnt(0).  (0x0F70: vmcnt 0, expcnt and lgkmcnt at their
// maximum, that is not waited for.  A wait written as inline assembly is not seen by that pass.)
__device__ __forceinline__ void rk_pin() { asm volatile(""); }
__device__ __forceinline__ void rk_drain() { __builtin_amdgcn_s_waitcnt(0x0F70); }
constexpr uint32_t kRkDocs = 8;                       // docs per thread per load (one 16-byte load per column)
constexpr uint32_t kRkStepDocs = kRkWG * kRkDocs;     // 4,096
static_assert(kBlockDocs == 2 * kRkStepDocs, "a zone block is two buffers of 8 docs per thread");

__device__ __forceinline__ u32x4_t rk_load16(const uint16_t* p) {
#if ESGPU_RK_NT
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
#else
    return load16(p);
#endif
}
__device__ __forceinline__ u32x2_t rk_load8(const uint8_t* p) {
#if ESGPU_RK_NT
    return __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
#else
    return load8(p);
#endif
}

// The rank column at its two widths (RW bytes per doc).  rk_r4: the ranks of 4 docs as loaded -- RW 1 one word of four
// bytes (0xFF: rank >= 255 or the missing ordinal), RW 2 two words of 16-bit halves (0xFFFF missing) -- either way a
// rank the kernel collects (< K <= kRankedMax = 128) reads the same.  rk_r8: a thread's 8 docs of one buffer, one
// 8-byte (RW 1) or 16-byte (RW 2) load.
template <int RW> struct rk_r4;
template <> struct rk_r4<1> {
    uint32_t a;
    __device__ __forceinline__ uint32_t at(uint32_t j) const { return (a >> (8u * j)) & 0xFFu; }
    __device__ __forceinline__ void unpack(uint32_t (&t)[4]) const {
        t[0] = a & 0xFFu; t[1] = (a >> 8) & 0xFFu; t[2] = (a >> 16) & 0xFFu; t[3] = a >> 24;
    }
};
template <> struct rk_r4<2> {
    uint32_t a, b;
    __device__ __forceinline__ uint32_t at(uint32_t j) const { return ((j < 2 ? a : b) >> ((j & 1u) * 16u)) & 0xFFFFu; }
    __device__ __forceinline__ void unpack(uint32_t (&t)[4]) const {
        t[0] = a & 0xFFFFu; t[1] = a >> 16; t[2] = b & 0xFFFFu; t[3] = b >> 16;
    }
};
template <int RW> struct rk_r8;
template <> struct rk_r8<1> {
    u32x2_t v;
    __device__ __forceinline__ void load(const void* col, size_t doc) { v = rk_load8((const uint8_t*)col + doc); }
    __device__ __forceinline__ rk_r4<1> lo() const { return {v.x}; }
    __device__ __forceinline__ rk_r4<1> hi() const { return {v.y}; }
};
template <> struct rk_r8<2> {
    u32x4_t v;
    __device__ __forceinline__ void load(const void* col, size_t doc) { v = rk_load16((const uint16_t*)col + doc); }
    __device__ __forceinline__ rk_r4<2> lo() const { return {v.x, v.y}; }
    __device__ __forceinline__ rk_r4<2> hi() const { return {v.z, v.w}; }
};

// The metric deltas at their two widths (MW bits per doc).  rk_m8: a thread's 8 docs of one buffer -- MW 16 one 16-byte
// load of d16, MW 12 the three words of d12's group (es_pack12.hpp: one 12-byte load, 4-byte aligned).  quad(h, d): the
// deltas of docs 4 h .. 4 h + 3; pair(i): a word holding docs 2 i and 2 i + 1 -- doc j's delta is
// (pair >> (even + (j & 1) * step)) & mask, which is how the per-doc body takes it.
typedef unsigned int u32x3_t __attribute__((ext_vector_type(3)));
typedef u32x3_t u32x3_a4_t __attribute__((aligned(4)));
template <int MW> struct rk_m8;
template <> struct rk_m8<16> {
    u32x4_t v;
    __device__ __forceinline__ void load(const void* col, size_t doc) { v = rk_load16((const uint16_t*)col + doc); }
    static constexpr uint32_t even = 0, step = 16, mask = 0xFFFFu;
    __device__ __forceinline__ uint32_t pair(int i) const { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
    __device__ __forceinline__ void quad(int h, uint32_t (&d)[4]) const {
        const uint32_t m0 = pair(2 * h), m1 = pair(2 * h + 1);
        d[0] = m0 & 0xFFFFu; d[1] = m0 >> 16; d[2] = m1 & 0xFFFFu; d[3] = m1 >> 16;
    }
};
template <> struct rk_m8<12> {
    u32x3_t v;
    static constexpr uint32_t even = kP12Even, step = kP12Odd - kP12Even, mask = kP12Mask;
    __device__ __forceinline__ void load(const void* col, size_t doc) {  // doc: a multiple of kP12Group, 1.5 bytes each
        const u32x3_a4_t* const p = reinterpret_cast<const u32x3_a4_t*>((const uint8_t*)col + doc + (doc >> 1));
#if ESGPU_RK_NT
        v = __builtin_nontemporal_load(p);
#else
        v = *p;
#endif
    }
    __device__ __forceinline__ uint32_t pair(int i) const { return p12_window(v.x, v.y, v.z, i); }
    __device__ __forceinline__ void quad(int h, uint32_t (&d)[4]) const {
        const uint32_t x0 = p12_window(v.x, v.y, v.z, 2 * h), x1 = p12_window(v.x, v.y, v.z, 2 * h + 1);
        d[0] = p12_even(x0); d[1] = p12_odd(x0); d[2] = p12_even(x1); d[3] = p12_odd(x1);
    }
};
static_assert(kRkDocs == kP12Group, "a thread's 8 docs of a buffer are one group of d12");

// The LDS carve of collect_kernel's packed cells (collect_lds_bytes(pi = true)) and its reset: pk the packed words of
// the ncp copies (CS > C words each: cell C of every copy is spare), mm the (min, max) pairs; the pair of the spare cell
// lies in what is there the threads' spare words, and is (0, ~0): it never moves.
struct rk_cells {
    unsigned long long* pk;
    uint32_t* mm;
    uint32_t coff;  // the lane's copy
};
template <int MET>
__device__ __forceinline__ rk_cells rk_carve(unsigned char* smem, uint32_t C, uint32_t CS, uint32_t ncp) {
    rk_cells c;
    c.pk = (unsigned long long*)smem;
    c.mm = (uint32_t*)(smem + ((8 * (size_t)CS * ncp + 15) & ~(size_t)15));
    c.coff = ((threadIdx.x & 63) % ncp) * CS;
    for (uint32_t i = threadIdx.x; i < CS * ncp; i += kRkWG) c.pk[i] = 0;
    if constexpr (MET >= 2) {
        for (uint32_t i = threadIdx.x; i < C; i += kRkWG) { c.mm[2 * i] = ~0u; c.mm[2 * i + 1] = 0u; }
        if (threadIdx.x == 0) { c.mm[2 * C] = 0u; c.mm[2 * C + 1] = ~0u; }
    }
    __syncthreads();
    return c;
}

// the window's cells into the grid, as flush_window_pi: exact integer sums (count * base + sum of deltas; compensated
// when g_sum_lo is set), order-preserving extrema, a cell's words read and reset before its atomics are issued
template <int MET>
__device__ __forceinline__ void rk_flush(unsigned long long* pk, uint32_t* mm, uint32_t C, uint32_t K, uint32_t CS,
                                         uint32_t ncp, uint32_t sh, uint32_t win0) {
    const auto& Q = *rk_again();
    __syncthreads();
    const unsigned long long mask = (1ull << sh) - 1ull;
    for (uint32_t c = threadIdx.x; c < C; c += kRkWG) {
        unsigned long long n = 0;
        for (uint32_t k = 0; k < ncp; ++k) n += pk[k * CS + c];
        if (n == 0) continue;
        const uint32_t local = c / K;
        const uint32_t t = c - local * K;
        const uint32_t slot = win0 + local;
        if (slot >= Q.H) continue;
        const size_t g = (size_t)slot * Q.T_full + Q.rank_ord[t];
        const unsigned long long cnt = n >> sh;
        uint32_t lo = 0, hi = 0;
        if constexpr (MET >= 2) {
            const u32x2_t m = *reinterpret_cast<const u32x2_t*>(mm + 2 * c);
            lo = m.x;
            hi = m.y;
            u32x2_t r;
            r.x = ~0u;
            r.y = 0u;
            *reinterpret_cast<u32x2_t*>(mm + 2 * c) = r;
        }
        atomicAdd(&Q.g_cnt[g], cnt);
        for (uint32_t k = 0; k < ncp; ++k) pk[k * CS + c] = 0;
        const long long isum = (long long)(n & mask) + (long long)cnt * Q.mv_base;
        if (Q.g_sum_lo) {
            double xh, xl;
            i64_to_dd(isum, xh, xl);
            dd_atomic_add(&Q.g_sum[g], Q.g_sum_lo + g, xh, xl);
        } else {
            atomicAdd(&Q.g_sum[g], (double)isum);
        }
        if constexpr (MET >= 2) {
            atomicMin(&Q.g_min[g], sortable((double)(Q.mv_base + (int64_t)lo)));
            atomicMax(&Q.g_max[g], sortable((double)(Q.mv_base + (int64_t)hi)));
        }
    }
    __syncthreads();
}

// any block, doc by doc: 4 docs of the thread (docs doc0 .. doc0 + 3, their ranks and metric words as the caller holds
// them, the metric as rk_m8's pair words) with their keys by the block-delta unpack, slots by the magic division of the
// value's distance from the block's first key (the zone map bounds the block's values, so the distance is non-negative
// and below the block's keys x interval; a block spanning 2^32 or more divides in 64 bits).  Docs inside the window
// (wn keys from win0; wn 0: no window yet) go to the LDS cells, the rest to the grid by global atomics.
template <int MET, int RW, int MW>
__device__ __forceinline__ void rk_slow_quad(uint32_t doc0, rk_r4<RW> r, uint32_t m0, uint32_t m1, int64_t kmn, int64_t kmx,
                                             uint32_t K, uint32_t win0, uint32_t wn, unsigned long long* pk, uint32_t* mm,
                                             uint32_t coff, uint32_t sh) {
    const auto& Q = *rk_again();
    const int64_t vb = (Q.key0 + kmn) * Q.interval + Q.offset;  // the first instant of key kmn
    const bool d32 = kmx - kmn < (int64_t)Q.keys32;            // the block's keys x interval < 2^32
    if (doc0 < Q.n_docs) {
        const uint32_t nd = min(Q.n_docs - doc0, 4u);
        const u32x2_t tw = load8(Q.hv16 + doc0);
        const uint32_t hb = *reinterpret_cast<const uint32_t*>(Q.hv8 + (doc0 & Q.hv8_mask)) & (Q.hv8_and * 0x01010101u);
        const u32x2_t bw = load8(Q.hv16_base + (doc0 >> kB16Shift));
        const int64_t b = (int64_t)join64(bw.x, bw.y);
#pragma unroll 1
        for (uint32_t j = 0; j < nd; ++j) {
            const uint32_t m2 = j < 2 ? m0 : m1, t2 = j < 2 ? tw.x : tw.y;
            const uint32_t hs = (j & 1u) * 16u;
            const uint32_t t = r.at(j), dv = (m2 >> (rk_m8<MW>::even + (j & 1u) * rk_m8<MW>::step)) & rk_m8<MW>::mask;
            if (t >= K) continue;
            const int64_t v = b + (int64_t)(((t2 >> hs) & 0xFFFFu) | (((hb >> (8u * j)) & 0xFFu) << 16));
            const int64_t k = d32 ? kmn + (int64_t)magic_div((uint32_t)((uint64_t)v - (uint64_t)vb), Q.mg_m, Q.mg_s1,
                                                             Q.mg_s2, (uint32_t)Q.interval)
                                  : floor_div64(v - Q.offset, Q.interval) - Q.key0;
            if ((uint64_t)k >= (uint64_t)Q.H) continue;
            const uint32_t sl = (uint32_t)k - win0;
            if (sl < wn) {
                const uint32_t c = sl * K + t;
                atomicAdd(&pk[c + coff], (1ull << sh) + dv);
                if constexpr (MET >= 2) {
                    const u32x2_t m = *reinterpret_cast<const u32x2_t*>(mm + 2 * c);
                    if ((dv < m.x) | (dv > m.y)) {
                        atomicMin(&mm[2 * c], dv);
                        atomicMax(&mm[2 * c + 1], dv);
                    }
                }
            } else {  // outside the window: the doc's grid cell, as the generic kernel's global-grid path
                const size_t g = (size_t)k * Q.T_full + Q.rank_ord[t];
                atomicAdd(&Q.g_cnt[g], 1ull);
                const double x = (double)(Q.mv_base + (int64_t)dv);
                dd_atomic_add(&Q.g_sum[g], Q.g_sum_lo ? Q.g_sum_lo + g : nullptr, x);
                if constexpr (MET >= 2) {
                    const unsigned long long e = sortable(x);
                    if (e < Q.g_min[g]) atomicMin(&Q.g_min[g], e);
                    if (e > Q.g_max[g]) atomicMax(&Q.g_max[g], e);
                }
            }
        }
    }
}

}  // namespace esgpu
