// esgpu_mask_docs.hpp — the two sources of a doc's bucket mask, shared by the metric-only collects (esgpu_range.hip,
// path 11; esgpu_filters.hip, path 12) and their keyed form (esgpu_mask_hist.hip, path 13): the tables in LDS, their
// staging, and one round's docs -- masks, metric values, metric-present bits -- into a thread's registers.
// (filters_kernel uses FlTab and fl_column and keeps its own copy of fl_stage's and fl_docs' few lines: see there.)
#pragma once
#include "esgpu_range_cells.hpp"

namespace esgpu {

// ---- a range field: RangeParams.table ---------------------------------------------------------------------------------
struct RgTab {
    long long cuts[kRangeCuts];
    unsigned long long masks[kRangeCuts + 1];
};

// (before a __syncthreads)
__device__ __forceinline__ void rg_stage(RgTab& T, const uint64_t* table, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += kRgWG) T.cuts[i] = (long long)table[i];
    for (uint32_t i = threadIdx.x; i <= n; i += kRgWG) T.masks[i] = table[kRangeCuts + i];
}

// a value's mask (rg_key puts -0.0 just below +0.0: the host's cut for a bound of 0.0 is the key of -0.0)
template <bool F64>
__device__ __forceinline__ unsigned long long rg_value_mask(const RgTab& T, uint32_t n, uint32_t step0, unsigned long long bits) {
    if (F64) {
        const double d = bits_dbl(bits);
        if (!(d < INFINITY)) return 0ull;  // NaN >= from and +Infinity < to are false for every range
        return rg_lookup(T.cuts, T.masks, n, step0, rg_key(bits));
    }
    return rg_lookup(T.cuts, T.masks, n, step0, (long long)bits);
}

// one round of a single-valued range field: 4 consecutive docs per quad, every column by 16-byte loads (the columns,
// present bitsets and the doc bitset are allocated over whole zone blocks; what lies past n_docs is masked here)
template <int MET>
__device__ __forceinline__ void rg_docs(const RgTab& T, const RangeParams& P, uint32_t n, uint32_t step0, uint32_t base,
                                        unsigned long long (&m)[kRgDocs], double (&x)[kRgDocs], uint32_t& mp) {
    long long rv[kRgDocs], mvv[kRgDocs];
    uint32_t ok = 0;
#pragma unroll
    for (uint32_t q = 0; q < kRgQuads; ++q) {
        const uint32_t doc0 = base + q * kRgQuad + threadIdx.x * 4;
        load_i64x4((const int64_t*)P.rv, doc0, (int64_t*)&rv[4 * q]);
        if constexpr (MET > 0) load_i64x4((const int64_t*)P.mv, doc0, (int64_t*)&mvv[4 * q]);
        uint32_t o = 0xFu;
        if (P.accept) o &= bits4(P.accept, doc0);
        if (P.rv_present) o &= bits4(P.rv_present, doc0);
        const uint32_t left = doc0 < P.n_docs ? P.n_docs - doc0 : 0u;
        if (left < 4) o &= (1u << left) - 1u;
        ok |= o << (4 * q);
        if constexpr (MET > 0) mp |= (P.mv_present ? bits4(P.mv_present, doc0) : 0xFu) << (4 * q);
    }
#pragma unroll
    for (uint32_t j = 0; j < kRgDocs; ++j) {
        const unsigned long long vm = P.rv_f64 ? rg_value_mask<true>(T, n, step0, (unsigned long long)rv[j])
                                               : rg_value_mask<false>(T, n, step0, (unsigned long long)rv[j]);
        m[j] = ((ok >> j) & 1u) ? vm : 0ull;
        if constexpr (MET > 0) x[j] = P.mv_f64 ? bits_dbl((unsigned long long)mvv[j]) : (double)mvv[j];
    }
}

// ---- the clause columns of a filters aggregation: FiltersParams.table -----------------------------------------------
struct FlTab {
    long long cuts[kFilterCols][kRangeCuts];
    unsigned long long masks[kFilterCols][kRangeCuts + 1];
    unsigned long long no_value[kFilterCols];
    FilterCol col[kFilterCols];
};

// (before a __syncthreads)
__device__ __forceinline__ void fl_stage(FlTab& S, const FiltersParams& P) {
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
}

// one clause column into the 8 masks of a thread's docs: every load unconditional (the columns and present bitsets are
// allocated over whole zone blocks; what lies past n_docs is masked by the caller)
__device__ __forceinline__ void fl_column(const FlTab& S, uint32_t c, const FilterCol& C, uint32_t base,
                                          unsigned long long (&m)[kRgDocs]) {
    const long long* cuts = S.cuts[c];
    const unsigned long long* masks = S.masks[c];
    const unsigned long long none = S.no_value[c];
    const uint32_t n = C.n_cuts;
    uint32_t step0 = 0;
    if (n) step0 = 1u << (31 - __clz((int)n));
    if (C.kind == FCOL_ORD) {
#pragma unroll
        for (uint32_t q = 0; q < kRgQuads; ++q) {
            const uint32_t doc0 = base + q * kRgQuad + threadIdx.x * 4;
            uint32_t o[4];
            load_u32x4((const uint32_t*)C.v, doc0, o);
            const uint32_t pr = C.present ? bits4(C.present, doc0) : 0xFu;
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                const bool has = ((pr >> t) & 1u) && o[t] != kMissingOrd;
                const unsigned long long vm = rg_lookup(cuts, masks, n, step0, (long long)o[t]);
                m[4 * q + t] &= has ? vm : none;
            }
        }
    } else {
        const bool f64 = C.kind == FCOL_F64;
#pragma unroll
        for (uint32_t q = 0; q < kRgQuads; ++q) {
            const uint32_t doc0 = base + q * kRgQuad + threadIdx.x * 4;
            long long v[4];
            load_i64x4((const int64_t*)C.v, doc0, (int64_t*)v);
            const uint32_t pr = C.present ? bits4(C.present, doc0) : 0xFu;
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                const double d = bits_dbl((unsigned long long)v[t]);
                const bool has = ((pr >> t) & 1u) && !(f64 && d != d);  // NaN satisfies no comparison
                const long long key = f64 ? rg_key((unsigned long long)v[t]) : v[t];
                const unsigned long long vm = rg_lookup(cuts, masks, n, step0, key);
                m[4 * q + t] &= has ? vm : none;
            }
        }
    }
}

// one round of a filters aggregation's docs; other: the other bucket's bit (0: none)
template <int MET>
__device__ __forceinline__ void fl_docs(const FlTab& S, const FiltersParams& P, unsigned long long other, uint32_t base,
                                        unsigned long long (&m)[kRgDocs], double (&x)[kRgDocs], uint32_t& mp) {
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
    // the clause columns one after another: a rolled loop (the descriptors in LDS), so that one column's values are
    // live at a time
#pragma unroll 1
    for (uint32_t c = 0; c < P.n_cols; ++c) fl_column(S, c, S.col[c], base, m);
#pragma unroll
    for (uint32_t j = 0; j < kRgDocs; ++j) {
        const bool in = (ok >> j) & 1u;
        m[j] = in ? (m[j] ? m[j] : other) : 0ull;
    }
    // the metric column after the clause columns: its 8 values are not live while the masks are made (loaded before
    // them, MET 1 / 2 took 86 VGPRs, 5 waves per SIMD, against 72 / 80 and 7 / 6 this way)
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
}

}  // namespace esgpu
