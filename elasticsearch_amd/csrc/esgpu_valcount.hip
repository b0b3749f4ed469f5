// esgpu_valcount.hip — the per-doc value-count product: how many values each doc of a column holds, as one u16 per doc
// (ValueCountAggregator.collect adds values.count() per doc, A/metrics/valuecount/ValueCountAggregator.java:75-88).  A
// lone value_count leaf collects it as a dense 16-bit integer metric, so its sums are exact.  Three sources:
//   a single-valued ordinal column: 1 unless the ordinal is missing (u32 0xFFFFFFFF, or 0xFFFF in the 16-bit copy);
//   a present bitset: the doc's bit;
//   CSR offsets: off[d + 1] - off[d].
// A column that is dense and single-valued needs no product (the count is the doc count); value_counts_ones_kernel
// writes its all-ones product for the request whose earlier segments already took a product.
// Each thread owns 4 consecutive docs per step: 16-byte loads where the source is wide enough, one 8-byte store of four
// counts.  The loads are unconditional -- past the range they re-read the last group, which is never written -- so the
// compiler keeps them in flight across the range check.  No LDS.  The one atomic is the largest per-doc count, one
// atomicMax per wave that holds a value above the word it read: it becomes the product column's vmax, and a count
// above 65,535 refuses the request.
#include <algorithm>

#include "esgpu_kernels.hpp"

namespace esgpu {

namespace {

constexpr uint32_t kThreads = 256;

// how many of the docs [d0, d0 + 4) lie inside [0, n_docs), as a 4-bit mask (d0 is a multiple of 4)
__device__ inline uint32_t inside4(uint32_t d0, uint32_t n_docs) {
    return d0 + 4 <= n_docs ? 0xFu : d0 >= n_docs ? 0u : (1u << (n_docs - d0)) - 1u;
}

__device__ inline uint2 pack4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    return make_uint2(c0 | (c1 << 16), c2 | (c3 << 16));
}

// groups: n_pad / 4 (n_pad is a multiple of kBlockDocs); a thread past the range clamps to the last group
template <class ORD>
__global__ __launch_bounds__(kThreads) void value_counts_ord_kernel(const ORD* __restrict__ ord, uint32_t n_docs, uint32_t groups,
                                                                    uint16_t* __restrict__ out) {
    constexpr uint32_t kMissing = sizeof(ORD) == 2 ? 0xFFFFu : 0xFFFFFFFFu;
    for (uint32_t g0 = blockIdx.x * kThreads; g0 < groups; g0 += gridDim.x * kThreads) {
        const uint32_t g = g0 + threadIdx.x, gl = min(g, groups - 1), d0 = gl << 2;
        uint32_t o[4];
        if constexpr (sizeof(ORD) == 2) {
            const uint2 a = *reinterpret_cast<const uint2*>(ord + d0);
            o[0] = a.x & 0xFFFFu; o[1] = a.x >> 16; o[2] = a.y & 0xFFFFu; o[3] = a.y >> 16;
        } else {
            const uint4 a = *reinterpret_cast<const uint4*>(ord + d0);
            o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
        }
        const uint32_t in = inside4(d0, n_docs);
        if (g < groups)
            *reinterpret_cast<uint2*>(out + d0) = pack4((in & 1u) && o[0] != kMissing, ((in >> 1) & 1u) && o[1] != kMissing,
                                                        ((in >> 2) & 1u) && o[2] != kMissing, ((in >> 3) & 1u) && o[3] != kMissing);
    }
}

// a present bitset: one 64-bit word covers 16 groups (the word is re-read by the 16 threads that share it: one
// cache line per wave)
__global__ __launch_bounds__(kThreads) void value_counts_present_kernel(const uint64_t* __restrict__ present, uint32_t n_docs,
                                                                        uint32_t groups, uint16_t* __restrict__ out) {
    for (uint32_t g0 = blockIdx.x * kThreads; g0 < groups; g0 += gridDim.x * kThreads) {
        const uint32_t g = g0 + threadIdx.x, gl = min(g, groups - 1), d0 = gl << 2;
        // (the bitset has a word for every 64 docs of [0, n_docs); a group past it reads the last word)
        const uint32_t w = min(d0, n_docs ? n_docs - 1 : 0u) >> 6;
        const uint32_t bits = (uint32_t)(present[w] >> (d0 & 63)) & inside4(d0, n_docs);
        if (g < groups) *reinterpret_cast<uint2*>(out + d0) = pack4(bits & 1u, (bits >> 1) & 1u, (bits >> 2) & 1u, (bits >> 3) & 1u);
    }
}

// CSR offsets [n_docs + 1]: five consecutive offsets per group, read as 16 + 16 + 8 bytes.  The offsets array holds
// n_docs + 1 entries, so a group that crosses n_docs clamps each index to n_docs (its counts become 0).
__global__ __launch_bounds__(kThreads) void value_counts_csr_kernel(const uint64_t* __restrict__ off, uint32_t n_docs, uint32_t groups,
                                                                    uint16_t* __restrict__ out, unsigned int* __restrict__ vmax) {
    unsigned int seen = 0;
    for (uint32_t g0 = blockIdx.x * kThreads; g0 < groups; g0 += gridDim.x * kThreads) {
        const uint32_t g = g0 + threadIdx.x, gl = min(g, groups - 1), d0 = gl << 2;
        uint64_t o[5];
        if (d0 + 4 <= n_docs) {  // (wave-uniform except in the wave that holds the column's end)
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(off + d0);
            const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(off + d0 + 2);
            o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
            o[4] = off[d0 + 4];
        } else {
#pragma unroll
            for (int k = 0; k < 5; ++k) o[k] = off[min(d0 + (uint32_t)k, n_docs)];
        }
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t n = o[k + 1] - o[k];
            c[k] = (uint32_t)min(n, (uint64_t)0xFFFFFFFFull);
            if (g < groups) seen = max(seen, c[k]);
        }
        // (a count above 65,535 is truncated here: the request is refused and the product dropped)
        if (g < groups) *reinterpret_cast<uint2*>(out + d0) = pack4(c[0] & 0xFFFFu, c[1] & 0xFFFFu, c[2] & 0xFFFFu, c[3] & 0xFFFFu);
    }
    for (int s = 32; s > 0; s >>= 1) seen = max(seen, (unsigned int)__shfl_xor((int)seen, s));
    if ((threadIdx.x & 63u) == 0 && seen > *vmax) atomicMax(vmax, seen);
}

__global__ __launch_bounds__(kThreads) void value_counts_ones_kernel(uint32_t n_docs, uint32_t groups, uint16_t* __restrict__ out) {
    for (uint32_t g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const uint32_t d0 = g << 2, in = inside4(d0, n_docs);
        *reinterpret_cast<uint2*>(out + d0) = pack4(in & 1u, (in >> 1) & 1u, (in >> 2) & 1u, (in >> 3) & 1u);
    }
}

// a cell grid's u64 doc counts as doubles (a lone value_count whose earlier segments were dense: their value counts
// are the doc counts collected so far)
__global__ __launch_bounds__(kThreads) void counts_to_f64_kernel(const unsigned long long* __restrict__ cnt, size_t n,
                                                                 double* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) out[i] = (double)cnt[i];
}

uint32_t grid_for(uint32_t groups) { return std::min<uint32_t>(8192, (groups + kThreads - 1) / kThreads); }

}  // namespace

void launch_value_counts_ord(const void* ord, int width, uint32_t n_docs, uint32_t n_pad, uint16_t* out, hipStream_t st) {
    const uint32_t groups = n_pad >> 2;
    if (!groups) return;
    if (width == 2)
        hipLaunchKernelGGL(value_counts_ord_kernel<uint16_t>, dim3(grid_for(groups)), dim3(kThreads), 0, st, (const uint16_t*)ord,
                           n_docs, groups, out);
    else
        hipLaunchKernelGGL(value_counts_ord_kernel<uint32_t>, dim3(grid_for(groups)), dim3(kThreads), 0, st, (const uint32_t*)ord,
                           n_docs, groups, out);
}
void launch_value_counts_present(const uint64_t* present, uint32_t n_docs, uint32_t n_pad, uint16_t* out, hipStream_t st) {
    const uint32_t groups = n_pad >> 2;
    if (groups) hipLaunchKernelGGL(value_counts_present_kernel, dim3(grid_for(groups)), dim3(kThreads), 0, st, present, n_docs, groups, out);
}
void launch_value_counts_csr(const uint64_t* offsets, uint32_t n_docs, uint32_t n_pad, uint16_t* out, unsigned int* vmax, hipStream_t st) {
    const uint32_t groups = n_pad >> 2;
    if (groups) hipLaunchKernelGGL(value_counts_csr_kernel, dim3(grid_for(groups)), dim3(kThreads), 0, st, offsets, n_docs, groups, out, vmax);
}
void launch_value_counts_ones(uint32_t n_docs, uint32_t n_pad, uint16_t* out, hipStream_t st) {
    const uint32_t groups = n_pad >> 2;
    if (groups) hipLaunchKernelGGL(value_counts_ones_kernel, dim3(grid_for(groups)), dim3(kThreads), 0, st, n_docs, groups, out);
}
void launch_counts_to_f64(const unsigned long long* cnt, size_t n, double* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(counts_to_f64_kernel, dim3((uint32_t)std::min<size_t>(4096, (n + kThreads - 1) / kThreads)), dim3(kThreads),
                              0, st, cnt, n, out);
}

}  // namespace esgpu
