// esgpu_numord.hip — numeric ordinals: a single-valued long column turned into the segment's sorted dictionary of
// distinct values and a u32 rank per doc (terms over long / date fields, LongTermsAggregator's per-doc LongHash done
// once per segment).  Two builds, chosen from the column's value range:
//   dense span (vmax - vmin < 2^26): a presence bitmap over value - vmin (mark), an exclusive prefix sum of its words'
//     popcounts that also scatters the dictionary (rank), and ord = base[word] + popcount(bits below) (encode);
//   wide span: an open-addressing set of the values (64-bit compare-and-swap, bounded probing), compacted; the host
//     sorts the distinct values; each slot's rank by binary search, then each doc's slot looked up again (encode).
// No kernel divides 64-bit values, no loop is unbounded, and the dense path issues a global atomic only for a bit that
// is still clear.
#include <algorithm>

#include "esgpu_kernels.hpp"

namespace esgpu {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMissing = 0xFFFFFFFFu;

// the delta (value - vmin) of 4 consecutive docs, from the upload-width column or one of its compact copies
template <class T>
__device__ inline void load_deltas4(const T* v, uint32_t d0, int64_t vmin, uint64_t (&dl)[4]);
template <>
__device__ inline void load_deltas4<int64_t>(const int64_t* v, uint32_t d0, int64_t vmin, uint64_t (&dl)[4]) {
    const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(v + d0);
    const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(v + d0 + 2);
    dl[0] = a.x - (uint64_t)vmin; dl[1] = a.y - (uint64_t)vmin; dl[2] = b.x - (uint64_t)vmin; dl[3] = b.y - (uint64_t)vmin;
}
template <>
__device__ inline void load_deltas4<uint32_t>(const uint32_t* v, uint32_t d0, int64_t, uint64_t (&dl)[4]) {
    const uint4 a = *reinterpret_cast<const uint4*>(v + d0);
    dl[0] = a.x; dl[1] = a.y; dl[2] = a.z; dl[3] = a.w;
}
template <>
__device__ inline void load_deltas4<uint16_t>(const uint16_t* v, uint32_t d0, int64_t, uint64_t (&dl)[4]) {
    const uint2 a = *reinterpret_cast<const uint2*>(v + d0);
    dl[0] = a.x & 0xFFFFu; dl[1] = a.x >> 16; dl[2] = a.y & 0xFFFFu; dl[3] = a.y >> 16;
}

// bits [d0, d0 + 4) of the live docs: inside [0, n_docs) and present (d0 is a multiple of 4: one present word)
__device__ inline uint32_t live4(const uint64_t* present, uint32_t d0, uint32_t n_docs) {
    uint32_t m = d0 + 4 <= n_docs ? 0xFu : d0 >= n_docs ? 0u : (1u << (n_docs - d0)) - 1u;
    if (present && m) m &= (uint32_t)(present[d0 >> 6] >> (d0 & 63));
    return m;
}

// ---- dense span: mark ----------------------------------------------------------------------------------------
// LDS form: the whole bitmap private to the workgroup (ds_or), then one global atomicOr per non-zero word
template <class T>
__global__ __launch_bounds__(kThreads) void numord_mark_lds_kernel(const T* v, const uint64_t* present, uint32_t n_docs,
                                                                   uint32_t n_pad, int64_t vmin, uint64_t span,
                                                                   uint32_t words32, uint32_t* bits) {
    extern __shared__ uint32_t lbits[];
    for (uint32_t w = threadIdx.x; w < words32; w += kThreads) lbits[w] = 0;
    __syncthreads();
    const uint32_t groups = n_pad >> 2;
    for (uint32_t g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const uint32_t d0 = g << 2;
        const uint32_t live = live4(present, d0, n_docs);
        if (!live) continue;
        uint64_t dl[4];
        load_deltas4<T>(v, d0, vmin, dl);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (((live >> k) & 1u) && dl[k] <= span) atomicOr(&lbits[(uint32_t)dl[k] >> 5], 1u << ((uint32_t)dl[k] & 31u));
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < words32; w += kThreads) {
        const uint32_t b = lbits[w];
        if (b) atomicOr(&bits[w], b);
    }
}

// global form: a plain load of the word first, the atomicOr only while the bit is still clear
template <class T>
__global__ __launch_bounds__(kThreads) void numord_mark_global_kernel(const T* v, const uint64_t* present, uint32_t n_docs,
                                                                      uint32_t n_pad, int64_t vmin, uint64_t span,
                                                                      uint32_t* bits) {
    const uint32_t groups = n_pad >> 2;
    for (uint32_t g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const uint32_t d0 = g << 2;
        const uint32_t live = live4(present, d0, n_docs);
        if (!live) continue;
        uint64_t dl[4];
        load_deltas4<T>(v, d0, vmin, dl);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!((live >> k) & 1u) || dl[k] > span) continue;
            const uint32_t w = (uint32_t)dl[k] >> 5, b = 1u << ((uint32_t)dl[k] & 31u);
            if (!(bits[w] & b)) atomicOr(&bits[w], b);
        }
    }
}

// ---- dense span: rank -----------------------------------------------------------------------------------------
// chunks of kRankChunk 64-bit words, one workgroup each: the chunk's popcount; one workgroup scans the chunk sums; then
// each chunk writes its words' rank bases and scatters the dictionary
constexpr uint32_t kRankPer = 4, kRankChunk = kThreads * kRankPer;

__device__ inline uint32_t block_exclusive_scan(uint32_t x, uint32_t* lds, uint32_t* total) {
    lds[threadIdx.x] = x;
    __syncthreads();
    for (uint32_t off = 1; off < kThreads; off <<= 1) {
        const uint32_t t = threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
        __syncthreads();
        lds[threadIdx.x] += t;
        __syncthreads();
    }
    const uint32_t incl = lds[threadIdx.x];
    if (total) *total = lds[kThreads - 1];
    __syncthreads();
    return incl - x;
}

__global__ __launch_bounds__(kThreads) void numord_rank_sum_kernel(const uint64_t* bits, uint32_t words, uint32_t* chunk_sum) {
    __shared__ uint32_t lds[kThreads];
    const uint32_t w0 = blockIdx.x * kRankChunk + threadIdx.x * kRankPer;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRankPer; ++k)
        if (w0 + k < words) c += (uint32_t)__popcll(bits[w0 + k]);
    uint32_t total;
    block_exclusive_scan(c, lds, &total);
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

// exclusive scan of up to kRankChunk chunk sums in place; chunk_sum[chunks] = the number of distinct values
__global__ __launch_bounds__(kThreads) void numord_rank_scan_kernel(uint32_t* chunk_sum, uint32_t chunks) {
    __shared__ uint32_t lds[kThreads];
    const uint32_t i0 = threadIdx.x * kRankPer;
    uint32_t x[kRankPer], c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRankPer; ++k) {
        x[k] = i0 + k < chunks ? chunk_sum[i0 + k] : 0;
        c += x[k];
    }
    uint32_t total;
    uint32_t run = block_exclusive_scan(c, lds, &total);
#pragma unroll
    for (uint32_t k = 0; k < kRankPer; ++k) {
        if (i0 + k < chunks) chunk_sum[i0 + k] = run;
        run += x[k];
    }
    if (threadIdx.x == 0) chunk_sum[chunks] = total;
}

__global__ __launch_bounds__(kThreads) void numord_rank_write_kernel(const uint64_t* bits, uint32_t words, const uint32_t* chunk_base,
                                                                     int64_t vmin, uint32_t n_dict, uint32_t* base, int64_t* dict) {
    __shared__ uint32_t lds[kThreads];
    const uint32_t w0 = blockIdx.x * kRankChunk + threadIdx.x * kRankPer;
    uint64_t b[kRankPer];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRankPer; ++k) {
        b[k] = w0 + k < words ? bits[w0 + k] : 0;
        c += (uint32_t)__popcll(b[k]);
    }
    uint32_t run = chunk_base[blockIdx.x] + block_exclusive_scan(c, lds, nullptr);
#pragma unroll
    for (uint32_t k = 0; k < kRankPer; ++k) {
        if (w0 + k >= words) break;
        base[w0 + k] = run;
        uint64_t m = b[k];
        while (m) {  // at most 64 rounds: one per set bit
            const uint32_t bit = (uint32_t)__ffsll((long long)m) - 1u;
            m &= m - 1;
            if (run < n_dict) dict[run] = (int64_t)((uint64_t)vmin + (((uint64_t)(w0 + k)) << 6) + bit);
            ++run;
        }
    }
}

// ---- dense span: encode -----------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kThreads) void numord_encode_dense_kernel(const T* v, const uint64_t* present, uint32_t n_docs,
                                                                       uint32_t n_pad, int64_t vmin, uint64_t span,
                                                                       const uint64_t* bits, const uint32_t* base, uint32_t* ord) {
    const uint32_t groups = n_pad >> 2;
    for (uint32_t g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const uint32_t d0 = g << 2;
        const uint32_t live = live4(present, d0, n_docs);
        uint32_t o[4] = {kMissing, kMissing, kMissing, kMissing};
        if (live) {
            uint64_t dl[4];
            load_deltas4<T>(v, d0, vmin, dl);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!((live >> k) & 1u) || dl[k] > span) continue;
                const uint32_t w = (uint32_t)(dl[k] >> 6), bit = (uint32_t)dl[k] & 63u;
                o[k] = base[w] + (uint32_t)__popcll(bits[w] & ((1ull << bit) - 1ull));
            }
        }
        *reinterpret_cast<uint4*>(ord + d0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// ---- wide span ---------------------------------------------------------------------------------------------------
constexpr unsigned long long kEmptySlot = 0xFFFFFFFFFFFFFFFFull;  // the long -1: kept in flags[kNumOrdFlagSentinel] instead

__device__ inline uint32_t slot_hash(uint64_t v, uint32_t mask) {  // murmur3's 64-bit finalizer
    v ^= v >> 33; v *= 0xff51afd7ed558ccdULL; v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ULL; v ^= v >> 33;
    return (uint32_t)v & mask;
}

__global__ __launch_bounds__(kThreads) void numord_hash_insert_kernel(const int64_t* v, const uint64_t* present, uint32_t n_docs,
                                                                      unsigned long long* table, uint32_t mask, uint32_t probe_limit,
                                                                      uint32_t* flags) {
    for (uint32_t d = blockIdx.x * kThreads + threadIdx.x; d < n_docs; d += gridDim.x * kThreads) {
        if (present && !((present[d >> 6] >> (d & 63)) & 1ull)) continue;
        const unsigned long long x = (unsigned long long)v[d];
        if (x == kEmptySlot) { flags[kNumOrdFlagSentinel] = 1; continue; }
        uint32_t h = slot_hash(x, mask);
        bool placed = false;
        for (uint32_t probe = 0; probe < probe_limit; ++probe) {
            unsigned long long cur = table[h];
            if (cur == kEmptySlot) cur = atomicCAS(&table[h], kEmptySlot, x);
            if (cur == kEmptySlot || cur == x) { placed = true; break; }
            h = (h + 1) & mask;
        }
        if (!placed) {  // the table is full, or the probe limit is reached: the host refuses the column
            flags[kNumOrdFlagOverflow] = 1;
            return;
        }
    }
}

// the occupied slots' values, in any order; *count ends at their number (values past `cap` are counted, not stored)
__global__ __launch_bounds__(kThreads) void numord_hash_compact_kernel(const unsigned long long* table, uint32_t slots, uint32_t cap,
                                                                       int64_t* out, uint32_t* count) {
    for (uint32_t s0 = blockIdx.x * kThreads; s0 < slots; s0 += gridDim.x * kThreads) {
        const uint32_t s = s0 + threadIdx.x;
        const unsigned long long x = s < slots ? table[s] : kEmptySlot;
        const bool full = x != kEmptySlot;
        const unsigned long long ballot = __ballot(full);
        if (!ballot) continue;
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t wave_base = 0;
        if (lane == (uint32_t)__ffsll((long long)ballot) - 1u) wave_base = atomicAdd(count, (uint32_t)__popcll(ballot));
        wave_base = __shfl(wave_base, (int)(__ffsll((long long)ballot) - 1));
        if (full) {
            const uint32_t at = wave_base + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
            if (at < cap) out[at] = (int64_t)x;
        }
    }
}

__device__ inline uint32_t dict_rank(const int64_t* dict, uint32_t n, int64_t x) {  // lower bound; at most 32 rounds
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (dict[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void numord_hash_rank_kernel(const unsigned long long* table, uint32_t slots, const int64_t* dict,
                                                                    uint32_t n_dict, uint32_t* slot_rank) {
    for (uint32_t s = blockIdx.x * kThreads + threadIdx.x; s < slots; s += gridDim.x * kThreads) {
        const unsigned long long x = table[s];
        uint32_t r = kMissing;
        if (x != kEmptySlot) {
            r = dict_rank(dict, n_dict, (int64_t)x);
            if (r >= n_dict) r = kMissing;
        }
        slot_rank[s] = r;
    }
}

__global__ __launch_bounds__(kThreads) void numord_encode_hash_kernel(const int64_t* v, const uint64_t* present, uint32_t n_docs,
                                                                      uint32_t n_pad, const unsigned long long* table, uint32_t mask,
                                                                      uint32_t probe_limit, const uint32_t* slot_rank,
                                                                      uint32_t sentinel_rank, uint32_t* ord) {
    const uint32_t groups = n_pad >> 2;
    for (uint32_t g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const uint32_t d0 = g << 2;
        const uint32_t live = live4(present, d0, n_docs);
        uint32_t o[4] = {kMissing, kMissing, kMissing, kMissing};
        if (live) {
            uint64_t x[4];
            load_deltas4<int64_t>(v, d0, 0, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!((live >> k) & 1u)) continue;
                if (x[k] == kEmptySlot) { o[k] = sentinel_rank; continue; }
                uint32_t h = slot_hash(x[k], mask);
                for (uint32_t probe = 0; probe < probe_limit; ++probe) {
                    const unsigned long long cur = table[h];
                    if (cur == x[k]) { o[k] = slot_rank[h]; break; }
                    if (cur == kEmptySlot) break;  // (every live value was inserted: not reached)
                    h = (h + 1) & mask;
                }
            }
        }
        *reinterpret_cast<uint4*>(ord + d0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

inline uint32_t doc_grid(uint32_t n_pad) { return std::max(1u, std::min<uint32_t>(2048, ((n_pad >> 2) + kThreads - 1) / kThreads)); }

}  // namespace

void launch_numord_mark(const void* v, int width, const uint64_t* present, uint32_t n_docs, uint32_t n_pad, int64_t vmin,
                        uint64_t span, uint32_t* bits, hipStream_t st) {
    if (!n_docs) return;
    const uint32_t words32 = (uint32_t)((span >> 5) + 1);
    const bool lds = span < kNumOrdLdsBits;
    // the LDS form flushes one bitmap per workgroup: a few workgroups per CU's worth, no more than the docs fill
    const uint32_t grid = lds ? std::max(1u, std::min<uint32_t>(1024, ((n_pad >> 2) + 16 * kThreads - 1) / (16 * kThreads))) : doc_grid(n_pad);
#define ESGPU_MARK(T)                                                                                                        \
    do {                                                                                                                     \
        if (lds) hipLaunchKernelGGL(numord_mark_lds_kernel<T>, dim3(grid), dim3(kThreads), words32 * 4, st, (const T*)v, present, \
                                    n_docs, n_pad, vmin, span, words32, bits);                                               \
        else hipLaunchKernelGGL(numord_mark_global_kernel<T>, dim3(grid), dim3(kThreads), 0, st, (const T*)v, present, n_docs,  \
                                n_pad, vmin, span, bits);                                                                    \
    } while (0)
    if (width == 2) ESGPU_MARK(uint16_t);
    else if (width == 4) ESGPU_MARK(uint32_t);
    else ESGPU_MARK(int64_t);
#undef ESGPU_MARK
}

void launch_numord_rank_sums(const uint64_t* bits, uint32_t words, uint32_t* chunk_sum, hipStream_t st) {
    const uint32_t chunks = (words + kRankChunk - 1) / kRankChunk;
    hipLaunchKernelGGL(numord_rank_sum_kernel, dim3(chunks), dim3(kThreads), 0, st, bits, words, chunk_sum);
    hipLaunchKernelGGL(numord_rank_scan_kernel, dim3(1), dim3(kThreads), 0, st, chunk_sum, chunks);
}

void launch_numord_rank_write(const uint64_t* bits, uint32_t words, const uint32_t* chunk_base, int64_t vmin, uint32_t n_dict,
                              uint32_t* base, int64_t* dict, hipStream_t st) {
    const uint32_t chunks = (words + kRankChunk - 1) / kRankChunk;
    hipLaunchKernelGGL(numord_rank_write_kernel, dim3(chunks), dim3(kThreads), 0, st, bits, words, chunk_base, vmin, n_dict, base, dict);
}

void launch_numord_encode_dense(const void* v, int width, const uint64_t* present, uint32_t n_docs, uint32_t n_pad, int64_t vmin,
                                uint64_t span, const uint64_t* bits, const uint32_t* base, uint32_t* ord, hipStream_t st) {
    if (!n_pad) return;
    const uint32_t grid = doc_grid(n_pad);
    if (width == 2)
        hipLaunchKernelGGL(numord_encode_dense_kernel<uint16_t>, dim3(grid), dim3(kThreads), 0, st, (const uint16_t*)v, present, n_docs,
                           n_pad, vmin, span, bits, base, ord);
    else if (width == 4)
        hipLaunchKernelGGL(numord_encode_dense_kernel<uint32_t>, dim3(grid), dim3(kThreads), 0, st, (const uint32_t*)v, present, n_docs,
                           n_pad, vmin, span, bits, base, ord);
    else
        hipLaunchKernelGGL(numord_encode_dense_kernel<int64_t>, dim3(grid), dim3(kThreads), 0, st, (const int64_t*)v, present, n_docs,
                           n_pad, vmin, span, bits, base, ord);
}

void launch_numord_hash_insert(const int64_t* v, const uint64_t* present, uint32_t n_docs, unsigned long long* table, uint32_t slots,
                               uint32_t probe_limit, uint32_t* flags, hipStream_t st) {
    if (!n_docs) return;
    const uint32_t grid = std::max(1u, std::min<uint32_t>(2048, (n_docs + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(numord_hash_insert_kernel, dim3(grid), dim3(kThreads), 0, st, v, present, n_docs, table, slots - 1, probe_limit,
                       flags);
}

void launch_numord_hash_compact(const unsigned long long* table, uint32_t slots, uint32_t cap, int64_t* out, uint32_t* count,
                                hipStream_t st) {
    const uint32_t grid = std::max(1u, std::min<uint32_t>(2048, (slots + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(numord_hash_compact_kernel, dim3(grid), dim3(kThreads), 0, st, table, slots, cap, out, count);
}

void launch_numord_hash_rank(const unsigned long long* table, uint32_t slots, const int64_t* dict, uint32_t n_dict, uint32_t* slot_rank,
                             hipStream_t st) {
    const uint32_t grid = std::max(1u, std::min<uint32_t>(2048, (slots + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(numord_hash_rank_kernel, dim3(grid), dim3(kThreads), 0, st, table, slots, dict, n_dict, slot_rank);
}

void launch_numord_encode_hash(const int64_t* v, const uint64_t* present, uint32_t n_docs, uint32_t n_pad,
                               const unsigned long long* table, uint32_t slots, uint32_t probe_limit, const uint32_t* slot_rank,
                               uint32_t sentinel_rank, uint32_t* ord, hipStream_t st) {
    if (!n_pad) return;
    hipLaunchKernelGGL(numord_encode_hash_kernel, dim3(doc_grid(n_pad)), dim3(kThreads), 0, st, v, present, n_docs, n_pad, table,
                       slots - 1, probe_limit, slot_rank, sentinel_rank, ord);
}

}  // namespace esgpu
