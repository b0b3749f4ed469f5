// esgpu_ranked_grouped.hip — the ranked-terms collect (path 10) over rank-grouped zone blocks (es_group12.hpp): the
// ranked kernel (esgpu_ranked.hip) with another body for the single-key block.
//
// The docs of a zone block are stored grouped by rank, so the docs a request collects (rank < K) are the block's
// positions [0, n), n = off[K]: the kernel streams that prefix only -- no rank column, and nothing of the docs it does
// not collect -- and a thread's 8 consecutive positions, which almost always hold one rank, are reduced in registers
// (count, sum, min, max) before one update of the LDS cell.  The block loop, the window, its slide and flush, the cells
// and everything downstream are esgpu_ranked.hip's (esgpu_ranked_cells.hpp):
//   - a block whose docs all round to one key inside the grid takes the grouped body, the segment's last partial block
//     included (its pad docs are in the group nothing collects);
//   - any other block (several keys, a key outside the grid) takes the per-doc body over the original, unpermuted
//     columns -- rank16, d16 and the block-delta keys -- loaded there.
// A block's prefix (both passes of 512 threads x 8 positions) is prefetched two blocks ahead into one of two buffers
// (even and odd blocks), with the block's offsets off[1..K], one per lane.  The offsets are uniform over the wave and
// never searched in memory: two ballots over them give a wave the rank of its first position and the number of
// offsets below its last, and a thread counts the ranks of its positions (g12_ranks8) over the offsets between the two,
// read from their lanes.  The zone keys and n = off[K] are scalar loads issued a further two blocks ahead, so that the
// prefetch of a block knows which lanes have something to load.  ESGPU_OPT_RANKED_TERMS = 5 takes this kernel up to 16
// ranks: with many offsets inside a wave's positions the rank count and the walk of the runs cost more than the
// per-doc body they replace.
#include "es_group12.hpp"
#include "esgpu_ranked_cells.hpp"

namespace esgpu {

#ifndef ESGPU_RG_WAVES  // waves per SIMD the register budget must allow (6: three 512-thread workgroups per CU, as the
#define ESGPU_RG_WAVES 6  // ranked kernel; at 8 the stats instantiation spills 12 bytes per lane)
#endif
constexpr uint32_t kRgPass = kRkWG * kP12Group;  // positions a workgroup covers per pass: 4,096
static_assert(kG12Block == kBlockDocs && kBlockDocs == 2 * kRgPass, "a g12 block is a zone block: two passes of a workgroup");
static_assert(kG12Groups == 2 * 64, "a block's offsets off[1..K] are two registers of a wave");

typedef const uint32_t __attribute__((address_space(4))) rg_word_c;

// one block's prefetch: the thread's group of 8 positions of each of the block's two passes, and the wave's copy of the
// offsets -- lane l holds off[1 + l] in o0 and off[65 + l] in o1 (those up to off[K]; 0xFFFF past them)
struct rg_buf {
    u32x3_t v[kBlockDocs / kRgPass];  // the thread's group of each pass
    uint32_t o0, o1;
};

__device__ __forceinline__ u32x3_t rg_load(const uint8_t* g12, uint32_t blk, uint32_t p0) {  // p0: a multiple of 8, < off[K]
    return __builtin_nontemporal_load(
        reinterpret_cast<const u32x3_a4_t*>(g12 + (size_t)blk * g12_block_bytes() + (p0 / kP12Group) * (kP12Words * 4)));
}

// one run of a thread's positions into its cell: the packed add of the run's sum and count, and the bounds -- READ:
// where they move, after a read of the cell's pair (a thread's last run: most lanes of a wave issue it, many to one
// cell); otherwise by the two atomics unasked (a run that ends inside the thread's positions: a lane or two of the wave,
// and no wait for a read between one run and the next)
template <int MET, bool READ = true>
__device__ __forceinline__ void rg_emit(uint32_t r, uint32_t K, uint32_t cnt, uint32_t sum, uint32_t mn, uint32_t mx,
                                        uint32_t rowm, uint32_t dpk, uint32_t onehi) {
    if (r < K) {  // (rank K: positions at or past off[K], not collected)
        const uint32_t ca = rowm + 8u * r;
        atomicAdd(lds_ptr<unsigned long long>(ca + dpk), join64(sum, cnt * onehi));
        if constexpr (MET >= 2) {
            if constexpr (READ) {
                const u32x2_t m = *lds_ptr<u32x2_t>(ca);
                if (mn < m.x) atomicMin(lds_ptr<uint32_t>(ca), mn);
                if (mx > m.y) atomicMax(lds_ptr<uint32_t>(ca + 4u), mx);
            } else {
                atomicMin(lds_ptr<uint32_t>(ca), mn);
                atomicMax(lds_ptr<uint32_t>(ca + 4u), mx);
            }
        }
    }
}

// The 8 positions p0 .. p0 + 7 of a single-key block, for a wave whose 512 positions start at rank `base` and hold the
// offsets off[base + 1 .. upto] (g12_ranks8; both uniform over the wave).  `rowm`, `dpk`: as rk_quad's.
//   upto == base: no offset inside the wave -- all its positions are of rank base: one reduction, one update;
//   otherwise: the lanes below n = off[K] count their positions' ranks over the wave's few offsets and walk the runs of
//   equal rank, each reduced in registers.
template <int MET>
__device__ __forceinline__ void rg_group8(u32x3_t v, uint32_t p0, uint32_t n, uint32_t K, uint32_t base, uint32_t upto,
                                          uint32_t o0, uint32_t o1, uint32_t rowm, uint32_t dpk, uint32_t onehi) {
    if (base >= K) return;  // (the wave starts at or past n)
    const uint32_t w[3] = {v.x, v.y, v.z};
    uint32_t d[8];
    if (upto == base) {
        p12_unpack8(w, d);
        const uint32_t sum = ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
        const uint32_t mn = min(min(min(d[0], d[1]), min(d[2], d[3])), min(min(d[4], d[5]), min(d[6], d[7])));
        const uint32_t mx = max(max(max(d[0], d[1]), max(d[2], d[3])), max(max(d[4], d[5]), max(d[6], d[7])));
        rg_emit<MET>(base, K, 8u, sum, mn, mx, rowm, dpk, onehi);
    } else if (p0 < n) {
        p12_unpack8(w, d);
        uint32_t r[8];
        g12_ranks8(p0, base, upto, [&](uint32_t j) {  // off[j]: uniform over the wave
            return (uint32_t)(j <= 64 ? __builtin_amdgcn_readlane((int)o0, (int)(j - 1)) : __builtin_amdgcn_readlane((int)o1, (int)(j - 65)));
        }, r);
        uint32_t cur = r[0], cnt = 1, sum = d[0], mn = d[0], mx = d[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) {
            if (r[i] != cur) {
                rg_emit<MET, false>(cur, K, cnt, sum, mn, mx, rowm, dpk, onehi);
                cur = r[i];
                cnt = 0; sum = 0; mn = ~0u; mx = 0;
            }
            ++cnt;
            sum += d[i];
            mn = min(mn, d[i]);
            mx = max(mx, d[i]);
        }
        rg_emit<MET>(cur, K, cnt, sum, mn, mx, rowm, dpk, onehi);
    }
}

template <int MET>
__global__ __launch_bounds__(kRkWG, ESGPU_RG_WAVES) void ranked_grouped_kernel(RankedParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t K = P.K, W = P.W, C = K * W;
    const uint32_t ncp = max(P.ncopies, 1u);
    const uint32_t CS = P.cstride;
    const rk_cells cells = rk_carve<MET>(smem, C, CS, ncp);
    unsigned long long* const pk = cells.pk;
    uint32_t* const mm = cells.mm;
    const uint32_t coff = cells.coff;

    const uint32_t b_begin = blockIdx.x * P.blocks_per_wg;
    const uint32_t b_end = min(b_begin + P.blocks_per_wg, P.n_blocks);
    if (b_begin >= b_end) return;

    const uint32_t sh = P.pk_shift;
    const uint32_t onehi = 1u << (sh - 32);
    const uint32_t cell0 = MET >= 2 ? lds_addr(mm) : lds_addr(pk + coff);
    const uint32_t dpk = MET >= 2 ? lds_addr(pk + coff) - lds_addr(mm) : 0u;

    uint32_t win0 = 0;
    bool win_set = false, dirty = false;
    auto flush = [&]() { rk_flush<MET>(pk, mm, C, K, CS, ncp, sh, win0); };
    auto slide_to = [&](uint32_t k0) {
        if (dirty) flush();
        dirty = false;
        win0 = k0;
        win_set = true;
    };

    const zkey_pair_c* const zk = zkey_view(P.zkey);
    rg_word_c* const offw = (rg_word_c*)P.g12_off;
    const uint8_t* const g12 = (const uint8_t*)P.g12;
    const uint32_t lane = threadIdx.x & 63u, tid8 = threadIdx.x * kP12Group;
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(tid8 & ~(64u * kP12Group - 1u));  // the wave's first position of a pass
    const uint32_t last = b_end - 1;
    // (past the range's end the scalar loads read the last block's again: the values are not used)
    auto zload = [&](uint32_t b) -> i64x2_t { return zk[__builtin_amdgcn_readfirstlane(min(b, last))]; };
    auto nload = [&](uint32_t b) -> uint32_t {  // off[K] of block b: one half of a word
        const uint32_t i = __builtin_amdgcn_readfirstlane(min(b, last)) * kG12OffStride + K;
        const uint32_t w = offw[i >> 1];
        return (i & 1u) ? w >> 16 : w & 0xFFFFu;
    };
    // block blk's prefix (n = its off[K]) and its offsets: only the lanes that have something to load
    auto prefetch = [&](rg_buf& B, uint32_t blk, uint32_t n) {
        if (n > 0) {
#pragma unroll
            for (uint32_t q = 0; q < kBlockDocs / kRgPass; ++q)
                if (q * kRgPass + tid8 < n) B.v[q] = rg_load(g12, blk, q * kRgPass + tid8);
            const uint16_t* const o = P.g12_off + (size_t)blk * kG12OffStride + 1;
            if (lane < K) B.o0 = o[lane];
            if (lane + 64u < K) B.o1 = o[lane + 64u];
        }
    };
    auto block = [&](const rg_buf& B, uint32_t blk, i64x2_t z, uint32_t n) {
        const int64_t kmn = z.x, kmx = z.y;
        // (every lane reads the same zone keys: the decisions are uniform over the workgroup)
        const bool any = kmn <= kmx && kmx >= 0 && kmn < (int64_t)P.H;  // some doc of the block may lie in the grid
        if (any) {
            const bool fits = kmx - kmn < (int64_t)W;
            if (!win_set || (fits && (kmn < (int64_t)win0 || kmx >= (int64_t)win0 + (int64_t)W)))
                slide_to((uint32_t)min(max(kmn, (int64_t)0), (int64_t)P.H - 1));
        }
        const bool fast = kmn == kmx && (uint64_t)kmn < (uint64_t)P.H;
        if (!fast && any) {  // the per-doc body: 16 docs per thread in quads, from the original columns
            const auto& Q = *rk_again();
#pragma unroll 1
            for (uint32_t q = 0; q < kBlockDocs / (4u * kRkWG); ++q) {
                const uint32_t doc0 = blk * kBlockDocs + (q * kRkWG + threadIdx.x) * 4u;
                rk_r4<2> r = {0xFFFFFFFFu, 0xFFFFFFFFu};
                uint32_t m0 = 0, m1 = 0;
                if (doc0 < Q.n_docs) {  // (the columns are padded to whole blocks: the quad lies inside them)
                    const u32x2_t rr = load8((const uint16_t*)Q.rank + doc0), mv = load8((const uint16_t*)Q.mv + doc0);
                    r = {rr.x, rr.y};
                    m0 = mv.x;
                    m1 = mv.y;
                }
                rk_slow_quad<MET, 2, 16>(doc0, r, m0, m1, kmn, kmx, K, win0, win_set ? W : 0u, pk, mm, coff, sh);
            }
        }
        dirty = dirty || any;
        if (fast && n > 0) {
            const uint32_t rowm = cell0 + 8u * (((uint32_t)kmn - win0) * K);
            // the wave's span of positions among the offsets: every lane compares its offset, two ballots count them
            auto span = [&](uint32_t w0, uint32_t& base, uint32_t& upto) {
                base = (uint32_t)__popcll(__ballot(B.o0 <= w0));
                upto = (uint32_t)__popcll(__ballot(B.o0 < w0 + 64u * kP12Group));
                if (K > 64u) {
                    base += (uint32_t)__popcll(__ballot(B.o1 <= w0));
                    upto += (uint32_t)__popcll(__ballot(B.o1 < w0 + 64u * kP12Group));
                }
            };
            // (the second pass: more than half of the block's docs collected)
#pragma unroll
            for (uint32_t q = 0; q < kBlockDocs / kRgPass; ++q) {
                if (q * kRgPass < n) {
                    uint32_t base, upto;
                    span(q * kRgPass + wave0, base, upto);
                    rg_group8<MET>(B.v[q], q * kRgPass + tid8, n, K, base, upto, B.o0, B.o1, rowm, dpk, onehi);
                }
            }
        }
    };

    i64x2_t za = zload(b_begin), zb = zload(b_begin + 1);
    uint32_t na = nload(b_begin), nb = nload(b_begin + 1);
    rg_buf A = {{{0, 0, 0}, {0, 0, 0}}, kG12Missing, kG12Missing}, B = A;  // (a lane past K holds no offset: above every position)
    prefetch(A, b_begin, na);
    rk_pin();
    if (b_begin + 1 < b_end) prefetch(B, b_begin + 1, nb);
    rk_pin();
#pragma unroll 1
    for (uint32_t cb = b_begin; cb < b_end; cb += 2) {
        const i64x2_t za2 = zload(cb + 2), zb2 = zload(cb + 3);
        const uint32_t na2 = nload(cb + 2), nb2 = nload(cb + 3);
        block(A, cb, za, na);
        if (cb + 2 < b_end) prefetch(A, cb + 2, na2);
        rk_pin();
        if (cb + 1 < b_end) block(B, cb + 1, zb, nb);
        if (cb + 3 < b_end) prefetch(B, cb + 3, nb2);
        rk_pin();
        za = za2; zb = zb2;
        na = na2; nb = nb2;
    }
    if (dirty) flush();
}

template <typename F>
static auto with_rg(int met, F&& f) {
    return met >= 2 ? f(ranked_grouped_kernel<2>) : f(ranked_grouped_kernel<1>);
}
void launch_ranked_grouped(const RankedParams& p, int met, uint32_t grid, size_t lds, hipStream_t st) {
    with_rg(met, [&](auto* k) { hipLaunchKernelGGL(k, dim3(grid), dim3(kRkWG), lds, st, p); return 0; });
}
int ranked_grouped_occupancy(int met, size_t lds) {
    int n = 0;
    const hipError_t e = with_rg(met, [&](auto* k) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, kRkWG, lds); });
    return e == hipSuccess ? n : 1;
}

}  // namespace esgpu
