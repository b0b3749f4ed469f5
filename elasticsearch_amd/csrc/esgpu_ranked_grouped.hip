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
// The unit of work is a (block, pass) pair: a pass is 512 threads x 8 positions, so a block with n <= 4096 -- nearly
// every block of a request for a few ranks -- is one unit, a block with more two.  Four units are in flight per
// workgroup, in a ring of four slots (rg_slot): the thread's group of 8 of the unit, and the block's offsets off[1..K],
// one per lane.  A slot is refilled for the unit four ahead right after its unit is processed.  Every lane issues every
// load of every unit, in one order (rk_pin keeps it): a lane with nothing to read loads a clamped address
// (g12_load_group; off[K] for the offsets; the range's last block past its end) and ignores what it got, so the waits
// are counted -- a unit is entered with the three younger slots' loads outstanding.  The offsets are uniform over the
// wave and never searched in memory: two ballots over them give a wave the rank of its first position and the number
// of offsets below its last, and a thread counts the ranks of its positions (g12_ranks8) over the offsets between the
// two, read from their lanes.  The blocks' scalars -- n = off[K] and the block's one key -- are held one block per lane
// for up to 64 blocks (a chunk of the range) from two vector loads in front of the chunk, so the sequence of units,
// which depends on the n alone, is known where a slot is refilled, and the loop has no scalar load to wait for.
// ESGPU_OPT_RANKED_TERMS = 5 takes this kernel up to 16 ranks: with many offsets inside a wave's positions the rank
// count and the walk of the runs cost more than the per-doc body they replace.
#include "es_group12.hpp"
#include "esgpu_ranked_cells.hpp"

namespace esgpu {

#ifndef ESGPU_RG_WAVES  // waves per SIMD the register budget must allow (6: three 512-thread workgroups per CU, as the
#define ESGPU_RG_WAVES 6  // ranked kernel; at 8 the stats instantiation spills 12 bytes per lane)
#endif
constexpr uint32_t kRgPass = kRkWG * kP12Group;  // positions a workgroup covers per pass: 4,096
static_assert(kG12Block == kBlockDocs && kBlockDocs == 2 * kRgPass, "a g12 block is a zone block: two passes of a workgroup");
static_assert(kG12Groups == 2 * 64, "a block's offsets off[1..K] are two registers of a wave");

constexpr uint32_t kRgOther = 0xFFFFFFFFu;  // (no key: the grid has fewer than 2^32 - 1)
constexpr uint32_t kRgChunk = 64;           // blocks whose scalars a wave holds, one per lane

// one slot of the ring: a unit, its scalars, the thread's group of 8 positions of the unit's pass, and the wave's copy
// of the block's offsets -- lane l loaded off[1 + l] into o0 and off[65 + l] into o1 (a lane past K: off[K], which the
// uses replace by 0xFFFF -- never a copy made where it is loaded)
struct rg_slot {
    uint32_t u;   // 2 * block + pass; a block at or past the range's end: nothing to process
    uint32_t n;   // the block's off[K]
    uint32_t key; // the block's one key inside the grid, or kRgOther: several keys, or one outside the grid
    u32x3_t v;
    uint32_t o0, o1;
};

__device__ __forceinline__ u32x3_t rg_load(const uint8_t* g12, uint32_t blk, uint32_t p0, uint32_t n) {  // p0: a multiple of 8
    return __builtin_nontemporal_load(
        reinterpret_cast<const u32x3_a4_t*>(g12 + (size_t)blk * g12_block_bytes() + g12_load_group(p0, n) * (kP12Words * 4)));
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
    const uint8_t* const g12 = (const uint8_t*)P.g12;
    const uint32_t lane = threadIdx.x & 63u, tid8 = threadIdx.x * kP12Group;
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(tid8 & ~(64u * kP12Group - 1u));  // the wave's first position of a pass
    // A range is walked in chunks of up to 64 blocks.  The scalars of a chunk's blocks -- n = off[K], and the block's one
    // key or kRgOther -- are held one block per lane (nv, kv: lane l holds block c0 + l, past the chunk's end its last
    // block again) from two vector loads in front of the chunk, and read from their lane where a slot is filled: the
    // loop has no scalar load, whose wait -- scalar loads return out of order, so it is a wait for all of them and
    // stands in front of every LDS read -- would expose a block's miss in every unit.
    uint32_t c0 = b_begin, last = b_begin, cu = 0, nv = 0, kv = 0;
    // fill: every lane loads the unit's group (its own or group 0) and two offsets (its own or off[K]), then the unit
    // behind it becomes the next; past the chunk's end the last block's again, with n = 0: one unit, nothing to read
    auto fill = [&](rg_slot& S) {
        const uint32_t blk = min(cu >> 1, last), q = cu & 1u;
        const uint32_t n = (cu >> 1) > last ? 0u : (uint32_t)__builtin_amdgcn_readlane((int)nv, (int)(blk - c0));
        S.u = cu;
        S.n = n;
        S.key = (uint32_t)__builtin_amdgcn_readlane((int)kv, (int)(blk - c0));
        S.v = rg_load(g12, blk, q * kRgPass + tid8, n);
        const uint16_t* const o = P.g12_off + (size_t)blk * kG12OffStride + 1;
        S.o0 = o[min(lane, K - 1u)];
        S.o1 = o[min(lane + 64u, K - 1u)];
        cu = q == 0 && n > kRgPass ? cu + 1u : (cu | 1u) + 1u;
    };
    auto unit = [&](const rg_slot& S) {
        const uint32_t blk = S.u >> 1, q = S.u & 1u, n = S.n, key = S.key;
        if (blk > last) return;  // (a unit past the chunk's end: the ring's last refills)
        const bool fast = key != kRgOther;
        if (q == 0) {  // the block's own business, once
            // one key inside the grid fits any window; any other block's keys are read again here
            int64_t kmn = key, kmx = key;
            if (!fast) {
                const i64x2_t z = zk[__builtin_amdgcn_readfirstlane(blk)];
                kmn = z.x;
                kmx = z.y;
            }
            const bool any = kmn <= kmx && kmx >= 0 && kmn < (int64_t)P.H;  // some doc of the block may lie in the grid
            if (any) {
                const bool fits = kmx - kmn < (int64_t)W;
                if (!win_set || (fits && (kmn < (int64_t)win0 || kmx >= (int64_t)win0 + (int64_t)W)))
                    slide_to((uint32_t)min(max(kmn, (int64_t)0), (int64_t)P.H - 1));
            }
            dirty = dirty || any;
            if (!fast && any) {  // the per-doc body: 16 docs per thread in quads, from the original columns
                const auto& Q = *rk_again();
#pragma unroll 1
                for (uint32_t i = 0; i < kBlockDocs / (4u * kRkWG); ++i) {
                    const uint32_t doc0 = blk * kBlockDocs + (i * kRkWG + threadIdx.x) * 4u;
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
                rk_drain();  // (its own loads have landed: the join below is not a wait for everything in flight)
            }
        }
        if (fast && q * kRgPass < n) {
            const uint32_t rowm = cell0 + 8u * ((key - win0) * K);
            // a lane past K holds no offset: above every position
            const uint32_t o0 = lane < K ? S.o0 : kG12Missing, o1 = lane + 64u < K ? S.o1 : kG12Missing;
            // the wave's span of positions among the offsets: every lane compares its offset, two ballots count them
            const uint32_t w0 = q * kRgPass + wave0;
            uint32_t base = (uint32_t)__popcll(__ballot(o0 <= w0));
            uint32_t upto = (uint32_t)__popcll(__ballot(o0 < w0 + 64u * kP12Group));
            if (K > 64u) {
                base += (uint32_t)__popcll(__ballot(o1 <= w0));
                upto += (uint32_t)__popcll(__ballot(o1 < w0 + 64u * kP12Group));
            }
            // (the offsets read from a lane are off[base + 1 .. upto], upto <= K: lanes that hold one)
            rg_group8<MET>(S.v, q * kRgPass + tid8, n, K, base, upto, S.o0, S.o1, rowm, dpk, onehi);
        }
    };

    for (; c0 < b_end; c0 += kRgChunk) {
        last = min(c0 + kRgChunk, b_end) - 1u;
        {  // (every lane of a wave reads its own block's zone keys; what is read back from a lane is uniform over the workgroup)
            const uint32_t bl = min(c0 + lane, last);
            const i64x2_t z = *reinterpret_cast<const i64x2_t*>(P.zkey + 2u * (size_t)bl);
            kv = z.x == z.y && (uint64_t)z.x < (uint64_t)P.H ? (uint32_t)z.x : kRgOther;
            nv = P.g12_off[(size_t)bl * kG12OffStride + K];
        }
        cu = 2u * c0;
        rg_slot S0, S1, S2, S3;
        fill(S0);
        rk_pin();
        fill(S1);
        rk_pin();
        fill(S2);
        rk_pin();
        fill(S3);
        rk_pin();
        // the loop is unrolled by the ring's depth, so every slot is a register set of its own, and has one exit (an
        // exit in front of each unit is compiled as a path from every refill to the loop's head, and the first slot is
        // then entered through vmcnt(0)): the chunk ends in any slot, and the refills behind it load the last block's
        // group 0 again
        do {
            unit(S0);
            fill(S0);
            rk_pin();
            unit(S1);
            fill(S1);
            rk_pin();
            unit(S2);
            fill(S2);
            rk_pin();
            unit(S3);
            fill(S3);
            rk_pin();
        } while ((S0.u >> 1) <= last);
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
