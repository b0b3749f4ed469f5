// esgpu_ranked.hip — the ranked-terms collect (path 10) over the rank column (8-bit rank8, or the 16-bit rank16 it is
// recoded from), the metric deltas (16-bit d16, or the packed 12-bit d12 recoded from it when the values span < 4096)
// and block-delta keys of time-sorted data: a kernel of its own for the one shape
// that path runs at, in place of the generic collect_kernel
// (esgpu_collect.hpp), whose step loop carries multi-pass groups, the global-grid fallback, per-step prefetch scheduling
// and the whole CollectParams block for shapes this path never sees.
//
// The unit of work is a zone block (kBlockDocs docs).  Its key range comes from the zone keys (zkey, a scalar load issued
// one block ahead); the window decision and the choice between the two bodies are made once per block:
//   - a full block whose docs all round to one key inside the grid (99.4 % of the north star's blocks at 1B docs) takes
//     the unrolled body: 16 docs per thread in two buffers of 8, each reloaded for the next block right after it is
//     processed, no key arithmetic, no tail mask, no per-step decision;
//   - any other block (several keys, the segment's last partial block, a key outside the grid) takes the per-doc body,
//     which loads the keys of the thread's 16 docs: docs inside the window go to the LDS cells, the rest to the grid by
//     global atomics.  Correct for any data; it is not the fast path.
// The LDS cells are collect_kernel's packed cells ([W keys][K ranks] count << pk_shift | sum of deltas in lane-rotated
// copies cstride apart, and one (min, max) delta pair per cell), and the flush decodes them as flush_window_pi does.
#include "esgpu_ranked_cells.hpp"

namespace esgpu {

// 4 docs of a single-key block: their ranks (rk_r4) and metric deltas.  `rowm` is the LDS address of
// the block's row of (min, max) pairs, `dpk` the lane's distance from a pair to the packed word of the same cell in the
// lane's copy, `missm` the pair of the spare cell (index K * W: never flushed, its pair (0, ~0) never moves), where the
// docs whose rank is not collected go -- so every lane issues the same straight-line LDS traffic: 4 pair reads, then 4
// adds, one wait for the reads; the bound atomics only where a bound moves.  MET 1 (avg): no pairs -- `rowm` / `missm`
// then address the packed words of the lane's copy themselves and dpk is 0.
template <int MET, int RW>
__device__ __forceinline__ void rk_quad(rk_r4<RW> r, const uint32_t (&dv)[4], uint32_t K, uint32_t rowm,
                                        uint32_t missm, uint32_t dpk, uint32_t onehi) {
    uint32_t t[4];
    r.unpack(t);
    uint32_t ca[4], mlo[4], mhi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // (a rank past K, the missing rank 0xFFFF / 0xFF included, is not collected)
        ca[j] = t[j] < K ? rowm + 8u * t[j] : missm;
        if constexpr (MET >= 2) {
            const u32x2_t m = *lds_ptr<u32x2_t>(ca[j]);
            mlo[j] = m.x;
            mhi[j] = m.y;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)  // pk_shift >= 33: the packed add is the pair {delta, 1 << (pk_shift - 32)}
        atomicAdd(lds_ptr<unsigned long long>(ca[j] + dpk), join64(dv[j], onehi));
    if constexpr (MET >= 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((dv[j] < mlo[j]) | (dv[j] > mhi[j])) {
                atomicMin(lds_ptr<uint32_t>(ca[j]), dv[j]);
                atomicMax(lds_ptr<uint32_t>(ca[j] + 4u), dv[j]);
            }
        }
    }
}

// MW: bits per metric delta (RankedParams.mv: 16 d16, 12 d12 -- the 12-bit form exists with the 8-bit ranks only)
template <int MET, int RW, int MW>
__global__ __launch_bounds__(kRkWG, ESGPU_RK_WAVES) void ranked_kernel(RankedParams P) {
    static_assert(MW == 16 || (MW == 12 && RW == 1), "d12 is streamed beside rank8");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t K = P.K, W = P.W, C = K * W;
    const uint32_t ncp = max(P.ncopies, 1u);
    const uint32_t CS = P.cstride;  // > C: cell C of every copy is spare
    const rk_cells cells = rk_carve<MET>(smem, C, CS, ncp);
    unsigned long long* const pk = cells.pk;
    uint32_t* const mm = cells.mm;
    const uint32_t coff = cells.coff;

    const uint32_t b_begin = blockIdx.x * P.blocks_per_wg;
    const uint32_t b_end = min(b_begin + P.blocks_per_wg, P.n_blocks);
    if (b_begin >= b_end) return;

    const uint32_t sh = P.pk_shift;
    const uint32_t onehi = 1u << (sh - 32);
    // LDS addresses of the fast body (rk_quad)
    const uint32_t cell0 = MET >= 2 ? lds_addr(mm) : lds_addr(pk + coff);
    const uint32_t missm = cell0 + 8u * C;
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
    // the per-doc body (rk_slow_quad) over 4 docs as the block's buffers hold them: the columns are not read again
    auto slow_quad = [&](uint32_t doc0, rk_r4<RW> r, uint32_t m0, uint32_t m1, int64_t kmn, int64_t kmx) {
        rk_slow_quad<MET, RW, MW>(doc0, r, m0, m1, kmn, kmx, K, win0, win_set ? W : 0u, pk, mm, coff, sh);
    };

    // Software pipeline over the block's two buffers.  The two columns are streamed once and never read again, so
    // their loads are non-temporal: they do not displace the grid, the zone keys and the rank table in L2 / MALL (north
    // star at 1B docs 0.730 -> 0.655 ms per step with them).  Loads are unconditional and no loaded register
    // is copied, as in collect_kernel.  The zone keys are
    // read through zkey_view (scalar loads), a block ahead.  A block starts while its second buffer is in flight: the
    // loads are issued in the order ra, ma, rb, mb here and in the loop (rk_pin keeps them there), so the first half waits
    // with vmcnt(2) for ra and ma only, and the second half, behind the first buffer's reload, with vmcnt(2) for rb and mb.
    const zkey_pair_c* const zk = zkey_view(P.zkey);
    const uint32_t tid8 = threadIdx.x * kRkDocs;
    i64x2_t z = zk[__builtin_amdgcn_readfirstlane(b_begin)];
    rk_r8<RW> ra, rb;
    rk_m8<MW> ma, mb;
    ra.load(P.rank, (size_t)b_begin * kBlockDocs + tid8);
    ma.load(P.mv, (size_t)b_begin * kBlockDocs + tid8);
    rk_pin();
    rb.load(P.rank, (size_t)b_begin * kBlockDocs + kRkStepDocs + tid8);
    mb.load(P.mv, (size_t)b_begin * kBlockDocs + kRkStepDocs + tid8);
    rk_pin();
#pragma unroll 1
    for (uint32_t cb = b_begin; cb < b_end; ++cb) {
        const int64_t kmn = z.x, kmx = z.y;
        const uint32_t nb = __builtin_amdgcn_readfirstlane(min(cb + 1, b_end - 1));
        z = zk[nb];
        // (past the range's end the loads stay, but every lane reads the columns' first words: one cached line instead
        // of the last block streamed again, which the non-temporal loads would fetch from HBM a second time -- with
        // ranges of 32 blocks that was 1.5 % of traffic)
        const bool more = cb + 1 < b_end;
        const size_t nd0 = more ? (size_t)nb * kBlockDocs + tid8 : 0, nd1 = more ? nd0 + kRkStepDocs : 0;
        // (every lane reads the same zone keys: the decisions are uniform over the workgroup)
        const bool any = kmn <= kmx && kmx >= 0 && kmn < (int64_t)P.H;  // some doc of the block may lie in the grid
        if (any) {
            const bool fits = kmx - kmn < (int64_t)W;
            if (!win_set || (fits && (kmn < (int64_t)win0 || kmx >= (int64_t)win0 + (int64_t)W)))
                slide_to((uint32_t)min(max(kmn, (int64_t)0), (int64_t)P.H - 1));
        }
        const bool fast = kmn == kmx && (uint64_t)kmn < (uint64_t)P.H && (uint64_t)(cb + 1) * kBlockDocs <= P.n_docs;
        if (!fast && any) {
            const uint32_t d0 = cb * kBlockDocs + tid8;
            slow_quad(d0, ra.lo(), ma.pair(0), ma.pair(1), kmn, kmx);
            slow_quad(d0 + 4u, ra.hi(), ma.pair(2), ma.pair(3), kmn, kmx);
            slow_quad(d0 + kRkStepDocs, rb.lo(), mb.pair(0), mb.pair(1), kmn, kmx);
            slow_quad(d0 + kRkStepDocs + 4u, rb.hi(), mb.pair(2), mb.pair(3), kmn, kmx);
            rk_drain();
        }
        dirty = dirty || any;
        // each buffer has one reload per block, outside the branches: a reload under a branch gives the buffer two
        // definitions, which the compiler joins by copying the loaded registers -- a vmcnt(0) wait per block
        const uint32_t rowm = cell0 + 8u * (((uint32_t)kmn - win0) * K);
        if (fast) {
            uint32_t dv[4];
            ma.quad(0, dv);
            rk_quad<MET, RW>(ra.lo(), dv, K, rowm, missm, dpk, onehi);
            ma.quad(1, dv);
            rk_quad<MET, RW>(ra.hi(), dv, K, rowm, missm, dpk, onehi);
        }
        ra.load(P.rank, nd0);
        ma.load(P.mv, nd0);
        if (fast) {
            uint32_t dv[4];
            mb.quad(0, dv);
            rk_quad<MET, RW>(rb.lo(), dv, K, rowm, missm, dpk, onehi);
            mb.quad(1, dv);
            rk_quad<MET, RW>(rb.hi(), dv, K, rowm, missm, dpk, onehi);
        }
        rb.load(P.rank, nd1);
        mb.load(P.mv, nd1);
        rk_pin();
    }
    if (dirty) flush();
}

// rw: the rank column's width in bytes (RankedParams.rank: 1 rank8, 2 rank16); mw: the metric deltas' width in bits
// (RankedParams.mv: 16 d16, 12 d12, which goes with rw 1).  with_rk: the instantiation of a launch's (met, rw, mw).
template <typename F>
static auto with_rk(int met, int rw, int mw, F&& f) {
    if (met >= 2) {
        if (rw == 1) return mw == 12 ? f(ranked_kernel<2, 1, 12>) : f(ranked_kernel<2, 1, 16>);
        return f(ranked_kernel<2, 2, 16>);
    }
    if (rw == 1) return mw == 12 ? f(ranked_kernel<1, 1, 12>) : f(ranked_kernel<1, 1, 16>);
    return f(ranked_kernel<1, 2, 16>);
}
void launch_ranked(const RankedParams& p, int met, int rw, int mw, uint32_t grid, size_t lds, hipStream_t st) {
    with_rk(met, rw, mw, [&](auto* k) { hipLaunchKernelGGL(k, dim3(grid), dim3(kRkWG), lds, st, p); return 0; });
}
int ranked_occupancy(int met, int rw, int mw, size_t lds) {
    int n = 0;
    const hipError_t e = with_rk(met, rw, mw, [&](auto* k) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, kRkWG, lds); });
    return e == hipSuccess ? n : 1;
}

}  // namespace esgpu
