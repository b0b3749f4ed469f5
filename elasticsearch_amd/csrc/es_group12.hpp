// es_group12.hpp — the one statement of the g12 layout: a metric column's 12-bit deltas (es_pack12.hpp) with the docs of
// every zone block grouped by the frequency rank of their term (TermRanks.g12).
//
// A zone block is kG12Block docs of the padded segment.  Each doc has a group g = min(rank, kG12Groups): the ranks the
// ranked-terms collect can ask for (rank < K <= kG12Groups) keep a group each, and group kG12Groups holds every other
// doc -- ranks past it, the missing ordinal, and the pad docs past the segment's last.
//   Data:    the block's deltas permuted into ascending g, packed as es_pack12.hpp packs a column (8 positions to three
//            dwords), p12_bytes(kG12Block) bytes per block.  The order inside a group is unspecified, and what group
//            kG12Groups holds is never read.
//   Offsets: per block kG12OffStride u16 -- off[r] = the block's docs with group < r, r = 0 .. kG12Groups (off[0] = 0,
//            off[kG12Groups] <= kG12Block), then padding to a 4-byte multiple.  The docs of rank r are the positions
//            [off[r], off[r + 1]).
// A collect of the ranks below K reads the positions [0, off[K]) of a block, in whole groups of 8: g12_prefix_bytes.
// The rank of a position follows from the offsets alone (g12_rank_at): position p holds rank #{j in 1..K: off[j] <= p},
// which is K -- not collected -- from off[K] on.
// Host and device: the recode kernel (esgpu_kernels.hip), the grouped ranked kernel (esgpu_ranked_grouped.hip), the
// runtime's byte counts and the host check (check/group12_check.cpp) all go through these definitions.
#pragma once
#include "es_pack12.hpp"

constexpr uint32_t kG12Block = 8192;                            // docs per zone block (kBlockDocs)
constexpr uint32_t kG12Groups = 128;                            // ranks with a group of their own (kRankedMax)
constexpr uint32_t kG12Offs = kG12Groups + 1;                   // offsets per block
constexpr uint32_t kG12OffStride = (kG12Offs + 1u) & ~1u;       // u16 per block, padded to a 4-byte multiple
constexpr uint32_t kG12OffBytes = kG12OffStride * 2;            // 260
constexpr uint32_t kG12Missing = 0xFFFFu;                       // rank16 of a doc without a term

ES_P12_HD uint32_t g12_group(uint32_t rank) { return rank < kG12Groups ? rank : kG12Groups; }
ES_P12_HD uint64_t g12_ceil8(uint64_t n) { return (n + (kP12Group - 1)) & ~(uint64_t)(kP12Group - 1); }
ES_P12_HD size_t g12_block_bytes() { return p12_bytes(kG12Block); }
ES_P12_HD size_t g12_data_bytes(size_t n_blocks) { return n_blocks * g12_block_bytes(); }
ES_P12_HD size_t g12_off_bytes(size_t n_blocks) { return n_blocks * kG12OffBytes; }
// bytes of a block's data a collect of the ranks below K streams: the groups of 8 that hold positions below n = off[K]
ES_P12_HD size_t g12_prefix_bytes(uint64_t n) { return p12_bytes((size_t)g12_ceil8(n)); }
// the group of 8 a thread that holds the positions p0 .. p0 + 7 (p0 a multiple of 8, < kG12Block) loads from a block
// with n = off[K]: its own where that holds a collected position, otherwise group 0 -- always inside the block's data,
// and re-read by the thread that owns it (the grouped kernel's loads are unconditional; what such a thread gets it
// ignores).  The byte offset inside the block is kP12Words * 4 times this.
ES_P12_HD uint32_t g12_load_group(uint32_t p0, uint32_t n) { return p0 < n ? p0 / kP12Group : 0u; }

// the rank of position p for a collect of the ranks below K (K <= kG12Groups): off(j) gives the block's off[j]
template <class OffAt>
ES_P12_HD uint32_t g12_rank_at(uint32_t p, uint32_t K, OffAt off) {
    uint32_t r = 0;
    for (uint32_t j = 1; j <= K; ++j) r += off(j) <= p ? 1u : 0u;
    return r;
}
// ... of the 8 positions p0 .. p0 + 7 of one packed group at once (the kernel's form: one pass over the offsets).  A
// caller that knows the rank `base` of an earlier position w <= p0 and the count `upto` of offsets below some position
// past p0 + 7 passes only the offsets between them: base = #{j: off[j] <= w}, upto = #{j: off[j] < e}, e > p0 + 7 -- the
// offsets off[base + 1 .. upto] are those inside (w, e), the others cannot tell the 8 positions apart.  (A wave of the
// kernel takes both counts for its 512 positions from two ballots.)  base 0, upto K: every offset.
template <class OffAt>
ES_P12_HD void g12_ranks8(uint32_t p0, uint32_t base, uint32_t upto, OffAt off, uint32_t (&r)[8]) {
    for (int i = 0; i < 8; ++i) r[i] = base;
    for (uint32_t j = base + 1; j <= upto; ++j) {
        const uint32_t o = off(j);
        for (int i = 0; i < 8; ++i) r[i] += o <= p0 + (uint32_t)i ? 1u : 0u;
    }
}

// Host reference: one block grouped.  rank / d: the block's n (<= kG12Block) docs -- their 16-bit ranks (kG12Missing: no
// term) and deltas (< 4096); positions past n are pad docs.  out: g12_block_bytes() bytes; off: kG12OffStride entries.
// Stable: the docs of a group keep their order (the recode kernel promises no order).
inline void g12_group_block(const uint16_t* rank, const uint16_t* d, uint32_t n, uint8_t* out, uint16_t* off) {
    uint32_t count[kG12Offs] = {};
    for (uint32_t i = 0; i < kG12Block; ++i) ++count[i < n ? g12_group(rank[i]) : kG12Groups];
    uint32_t cursor[kG12Offs], acc = 0;
    for (uint32_t g = 0; g < kG12Offs; ++g) {
        off[g] = (uint16_t)acc;
        cursor[g] = acc;
        acc += count[g];
    }
    for (uint32_t g = kG12Offs; g < kG12OffStride; ++g) off[g] = 0;
    uint16_t staged[kG12Block];
    for (uint32_t i = 0; i < kG12Block; ++i) {
        const uint32_t g = i < n ? g12_group(rank[i]) : kG12Groups;
        staged[cursor[g]++] = i < n ? (uint16_t)(d[i] & kP12Mask) : (uint16_t)0;
    }
    p12_pack(staged, kG12Block, out);
}
