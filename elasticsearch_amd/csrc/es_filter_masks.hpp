// Filter clauses as key intervals, and the mask tables of a filters aggregation (host only, no device dependencies:
// csrc/check/filters_check.cpp runs it stand-alone).
//
// A clause (ESGPU_FILTER_TERM / ESGPU_FILTER_RANGE) over a single-valued column accepts exactly the docs whose value's
// key lies in one inclusive interval [lo, hi] of signed 64-bit keys:
//   long / date column   the key is the value; an exclusive bound steps by one, gt(INT64_MAX) and lt(INT64_MIN) are empty;
//                        a bound whose lo_d / hi_d is infinite is that infinity (no long reaches +Infinity: a lower
//                        bound there is empty, an upper one no bound), whatever lo_i / hi_i hold
//   keyword column       the key is the ordinal; a term is [ord, ord] (-1, a term absent from the dictionary, lies outside
//                        the ordinals), a TermRangeQuery an ordinal range of the segment's sorted dictionary
//   double column        the key is the bits, sign-folded (fm_f64_key: ascending with the value, -0.0 just below 0.0);
//                        IEEE comparisons: both zeros satisfy every bound at either zero alike, a NaN bound accepts
//                        nothing, +-Infinity compare as values
// set_preds (the clause predicates of the collect kernels) and the filters collect (path 12) share these.
//
// build_filter_masks cuts one column's key line at the bounds of the clauses on it: interval k holds the keys with
// exactly k cuts <= key, and its u64 mask has bit i set iff every clause of filter i on the column accepts the interval
// (a filter without a clause there: everywhere; two clauses of one filter intersect, possibly to nothing).  One more
// mask is for a doc without a value in the column -- a clear present bit, the missing ordinal, NaN: the filters without
// a clause on the column.  A doc's filters are the AND of its masks over the clause columns.
//
// A bool query (ESGPU_FILTER_TERMS / EXISTS / BOOL, occur, group) uses the same tables with the leaf as the slot:
// build_leaf_masks lets a leaf accept a union of intervals, BoolComb / bool_comb_match evaluate the owner's clauses on a
// doc's leaf mask (csrc/check/bool_query_check.cpp runs them stand-alone; esgpu_bool_bits.hip on the device).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/esgpu.h"

struct KeyInterval {
    int64_t lo, hi;  // inclusive; lo > hi: empty
    bool empty() const { return lo > hi; }
    bool holds(int64_t k) const { return lo <= k && k <= hi; }
};
inline KeyInterval key_intersect(KeyInterval a, KeyInterval b) { return {std::max(a.lo, b.lo), std::min(a.hi, b.hi)}; }

// a clause over a long / date column (a term is the degenerate range [t, t])
inline KeyInterval fm_long_interval(const esgpu_filter& f) {
    if (f.type == ESGPU_FILTER_TERM) return {f.term, f.term};
    int64_t lo = INT64_MIN, hi = INT64_MAX;
    bool empty = false;
    const double inf = __builtin_inf();
    if (f.has_lower && (f.lo_d == inf || f.lo_d == -inf)) {
        empty = f.lo_d > 0;  // v >= +Infinity holds for no long, v >= -Infinity for every one
    } else if (f.has_lower) {
        if (f.include_lower) lo = f.lo_i;
        else if (f.lo_i == INT64_MAX) empty = true;
        else lo = f.lo_i + 1;
    }
    if (f.has_upper && (f.hi_d == inf || f.hi_d == -inf)) {
        empty = empty || f.hi_d < 0;
    } else if (f.has_upper) {
        if (f.include_upper) hi = f.hi_i;
        else if (f.hi_i == INT64_MIN) empty = true;
        else hi = f.hi_i - 1;
    }
    if (empty) { lo = 1; hi = 0; }
    return {lo, hi};
}

// a TermRangeQuery over a keyword column of n ordinals: the dictionary is sorted by unsigned bytes, so the range is an
// ordinal range.  less(bytes, len, ord, strict): term(ord) < the bytes (strict) or term(ord) <= the bytes.
template <class Less>
inline KeyInterval fm_ord_range(const esgpu_filter& f, uint64_t n, Less less) {
    auto bound = [&](const uint8_t* t, uint64_t len, bool upper) {  // first ord with term > t (upper) / >= t
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (less(t, len, mid, !upper)) lo = mid + 1; else hi = mid;
        }
        return (int64_t)lo;
    };
    KeyInterval r{0, (int64_t)n - 1};
    if (f.has_lower) r.lo = bound(f.lo_term, f.lo_term_len, !f.include_lower);
    if (f.has_upper) r.hi = bound(f.hi_term, f.hi_term_len, f.include_upper) - 1;
    return r;
}
// the ordinals a doc can hold (0xFFFFFFFF is the missing ordinal)
constexpr KeyInterval kOrdDomain{0, 0xFFFFFFFEll};

// a clause over a double column as the comparison the predicate kernels make: lo_incl ? v >= lo : v > lo, and the same
// above; a term is [t, t] on (double) term
struct F64Bounds {
    double lo, hi;
    int32_t lo_incl, hi_incl;
};
inline F64Bounds fm_f64_bounds(const esgpu_filter& f) {
    if (f.type == ESGPU_FILTER_TERM) return {(double)f.term, (double)f.term, 1, 1};
    const double inf = __builtin_inf();
    return {f.has_lower ? f.lo_d : -inf, f.has_upper ? f.hi_d : inf, f.has_lower ? f.include_lower : 1,
            f.has_upper ? f.include_upper : 1};
}
// the signed key doubles compare by: the bits with the magnitude of a negative value inverted
inline int64_t fm_f64_key(double d) {
    int64_t b;
    std::memcpy(&b, &d, 8);
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFll);
}
// the keys of -Infinity .. +Infinity: every value a clause can accept (NaN keys lie outside on both sides)
inline KeyInterval fm_f64_domain() { return {fm_f64_key(-__builtin_inf()), fm_f64_key(__builtin_inf())}; }
inline KeyInterval fm_f64_interval(const F64Bounds& b) {
    if (b.lo != b.lo || b.hi != b.hi) return {1, 0};  // every comparison with NaN is false
    // the two zeros are one value: an inclusive bound at either reaches both keys (-1 and 0), an exclusive one neither
    KeyInterval r;
    if (b.lo == 0.0) r.lo = b.lo_incl ? -1 : 1;
    else r.lo = fm_f64_key(b.lo) + (b.lo_incl ? 0 : 1);
    if (b.hi == 0.0) r.hi = b.hi_incl ? 0 : -2;
    else r.hi = fm_f64_key(b.hi) - (b.hi_incl ? 0 : 1);
    return key_intersect(r, fm_f64_domain());
}

// ---- the mask table of one clause column -----------------------------------------------------------------------------
constexpr uint32_t kFilterMaskCuts = 128;                         // distinct cuts per column at most
constexpr uint32_t kFilterMaskStride = 2 * kFilterMaskCuts + 2;   // u64 per column: cuts, masks [cuts + 1], the no-value mask
constexpr uint32_t kFilterMaskNoValue = 2 * kFilterMaskCuts + 1;

struct FilterClause {
    int32_t slot;    // the filter it belongs to: bit `slot` of the masks
    KeyInterval iv;
};

// table[kFilterMaskStride] of a column from the clauses on it; `domain`: the keys a doc of the column can hold (clauses
// are clipped to it).  false: more than kFilterMaskCuts distinct cuts.
inline bool build_filter_masks(const std::vector<FilterClause>& clauses, int32_t n_filters, KeyInterval domain, uint64_t* table,
                               uint32_t* n_cuts) {
    const uint64_t all = n_filters >= 64 ? ~0ull : (1ull << n_filters) - 1ull;
    std::vector<int64_t> cuts;
    uint64_t with_clause = 0;
    for (const FilterClause& c : clauses) {
        with_clause |= 1ull << c.slot;
        const KeyInterval iv = key_intersect(c.iv, domain);
        if (iv.empty()) continue;
        if (iv.lo > INT64_MIN) cuts.push_back(iv.lo);
        if (iv.hi < INT64_MAX) cuts.push_back(iv.hi + 1);
    }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    if (cuts.size() > kFilterMaskCuts) return false;
    std::fill(table, table + kFilterMaskStride, 0ull);
    const uint32_t n = (uint32_t)cuts.size();
    for (uint32_t k = 0; k < n; ++k) table[k] = (uint64_t)cuts[k];
    for (uint32_t k = 0; k <= n; ++k) {
        // every bound is a cut, so an interval lies wholly inside or outside each clause: its least key decides
        const int64_t rep = k == 0 ? INT64_MIN : cuts[k - 1];
        uint64_t m = all;
        for (const FilterClause& c : clauses)
            if (!key_intersect(c.iv, domain).holds(rep)) m &= ~(1ull << c.slot);
        table[kFilterMaskCuts + k] = m;
    }
    table[kFilterMaskNoValue] = all & ~with_clause;
    *n_cuts = n;
    return true;
}

// ---- the leaves of a bool query ---------------------------------------------------------------------------------------
// A bool query's leaf (term, range, terms, exists) is the slot of the same tables: bit i of a doc's mask says that leaf i
// holds for the doc.  A leaf has a clause only on its own column and is all ones on the others, so the AND over the
// columns is the doc's leaf mask.  A terms leaf is a union of [t, t]; exists is the whole domain.
struct LeafClause {
    int32_t slot;                  // the leaf: bit `slot` of the masks
    std::vector<KeyInterval> ivs;  // the keys it accepts: their union (none: an empty terms list, no key)
    bool exists = false;           // an exists leaf: see nan_is_value below
};

// build_filter_masks with a union of intervals per leaf.  The no-value mask is for a doc without a value in the column:
// the leaves without a clause on it.  nan_is_value (a double column, whose lookup hands a NaN the no-value mask too): the
// exists leaves are set in it as well, and *exists_mask names them -- the caller clears them for a doc whose present bit
// is clear.  false: more than kFilterMaskCuts distinct cuts.
inline bool build_leaf_masks(const std::vector<LeafClause>& leaves, int32_t n_leaves, KeyInterval domain, bool nan_is_value,
                             uint64_t* table, uint32_t* n_cuts, uint64_t* exists_mask) {
    const uint64_t all = n_leaves >= 64 ? ~0ull : (1ull << n_leaves) - 1ull;
    std::vector<int64_t> cuts;
    std::vector<std::vector<KeyInterval>> clipped(leaves.size());
    uint64_t with_clause = 0, ex = 0;
    for (size_t i = 0; i < leaves.size(); ++i) {
        with_clause |= 1ull << leaves[i].slot;
        if (leaves[i].exists) ex |= 1ull << leaves[i].slot;
        for (const KeyInterval& raw : leaves[i].ivs) {
            KeyInterval iv = key_intersect(raw, domain);
            if (iv.empty()) continue;
            // the whole domain is the whole key line (no key outside it is looked up): no cut
            if (iv.lo == domain.lo && iv.hi == domain.hi) iv = {INT64_MIN, INT64_MAX};
            clipped[i].push_back(iv);
            if (iv.lo > INT64_MIN) cuts.push_back(iv.lo);
            if (iv.hi < INT64_MAX) cuts.push_back(iv.hi + 1);
        }
    }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    if (cuts.size() > kFilterMaskCuts) return false;
    std::fill(table, table + kFilterMaskStride, 0ull);
    const uint32_t n = (uint32_t)cuts.size();
    for (uint32_t k = 0; k < n; ++k) table[k] = (uint64_t)cuts[k];
    for (uint32_t k = 0; k <= n; ++k) {
        // every bound is a cut, so an elementary interval lies wholly inside or outside each leaf interval
        const int64_t rep = k == 0 ? INT64_MIN : cuts[k - 1];
        uint64_t m = all;
        for (size_t i = 0; i < leaves.size(); ++i) {
            bool holds = false;
            for (const KeyInterval& iv : clipped[i]) holds = holds || iv.holds(rep);
            if (!holds) m &= ~(1ull << leaves[i].slot);
        }
        table[kFilterMaskCuts + k] = m;
    }
    table[kFilterMaskNoValue] = (all & ~with_clause) | (nan_is_value ? ex : 0ull);
    *n_cuts = n;
    *exists_mask = nan_is_value ? ex : 0ull;
    return true;
}

// The combinator of one owner's clauses over a doc's leaf mask (BoolQueryBuilder.doToQuery, Queries.applyMinimumShouldMatch
// / fixNegativeQueryIfNeeded, BooleanQuery's matching rules).  A clause is one leaf or a group of leaves that holds when
// any of them holds (a nested bool of should leaves).
constexpr uint32_t kBoolLeaves = 64;
constexpr uint32_t kBoolGroups = kBoolLeaves / 2;  // multi-leaf clauses at most
struct BoolComb {
    uint64_t must;                 // the single-leaf required clauses (must and filter alike)
    uint64_t must_not;             // every prohibited leaf (a prohibited group is an OR: one mask covers all of them)
    uint64_t should;               // the single-leaf optional clauses, counted by popcount
    uint64_t group[kBoolGroups];   // multi-leaf clauses: the first n_must_groups required, the others optional
    uint32_t n_must_groups, n_groups;
    int32_t m;                     // optional clauses that must hold at least
    int32_t match_none;            // only prohibited clauses and adjust_pure_negative false
};

#if defined(__HIPCC__)
#define FM_HD __host__ __device__ inline
#else
#define FM_HD inline
#endif
FM_HD bool bool_comb_match(const BoolComb& c, uint64_t leaves) {
    bool ok = !c.match_none && (leaves & c.must) == c.must && (leaves & c.must_not) == 0;
    int32_t opt = __builtin_popcountll(leaves & c.should);
    for (uint32_t g = 0; g < c.n_groups; ++g) {
        const bool holds = (leaves & c.group[g]) != 0;
        if (g < c.n_must_groups) ok = ok && holds;
        else opt += holds ? 1 : 0;
    }
    return ok && opt >= c.m;
}
#undef FM_HD

// one clause of an owner as the C-ABI states it: the leaves' bits (one bit: a leaf by itself; more: a group) and its occur
struct BoolClauseBits {
    uint64_t leaves;
    int32_t occur;  // ESGPU_OCCUR_*
};
// m as BooleanQuery applies it: the resolved minimum_should_match when it is > 0 (msm < 0: not given), else 1 when there
// is no required clause and an optional one, else 0.  No clause at all is match_all; only prohibited clauses match the
// docs none of them holds for when adjust_pure_negative, else no doc.
inline BoolComb make_bool_comb(const std::vector<BoolClauseBits>& clauses, int64_t msm, bool adjust_pure_negative) {
    BoolComb c{};
    uint32_t n_must = 0, n_should = 0, n_not = 0;
    for (int pass = 0; pass < 2; ++pass)  // required groups first
        for (const BoolClauseBits& cl : clauses) {
            const bool multi = (cl.leaves & (cl.leaves - 1)) != 0;
            if (cl.occur == ESGPU_OCCUR_MUST_NOT) {
                if (pass == 0) { c.must_not |= cl.leaves; ++n_not; }
                continue;
            }
            const bool must = cl.occur == ESGPU_OCCUR_MUST;
            if (pass == 0) (must ? n_must : n_should) += 1;
            if (!multi) {
                if (pass == 0) (must ? c.must : c.should) |= cl.leaves;
            } else if (must == (pass == 0)) {
                c.group[c.n_groups++] = cl.leaves;
                if (must) ++c.n_must_groups;
            }
        }
    c.m = msm > 0 ? (int32_t)std::min<int64_t>(msm, INT32_MAX) : (n_must == 0 && n_should > 0 ? 1 : 0);
    if (clauses.empty()) c.m = 0;  // match_all, whatever minimum_should_match says (doToQuery returns before applying it)
    c.match_none = n_not > 0 && n_must == 0 && n_should == 0 && !adjust_pure_negative;
    return c;
}

// the lookup the kernel makes (branch-free binary search): the mask of the interval with exactly k cuts <= key
inline uint64_t filter_mask_lookup(const uint64_t* table, uint32_t n_cuts, int64_t key) {
    uint32_t k = 0, step = 1;
    while (step * 2 <= n_cuts) step *= 2;
    for (; n_cuts && step; step >>= 1) {
        const uint32_t t = k + step;
        if (t <= n_cuts && (int64_t)table[t - 1] <= key) k = t;
    }
    return table[kFilterMaskCuts + k];
}
