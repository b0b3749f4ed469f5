// bool_query_check.cpp — a stand-alone exercise of the host code behind bool queries, meant to be built with
// -fsanitize=address,undefined (make -C elasticsearch_amd/csrc check-bool-query): the union builder (build_leaf_masks)
// and the combinator (make_bool_comb, bool_comb_match) of es_filter_masks.hpp against brute-force evaluation of the leaves
// on the values themselves and of the clauses on the leaves -- random leaves (term, range, terms, exists) on a long, a
// double and an ordinal column with random occurs and groups, 64 leaves, 128 cuts and one more, the two zeros, NaN under
// a set and a clear present bit, the INT64 edges and an empty terms list.  The lookup is the kernel's: the table entry of
// the value's key, the no-value mask for a doc without a value and for a NaN, the exists bits of a double column cleared
// where the present bit is clear.  Needs no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>
#include <vector>

#include "../es_filter_masks.hpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

constexpr uint32_t kMissing = 0xFFFFFFFFu;
static const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

struct Doc {
    int64_t l; bool has_l;
    double d; bool has_d;
    uint32_t o;
};
struct Leaf {
    int col;  // 0 long, 1 double, 2 ordinal
    esgpu_filter f;
    std::vector<int64_t> terms;
};

// ---- brute force: a leaf on the value itself ---------------------------------------------------------------------------
static bool long_holds(const Leaf& L, int64_t v) {
    const esgpu_filter& f = L.f;
    if (f.type == ESGPU_FILTER_EXISTS) return true;
    if (f.type == ESGPU_FILTER_TERM) return v == f.term;
    if (f.type == ESGPU_FILTER_TERMS) {
        for (int64_t t : L.terms) if (v == t) return true;
        return false;
    }
    if (f.has_lower && !(f.include_lower ? v >= f.lo_i : v > f.lo_i)) return false;
    if (f.has_upper && !(f.include_upper ? v <= f.hi_i : v < f.hi_i)) return false;
    return true;
}
static bool double_holds(const Leaf& L, double v) {  // IEEE comparisons; a NaN is a value only for exists
    const esgpu_filter& f = L.f;
    if (f.type == ESGPU_FILTER_EXISTS) return true;
    if (f.type == ESGPU_FILTER_TERM) return v == (double)f.term;
    if (f.type == ESGPU_FILTER_TERMS) {
        for (int64_t t : L.terms) if (v == (double)t) return true;
        return false;
    }
    if (f.has_lower && !(f.include_lower ? v >= f.lo_d : v > f.lo_d)) return false;
    if (f.has_upper && !(f.include_upper ? v <= f.hi_d : v < f.hi_d)) return false;
    return !(v != v);
}
static bool ord_holds(const Leaf& L, uint32_t o) {
    const esgpu_filter& f = L.f;
    if (f.type == ESGPU_FILTER_EXISTS) return true;
    if (f.type == ESGPU_FILTER_TERM) return (int64_t)o == f.term;
    if (f.type == ESGPU_FILTER_TERMS) {
        for (int64_t t : L.terms) if ((int64_t)o == t) return true;
        return false;
    }
    return (!f.has_lower || (int64_t)o >= f.lo_i) && (!f.has_upper || (int64_t)o <= f.hi_i);  // (an ordinal range, inclusive)
}
static bool leaf_holds(const Leaf& L, const Doc& d) {
    if (L.col == 0) return d.has_l && long_holds(L, d.l);
    if (L.col == 1) return d.has_d && double_holds(L, d.d);
    return d.o != kMissing && ord_holds(L, d.o);
}

// ---- the tables, as the runtime builds them ----------------------------------------------------------------------------
static LeafClause leaf_clause(const Leaf& L, int slot) {
    LeafClause lc;
    lc.slot = slot;
    const esgpu_filter& f = L.f;
    auto term_iv = [&](int64_t t) { return L.col == 1 ? fm_f64_interval(F64Bounds{(double)t, (double)t, 1, 1}) : KeyInterval{t, t}; };
    if (f.type == ESGPU_FILTER_EXISTS) {
        lc.exists = true;
        lc.ivs.push_back({INT64_MIN, INT64_MAX});
    } else if (f.type == ESGPU_FILTER_TERMS) {
        for (int64_t t : L.terms) lc.ivs.push_back(term_iv(t));
    } else if (f.type == ESGPU_FILTER_TERM) {
        lc.ivs.push_back(term_iv(f.term));
    } else if (L.col == 2) {
        lc.ivs.push_back({f.has_lower ? f.lo_i : INT64_MIN, f.has_upper ? f.hi_i : INT64_MAX});
    } else {
        lc.ivs.push_back(L.col == 1 ? fm_f64_interval(fm_f64_bounds(f)) : fm_long_interval(f));
    }
    return lc;
}

struct Tables {
    std::vector<uint64_t> table[3];
    uint32_t n_cuts[3] = {0, 0, 0};
    uint64_t ex[3] = {0, 0, 0};
    bool used[3] = {false, false, false};
    uint64_t all = 0;
};
static bool build(const std::vector<Leaf>& leaves, Tables& T) {
    const int n = (int)leaves.size();
    T.all = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    for (int col = 0; col < 3; ++col) {
        std::vector<LeafClause> lcs;
        for (int i = 0; i < n; ++i) if (leaves[i].col == col) lcs.push_back(leaf_clause(leaves[i], i));
        if (lcs.empty()) continue;
        T.used[col] = true;
        T.table[col].assign(kFilterMaskStride, 0xDEADBEEFull);
        const KeyInterval domain = col == 2 ? kOrdDomain : col == 1 ? fm_f64_domain() : KeyInterval{INT64_MIN, INT64_MAX};
        if (!build_leaf_masks(lcs, n, domain, col == 1, T.table[col].data(), &T.n_cuts[col], &T.ex[col])) return false;
    }
    return true;
}
// the kernel's doc mask
static uint64_t doc_mask(const Tables& T, const Doc& d) {
    uint64_t m = ~0ull;
    for (int col = 0; col < 3; ++col) {
        if (!T.used[col]) continue;
        const uint64_t* tab = T.table[col].data();
        bool has;
        int64_t key;
        if (col == 0) { has = d.has_l; key = d.l; }
        else if (col == 1) { has = d.has_d && !(d.d != d.d); key = fm_f64_key(d.d); }
        else { has = d.o != kMissing; key = (int64_t)d.o; }
        m &= has ? filter_mask_lookup(tab, T.n_cuts[col], key) : tab[kFilterMaskNoValue];
        if (col == 1 && !d.has_d) m &= ~T.ex[col];
    }
    return m & T.all;
}

// ---- brute force: the clauses on the leaves ----------------------------------------------------------------------------
static bool brute_match(const std::vector<Leaf>& leaves, const Doc& d, int64_t msm, bool adjust) {
    std::map<std::pair<int, int>, bool> grouped;  // (group, occur) -> holds
    int n_must = 0, n_should = 0, n_not = 0, should_held = 0;
    bool ok = true;
    auto clause = [&](int occur, bool holds) {
        if (occur == ESGPU_OCCUR_MUST) { ++n_must; ok = ok && holds; }
        else if (occur == ESGPU_OCCUR_MUST_NOT) { ++n_not; ok = ok && !holds; }
        else { ++n_should; should_held += holds ? 1 : 0; }
    };
    for (const Leaf& L : leaves) {
        const bool h = leaf_holds(L, d);
        if (L.f.group > 0) {
            auto it = grouped.emplace(std::make_pair(L.f.group, L.f.occur), false).first;
            it->second = it->second || h;
        } else {
            clause(L.f.occur, h);
        }
    }
    for (const auto& g : grouped) clause(g.first.second, g.second);
    if (n_must + n_should + n_not == 0) return true;
    if (n_must + n_should == 0 && !adjust) return false;
    const int64_t m = msm > 0 ? msm : (n_must == 0 && n_should > 0 ? 1 : 0);
    return ok && should_held >= m;
}
static BoolComb comb_of(const std::vector<Leaf>& leaves, int64_t msm, bool adjust) {
    std::vector<BoolClauseBits> clauses;
    std::map<std::pair<int, int>, size_t> groups;
    for (size_t i = 0; i < leaves.size(); ++i) {
        const esgpu_filter& f = leaves[i].f;
        auto at = f.group > 0 ? groups.find({f.group, f.occur}) : groups.end();
        if (at == groups.end()) {
            if (f.group > 0) groups[{f.group, f.occur}] = clauses.size();
            clauses.push_back({1ull << i, f.occur});
        } else {
            clauses[at->second].leaves |= 1ull << i;
        }
    }
    return make_bool_comb(clauses, msm, adjust);
}

static std::vector<Doc> docs() {
    const std::vector<int64_t> lp = {INT64_MIN, INT64_MIN + 1, -2, -1, 0, 1, 2, 7, 100, INT64_MAX - 1, INT64_MAX};
    const std::vector<double> dp = {-kInf, -1.7976931348623157e308, -1.5, -4.9e-324, -0.0, 0.0, 4.9e-324, 1.0, 1.5, 2.0, 7.0, kInf, kNaN, -kNaN};
    const std::vector<uint32_t> op = {0, 1, 2, 3, 7, 0xFFFFFFFEu, kMissing};
    std::vector<Doc> out;
    for (size_t i = 0; i < lp.size() * 2; ++i)
        for (size_t j = 0; j < dp.size() * 2; ++j)
            out.push_back({lp[i / 2], i % 2 == 0, dp[j / 2], j % 2 == 0, op[(i + j) % op.size()]});
    return out;
}

static void check_all(const std::vector<Leaf>& leaves, int64_t msm, bool adjust, uint64_t* checked) {
    Tables T;
    CHECK(build(leaves, T));
    const BoolComb c = comb_of(leaves, msm, adjust);
    static const std::vector<Doc> D = docs();
    for (const Doc& d : D) {
        const uint64_t m = doc_mask(T, d);
        for (size_t i = 0; i < leaves.size(); ++i) CHECK(((m >> i) & 1ull) == (leaf_holds(leaves[i], d) ? 1ull : 0ull));
        CHECK(bool_comb_match(c, m) == brute_match(leaves, d, msm, adjust));
        ++*checked;
    }
}

static Leaf random_leaf(std::mt19937_64& rng, bool flat) {
    const std::vector<int64_t> lp = {INT64_MIN, INT64_MIN + 1, -2, -1, 0, 1, 2, 7, 100, INT64_MAX - 1, INT64_MAX};
    const std::vector<double> dp = {-kInf, -1.5, -0.0, 0.0, 4.9e-324, 1.5, 2.0, kInf, kNaN};
    auto pick = [&](size_t n) { return (size_t)(rng() % n); };
    Leaf L{};
    L.col = (int)pick(3);
    esgpu_filter& f = L.f;
    f.type = (int32_t)(1 + pick(4));
    f.occur = (int32_t)pick(3);
    f.group = flat ? 0 : (int32_t)pick(4);
    f.has_lower = (int32_t)pick(2);
    f.has_upper = (int32_t)pick(2);
    f.include_lower = (int32_t)pick(2);
    f.include_upper = (int32_t)pick(2);
    if (L.col == 0) {
        f.term = lp[pick(lp.size())];
        f.lo_i = lp[pick(lp.size())];
        f.hi_i = lp[pick(lp.size())];
        for (size_t k = pick(5); k > 0; --k) L.terms.push_back(lp[pick(lp.size())]);
    } else if (L.col == 1) {
        f.term = (int64_t)pick(4) - 1;
        f.lo_d = dp[pick(dp.size())];
        f.hi_d = dp[pick(dp.size())];
        for (size_t k = pick(5); k > 0; --k) L.terms.push_back((int64_t)pick(9) - 1);
    } else {
        f.term = (int64_t)pick(10) - 1;  // -1: a term absent from the dictionary
        f.lo_i = (int64_t)pick(9);
        f.hi_i = (int64_t)pick(9);
        for (size_t k = pick(5); k > 0; --k) L.terms.push_back((int64_t)pick(10) - 1);
    }
    return L;
}

int main() {
    std::mt19937_64 rng(0x5EED);
    uint64_t checked = 0;
    // random leaves, occurs and groups
    for (int round = 0; round < 400; ++round) {
        std::vector<Leaf> leaves;
        const size_t n = rng() % 9;  // (0: the empty bool)
        for (size_t i = 0; i < n; ++i) leaves.push_back(random_leaf(rng, round % 2 == 0));
        const int64_t msm = (int64_t)(rng() % 5) - 1;
        check_all(leaves, msm, rng() % 2 == 0, &checked);
    }
    // 64 leaves: every bit, bit 63 included
    for (int round = 0; round < 10; ++round) {
        std::vector<Leaf> leaves;
        for (int i = 0; i < 64; ++i) {
            Leaf L = random_leaf(rng, false);
            if (L.f.type == ESGPU_FILTER_RANGE || L.f.type == ESGPU_FILTER_TERMS) L.f.type = ESGPU_FILTER_TERM;  // (few cuts)
            leaves.push_back(L);
        }
        check_all(leaves, (int64_t)(rng() % 4), true, &checked);
    }
    {   // a 64-value terms leaf is 128 cuts; one more value is refused
        Leaf L{};
        L.col = 0;
        L.f.type = ESGPU_FILTER_TERMS;
        L.f.occur = ESGPU_OCCUR_SHOULD;
        for (int k = 0; k < 64; ++k) L.terms.push_back(-50 + 3 * k);
        Tables T;
        CHECK(build({L}, T) && T.n_cuts[0] == 128);
        check_all({L}, -1, true, &checked);
        L.terms.push_back(1000);
        Tables T2;
        CHECK(!build({L}, T2));
        L.terms.back() = -50 + 3;  // (a repeated value adds no cut)
        CHECK(build({L}, T2));
    }
    {   // an empty terms list matches no doc; prohibited, it matches every doc
        Leaf L{};
        L.col = 0;
        L.f.type = ESGPU_FILTER_TERMS;
        for (int occur = 0; occur < 3; ++occur) {
            L.f.occur = occur;
            Tables T;
            CHECK(build({L}, T) && T.n_cuts[0] == 0);
            const BoolComb c = comb_of({L}, -1, true);
            for (const Doc& d : docs()) {
                CHECK(doc_mask(T, d) == 0);
                CHECK(bool_comb_match(c, doc_mask(T, d)) == (occur == ESGPU_OCCUR_MUST_NOT));
            }
            check_all({L}, -1, true, &checked);
        }
    }
    {   // the two zeros are one value; exists on a double column: a NaN counts, a doc without a value does not
        Leaf z{};
        z.col = 1;
        z.f.type = ESGPU_FILTER_TERMS;
        z.terms = {0};
        Leaf e{};
        e.col = 1;
        e.f.type = ESGPU_FILTER_EXISTS;
        Tables T;
        CHECK(build({z, e}, T) && T.ex[1] == 2);
        CHECK(doc_mask(T, {0, false, -0.0, true, 0}) == 3 && doc_mask(T, {0, false, 0.0, true, 0}) == 3);
        CHECK(doc_mask(T, {0, false, kNaN, true, 0}) == 2 && doc_mask(T, {0, false, kNaN, false, 0}) == 0);
        CHECK(doc_mask(T, {0, false, 0.0, false, 0}) == 0 && doc_mask(T, {0, false, 4.9e-324, true, 0}) == 2);
        check_all({z, e}, -1, true, &checked);
    }
    {   // the INT64 edges: terms and ranges at both ends, exists beside them (no cut for a whole-domain leaf)
        Leaf t{};
        t.col = 0;
        t.f.type = ESGPU_FILTER_TERMS;
        t.terms = {INT64_MIN, INT64_MAX};
        Leaf r{};
        r.col = 0;
        r.f.type = ESGPU_FILTER_RANGE;
        r.f.has_lower = r.f.has_upper = 1;
        r.f.include_lower = r.f.include_upper = 1;
        r.f.lo_i = INT64_MIN;
        r.f.hi_i = INT64_MAX;
        Leaf e{};
        e.col = 0;
        e.f.type = ESGPU_FILTER_EXISTS;
        Tables T;
        CHECK(build({t, r, e}, T) && T.n_cuts[0] == 2);
        CHECK(doc_mask(T, {INT64_MIN, true, 0, false, 0}) == 7 && doc_mask(T, {INT64_MAX, true, 0, false, 0}) == 7);
        CHECK(doc_mask(T, {0, true, 0, false, 0}) == 6 && doc_mask(T, {0, false, 0, false, 0}) == 0);
        check_all({t, r, e}, 2, true, &checked);
    }
    {   // m: the default, a given one, more than the optional clauses; pure negative both ways
        CHECK(make_bool_comb({{1, ESGPU_OCCUR_SHOULD}, {2, ESGPU_OCCUR_SHOULD}}, -1, true).m == 1);
        CHECK(make_bool_comb({{1, ESGPU_OCCUR_SHOULD}, {2, ESGPU_OCCUR_MUST}}, -1, true).m == 0);
        CHECK(make_bool_comb({{1, ESGPU_OCCUR_SHOULD}, {2, ESGPU_OCCUR_MUST}}, 0, true).m == 0);
        CHECK(make_bool_comb({{1, ESGPU_OCCUR_SHOULD}, {2, ESGPU_OCCUR_MUST}}, 1, true).m == 1);
        const BoolComb over = make_bool_comb({{1, ESGPU_OCCUR_SHOULD}}, 2, true);
        CHECK(!bool_comb_match(over, 1) && !bool_comb_match(over, 0));
        const BoolComb neg = make_bool_comb({{1, ESGPU_OCCUR_MUST_NOT}}, -1, true), none = make_bool_comb({{1, ESGPU_OCCUR_MUST_NOT}}, -1, false);
        CHECK(bool_comb_match(neg, 0) && !bool_comb_match(neg, 1) && !bool_comb_match(none, 0) && !bool_comb_match(none, 1));
        CHECK(bool_comb_match(make_bool_comb({}, -1, false), 0));  // no clause at all: match_all
        const BoolComb g = make_bool_comb({{0x6, ESGPU_OCCUR_MUST}, {0x18, ESGPU_OCCUR_SHOULD}, {1, ESGPU_OCCUR_SHOULD}}, 2, true);
        CHECK(g.n_groups == 2 && g.n_must_groups == 1 && bool_comb_match(g, 0x2 | 0x8 | 0x1) && !bool_comb_match(g, 0x8 | 0x1) &&
              !bool_comb_match(g, 0x2 | 0x18));
    }
    std::printf("bool_query_check: %llu docs x leaf sets against brute force, 64 leaves, 128 cuts, zeros, NaN, INT64 edges, "
                "empty terms: ok\n", (unsigned long long)checked);
    return 0;
}
