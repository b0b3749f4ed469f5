// filters_check.cpp — a stand-alone exercise of the host code behind the filters aggregation, meant to be built with
// -fsanitize=address,undefined (make -C elasticsearch_amd/csrc check-filters): the clause intervals and the mask tables of
// es_filter_masks.hpp against brute-force clause evaluation on the values themselves (random clause sets over a long, a
// double and a keyword column, the edge keys of each included), the bucket keys of a spec and its refusals, and filters
// blocks with stats / max children through the reduce by position (an empty shard, a mismatching shard), the shard
// record written, read back (every truncation of it included) and reduced again, the transport bytes and the XContent,
// keyed and anonymous.  Needs no GPU and links esgpu_results.cpp alone.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../es_filter_masks.hpp"
#include "../esgpu_results.hpp"

using esgpu::Block;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

template <class E, class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const E&) {
        return true;
    }
    return false;
}

// ---- brute force: a clause on the value itself ---------------------------------------------------------------------------
static bool long_accepts(const esgpu_filter& f, int64_t v) {
    if (f.type == ESGPU_FILTER_TERM) return v == f.term;
    if (f.has_lower && std::isinf(f.lo_d)) {  // an infinite bound is compared as the double it is
        if (!(f.include_lower ? (double)v >= f.lo_d : (double)v > f.lo_d)) return false;
    } else if (f.has_lower && !(f.include_lower ? v >= f.lo_i : v > f.lo_i)) {
        return false;
    }
    if (f.has_upper && std::isinf(f.hi_d)) {
        if (!(f.include_upper ? (double)v <= f.hi_d : (double)v < f.hi_d)) return false;
    } else if (f.has_upper && !(f.include_upper ? v <= f.hi_i : v < f.hi_i)) {
        return false;
    }
    return true;
}
static bool double_accepts(const esgpu_filter& f, double v) {  // IEEE comparisons, as the predicate kernels make them
    if (f.type == ESGPU_FILTER_TERM) return v == (double)f.term;
    if (f.has_lower && !(f.include_lower ? v >= f.lo_d : v > f.lo_d)) return false;
    if (f.has_upper && !(f.include_upper ? v <= f.hi_d : v < f.hi_d)) return false;
    return !(v != v);
}
static bool ord_accepts(const esgpu_filter& f, const std::vector<std::string>& dict, uint32_t ord) {
    if (f.type == ESGPU_FILTER_TERM) return (int64_t)ord == f.term;
    const std::string& t = dict[ord];
    if (f.has_lower) {
        const std::string lo((const char*)f.lo_term, (size_t)f.lo_term_len);
        if (!(f.include_lower ? t >= lo : t > lo)) return false;
    }
    if (f.has_upper) {
        const std::string hi((const char*)f.hi_term, (size_t)f.hi_term_len);
        if (!(f.include_upper ? t <= hi : t < hi)) return false;
    }
    return true;
}

constexpr uint32_t kMissing = 0xFFFFFFFFu;
struct Doc {
    int64_t l; bool has_l;
    double d; bool has_d;
    uint32_t o;
};
struct Clause { int col; int slot; esgpu_filter f; };  // col: 0 long, 1 double, 2 keyword

static void check_tables(std::mt19937_64& rng, int n_filters, int n_clauses, bool many_cuts) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<int64_t> lpool = {INT64_MIN, INT64_MIN + 1, -2, -1, 0, 1, 2, 7, 100, INT64_MAX - 1, INT64_MAX};
    const std::vector<double> dpool = {-inf, -1.7976931348623157e308, -1.5, -1e-300, -4.9e-324, -0.0, 0.0, 4.9e-324, 1e-300, 1.5,
                                       2.5, 1.7976931348623157e308, inf, nan, -nan};
    const std::vector<std::string> dict = {"", "a", "aa", "ab", "b", "b\xff", "c", "zz"};  // sorted by unsigned bytes
    const std::vector<std::string> tpool = {"", "a", "aa", "aaa", "ab", "b", "b\xff", "bz", "c", "d", "zz", "zzz", "\xff"};
    auto pick = [&](size_t n) { return (size_t)(rng() % n); };
    std::vector<Clause> clauses;
    for (int k = 0; k < n_clauses; ++k) {
        Clause c{};
        c.col = (int)pick(3);
        c.slot = (int)pick((size_t)n_filters);
        esgpu_filter& f = c.f;
        f.type = pick(4) == 0 ? ESGPU_FILTER_TERM : ESGPU_FILTER_RANGE;
        f.has_lower = (int32_t)pick(2);
        f.has_upper = (int32_t)pick(2);
        f.include_lower = (int32_t)pick(2);
        f.include_upper = (int32_t)pick(2);
        if (c.col == 0) {
            f.term = many_cuts ? (int64_t)k * 3 : lpool[pick(lpool.size())];
            f.lo_i = many_cuts ? (int64_t)k * 5 : lpool[pick(lpool.size())];
            f.hi_i = many_cuts ? (int64_t)k * 5 + 1000 : lpool[pick(lpool.size())];
            if (!many_cuts && pick(6) == 0) f.lo_d = pick(2) ? inf : -inf;  // (else 0.0: the longs are the bounds)
            if (!many_cuts && pick(6) == 0) f.hi_d = pick(2) ? inf : -inf;
        } else if (c.col == 1) {
            f.term = (int64_t)pick(4) - 1;
            f.lo_d = dpool[pick(dpool.size())];
            f.hi_d = dpool[pick(dpool.size())];
        } else {
            f.term = (int64_t)pick(dict.size() + 2) - 1;  // -1: a term absent from the dictionary; one past the end too
            const std::string& lo = tpool[pick(tpool.size())];
            const std::string& hi = tpool[pick(tpool.size())];
            f.lo_term = (const uint8_t*)lo.data();
            f.lo_term_len = lo.size();
            f.hi_term = (const uint8_t*)hi.data();
            f.hi_term_len = hi.size();
        }
        clauses.push_back(c);
    }
    // the tables, one per column with a clause
    std::vector<uint64_t> table[3];
    uint32_t n_cuts[3] = {0, 0, 0};
    bool used[3] = {false, false, false};
    for (int col = 0; col < 3; ++col) {
        std::vector<FilterClause> fc;
        for (const Clause& c : clauses) {
            if (c.col != col) continue;
            KeyInterval iv;
            if (col == 0) iv = fm_long_interval(c.f);
            else if (col == 1) iv = fm_f64_interval(fm_f64_bounds(c.f));
            else if (c.f.type == ESGPU_FILTER_TERM) iv = {c.f.term, c.f.term};
            else
                iv = fm_ord_range(c.f, dict.size(), [&](const uint8_t* t, uint64_t len, uint64_t ord, bool strict) {
                    const std::string key((const char*)t, (size_t)len);
                    return strict ? dict[ord] < key : !(key < dict[ord]);
                });
            fc.push_back({c.slot, iv});
        }
        if (fc.empty()) continue;
        used[col] = true;
        table[col].assign(kFilterMaskStride, 0xDEADull);
        const KeyInterval domain = col == 0 ? KeyInterval{INT64_MIN, INT64_MAX} : col == 1 ? fm_f64_domain() : kOrdDomain;
        const bool ok = build_filter_masks(fc, n_filters, domain, table[col].data(), &n_cuts[col]);
        if (!ok) {
            CHECK(many_cuts && fc.size() * 2 > kFilterMaskCuts);
            return;
        }
        CHECK(n_cuts[col] <= kFilterMaskCuts);
        for (uint32_t k = 1; k < n_cuts[col]; ++k) CHECK((int64_t)table[col][k - 1] < (int64_t)table[col][k]);
    }
    const uint64_t all = n_filters >= 64 ? ~0ull : (1ull << n_filters) - 1ull;
    // every combination would be 11 * 15 * 9 docs with and without values: sample
    for (int it = 0; it < 400; ++it) {
        Doc d;
        d.l = many_cuts ? (int64_t)(rng() % 2000) - 10 : lpool[pick(lpool.size())];
        d.has_l = pick(5) != 0;
        d.d = dpool[pick(dpool.size())];
        d.has_d = pick(5) != 0;
        d.o = pick(5) == 0 ? kMissing : (uint32_t)pick(dict.size());
        uint64_t want = all;
        for (const Clause& c : clauses) {
            bool ok;
            if (c.col == 0) ok = d.has_l && long_accepts(c.f, d.l);
            else if (c.col == 1) ok = d.has_d && double_accepts(c.f, d.d);
            else ok = d.o != kMissing && ord_accepts(c.f, dict, d.o);
            if (!ok) want &= ~(1ull << c.slot);
        }
        uint64_t got = all;
        if (used[0]) got &= d.has_l ? filter_mask_lookup(table[0].data(), n_cuts[0], d.l) : table[0][kFilterMaskNoValue];
        if (used[1])
            got &= d.has_d && !(d.d != d.d) ? filter_mask_lookup(table[1].data(), n_cuts[1], fm_f64_key(d.d)) : table[1][kFilterMaskNoValue];
        if (used[2]) got &= d.o != kMissing ? filter_mask_lookup(table[2].data(), n_cuts[2], (int64_t)d.o) : table[2][kFilterMaskNoValue];
        if (got != want) {
            std::fprintf(stderr, "doc l=%lld(%d) d=%g(%d) o=%u: got %llx want %llx\n", (long long)d.l, d.has_l, d.d, d.has_d, d.o,
                         (unsigned long long)got, (unsigned long long)want);
            std::exit(1);
        }
    }
}

// ---- blocks --------------------------------------------------------------------------------------------------------------
static Block shell(int type, const char* name) {
    Block a;
    a.type = type;
    a.name = name;
    return a;
}

static void push_metric(Block& a, int64_t count, double sum, double mn, double mx) {
    ++a.n;
    a.count.push_back(count);
    a.sum.push_back(sum);
    a.min.push_back(count ? mn : INFINITY);
    a.max.push_back(count ? mx : -INFINITY);
    a.sumsq.push_back(0.0);
}

struct Row { int64_t docs, count; double sum, mn, mx; };
// one instance of the filters [fast, slow, _other_] (anonymous: 0, 1, 2) with a stats and a max child per bucket
static std::vector<Block> shard(const std::vector<Row>& rows, bool keyed) {
    const char* named[] = {"fast", "slow", "_other_"};
    const char* anon[] = {"0", "1", "2"};
    Block r = shell(ESGPU_AGG_FILTERS, "f");
    r.keyed = keyed;
    r.n = 1;
    r.doc_count_error.push_back(0);
    r.other_doc_count.push_back(0);
    r.boff = {0, rows.size()};
    r.term_off.push_back(0);
    Block s = shell(ESGPU_AGG_STATS, "s"), m = shell(ESGPU_AGG_MAX, "m");
    for (size_t k = 0; k < rows.size(); ++k) {
        r.key.push_back((int64_t)k);
        r.term_pool += keyed ? named[k] : anon[k];
        r.term_off.push_back(r.term_pool.size());
        r.bcount.push_back(rows[k].docs);
        r.berr.push_back(0);
        push_metric(s, rows[k].count, rows[k].sum, rows[k].mn, rows[k].mx);
        push_metric(m, 0, 0.0, 0.0, 0.0);
        m.max.back() = rows[k].count ? rows[k].mx : -INFINITY;
    }
    r.subs.push_back(std::move(s));
    r.subs.push_back(std::move(m));
    std::vector<Block> l;
    l.push_back(std::move(r));
    return l;
}

static void round_trip(const std::vector<Block>& red) {
    std::string blob, again;
    esgpu::serialize(red, blob);
    CHECK(blob.size() > 8 && blob[4] == 8);  // a result with a filters block: record version 8
    std::vector<Block> back;
    CHECK(esgpu::deserialize((const uint8_t*)blob.data(), blob.size(), back));
    esgpu::serialize(back, again);
    CHECK(again == blob);
    CHECK(esgpu::to_xcontent(back) == esgpu::to_xcontent(red) && esgpu::to_json(back) == esgpu::to_json(red));
    std::string w0, w1;
    esgpu::to_es_stream(red, w0);
    esgpu::to_es_stream(back, w1);
    CHECK(w0 == w1 && !w0.empty());
    for (size_t n = 0; n < blob.size(); ++n) {  // every truncation is refused without reading past the buffer
        std::vector<uint8_t> cut(blob.begin(), blob.begin() + n);
        std::vector<Block> out;
        bool ok = false;
        try {
            ok = esgpu::deserialize(cut.data(), cut.size(), out);
        } catch (const std::exception&) {
            ok = false;
        }
        CHECK(!ok);
    }
    for (const char v : {(char)4, (char)9}) {  // versions outside 5 .. 8 are refused
        std::string other = blob;
        other[4] = v;
        std::vector<Block> out;
        CHECK(!esgpu::deserialize((const uint8_t*)other.data(), other.size(), out));
    }
}

int main() {
    // ---- clause intervals at the edges ----
    {
        esgpu_filter f{};
        f.type = ESGPU_FILTER_RANGE;
        f.has_lower = 1;
        f.lo_i = INT64_MAX;
        CHECK(fm_long_interval(f).empty());                                   // gt(INT64_MAX)
        f.include_lower = 1;
        CHECK(fm_long_interval(f).lo == INT64_MAX && fm_long_interval(f).hi == INT64_MAX);
        f = esgpu_filter{};
        f.type = ESGPU_FILTER_RANGE;
        f.has_upper = 1;
        f.hi_i = INT64_MIN;
        CHECK(fm_long_interval(f).empty());                                   // lt(INT64_MIN)
        f.hi_i = INT64_MAX;
        f.hi_d = INFINITY;                                                    // lt(+Infinity): every long
        CHECK(fm_long_interval(f).lo == INT64_MIN && fm_long_interval(f).hi == INT64_MAX);
        f.hi_d = -INFINITY;
        f.include_upper = 1;                                                  // lte(-Infinity): none
        CHECK(fm_long_interval(f).empty());
        f = esgpu_filter{};
        f.type = ESGPU_FILTER_RANGE;
        f.has_lower = f.include_lower = 1;
        f.lo_i = INT64_MAX;
        f.lo_d = INFINITY;                                                    // gte(+Infinity): none, INT64_MAX included
        CHECK(fm_long_interval(f).empty());
        f.lo_d = -INFINITY;
        f.include_lower = 0;                                                  // gt(-Infinity): every long
        CHECK(fm_long_interval(f).lo == INT64_MIN && fm_long_interval(f).hi == INT64_MAX);
        CHECK(fm_f64_key(-0.0) == -1 && fm_f64_key(0.0) == 0 && fm_f64_key(-4.9e-324) == -2 && fm_f64_key(4.9e-324) == 1);
        for (const double z : {0.0, -0.0}) {                                  // both zeros under every bound kind
            CHECK(fm_f64_interval({z, INFINITY, 1, 1}).lo == -1 && fm_f64_interval({z, INFINITY, 0, 1}).lo == 1);
            CHECK(fm_f64_interval({-INFINITY, z, 1, 1}).hi == 0 && fm_f64_interval({-INFINITY, z, 1, 0}).hi == -2);
        }
        CHECK(fm_f64_interval({NAN, 1.0, 1, 1}).empty() && fm_f64_interval({0.0, NAN, 1, 1}).empty());
        CHECK(fm_f64_interval({INFINITY, INFINITY, 0, 1}).empty() && !fm_f64_interval({INFINITY, INFINITY, 1, 1}).empty());
        CHECK(fm_f64_interval({-INFINITY, -INFINITY, 1, 0}).empty() && !fm_f64_interval({-INFINITY, INFINITY, 0, 0}).empty());
    }
    // ---- the tables against brute force ----
    {
        std::mt19937_64 rng(0x5EED);
        for (int it = 0; it < 1500; ++it) {
            const int nf = it % 7 == 0 ? 64 : 1 + (int)(rng() % 64);
            check_tables(rng, nf, (int)(rng() % 12), false);
        }
        for (int it = 0; it < 20; ++it) check_tables(rng, 64, 40 + 20 * it, true);  // up to and past the cut limit
        // no clause at all on a column: never built; a column with only empty clauses has no cut
        uint64_t t[kFilterMaskStride];
        uint32_t n = 99;
        CHECK(build_filter_masks({{3, {1, 0}}}, 5, {INT64_MIN, INT64_MAX}, t, &n));
        CHECK(n == 0 && t[kFilterMaskCuts] == 0x17 && t[kFilterMaskNoValue] == 0x17);
        // two clauses of one filter on one column intersect
        CHECK(build_filter_masks({{0, {0, 10}}, {0, {5, 20}}, {1, {0, 3}}, {1, {4, 9}}}, 2, {INT64_MIN, INT64_MAX}, t, &n));
        CHECK(filter_mask_lookup(t, n, 4) == 0 && filter_mask_lookup(t, n, 5) == 1 && filter_mask_lookup(t, n, 10) == 1 &&
              filter_mask_lookup(t, n, 11) == 0 && filter_mask_lookup(t, n, 2) == 0 && t[kFilterMaskNoValue] == 0);
    }
    // ---- the bucket keys of a spec and its refusals ----
    {
        const char* keys[] = {"a", "b"};
        esgpu_agg_spec sp{};
        sp.type = ESGPU_AGG_FILTERS;
        sp.filter_keys = keys;
        sp.n_filters = 2;
        sp.keyed = 1;
        CHECK((esgpu::filters_bucket_keys(sp) == std::vector<std::string>{"a", "b"}));
        sp.other_bucket = 1;
        CHECK((esgpu::filters_bucket_keys(sp) == std::vector<std::string>{"a", "b", "_other_"}));
        sp.other_bucket_key = "rest";
        sp.keyed = 0;
        sp.filter_keys = nullptr;
        CHECK((esgpu::filters_bucket_keys(sp) == std::vector<std::string>{"0", "1", "rest"}));
        sp.keyed = 1;
        CHECK(throws<std::invalid_argument>([&] { esgpu::filters_bucket_keys(sp); }));
        sp.keyed = 0;
        sp.n_filters = 0;
        CHECK(throws<std::invalid_argument>([&] { esgpu::filters_bucket_keys(sp); }));
        sp.n_filters = 64;
        CHECK(throws<std::domain_error>([&] { esgpu::filters_bucket_keys(sp); }));
        sp.other_bucket = 0;
        CHECK(esgpu::filters_bucket_keys(sp).size() == 64 && esgpu::filters_bucket_keys(sp)[63] == "63");
        sp.n_filters = 65;
        CHECK(throws<std::domain_error>([&] { esgpu::filters_bucket_keys(sp); }));
    }
    // ---- reduce by position over three shards, one of them empty; record, transport bytes, XContent ----
    for (const bool keyed : {false, true}) {
        const std::vector<Block> a = shard({{4, 4, 10.5, 1.0, 6.0}, {2, 1, 7.0, 7.0, 7.0}, {0, 0, 0, 0, 0}}, keyed),
                                 e = shard({{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}}, keyed),
                                 b = shard({{1, 1, -3.0, -3.0, -3.0}, {5, 5, 60.25, 5.0, 19.5}, {9, 8, 800.0, 20.0, 300.0}}, keyed);
        const std::vector<Block> red = esgpu::reduce_lists({&a, &e, &b});
        CHECK(red.size() == 1 && red[0].nbuckets() == 3 && red[0].n == 1 && red[0].is_filters());
        CHECK(red[0].bcount[0] == 5 && red[0].bcount[1] == 7 && red[0].bcount[2] == 9);
        CHECK(red[0].subs[0].count[0] == 5 && red[0].subs[0].sum[0] == 7.5 && red[0].subs[0].min[0] == -3.0);
        CHECK(red[0].subs[0].sum[1] == 67.25 && red[0].subs[1].max[1] == 19.5 && red[0].subs[1].max[2] == 300.0);
        CHECK(red[0].term(1) == (keyed ? "slow" : "1") && red[0].rfrom.empty() && red[0].rto.empty());
        round_trip(red);
        const std::vector<Block> none = esgpu::reduce_lists({&e, &e});
        const std::string x = esgpu::to_xcontent(none);
        if (keyed)
            CHECK(x == "{\"f\":{\"buckets\":{\"fast\":{\"doc_count\":0,\"s\":{\"count\":0,\"min\":null,\"max\":null,\"avg\":null,"
                       "\"sum\":null},\"m\":{\"value\":null}},\"slow\":{\"doc_count\":0,\"s\":{\"count\":0,\"min\":null,\"max\":null,"
                       "\"avg\":null,\"sum\":null},\"m\":{\"value\":null}},\"_other_\":{\"doc_count\":0,\"s\":{\"count\":0,\"min\":null,"
                       "\"max\":null,\"avg\":null,\"sum\":null},\"m\":{\"value\":null}}}}}");
        else
            CHECK(x.find("{\"f\":{\"buckets\":[{\"doc_count\":0,\"s\":{\"count\":0,") == 0);
        round_trip(none);
        std::string wire;
        esgpu::to_es_stream(red, wire);
        // vInt 1, "filters", name "f", null metadata, no pipeline aggregators, keyed, 3 buckets, the first key, vLong 5
        std::string head("\x01\x07" "filters\x01" "f\xff\x00", 13);
        head.push_back(keyed ? '\x01' : '\x00');
        head += keyed ? std::string("\x03\x01\x04" "fast\x05", 8) : std::string("\x03\x01\x01" "0\x05", 5);
        CHECK(wire.substr(0, head.size()) == head);
    }
    // ---- shards whose bucket counts differ are rejected ----
    {
        const std::vector<Block> a = shard({{1, 1, 1.0, 1.0, 1.0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}}, true),
                                 b = shard({{1, 1, 1.0, 1.0, 1.0}, {0, 0, 0, 0, 0}}, true);
        CHECK(throws<std::invalid_argument>([&] { esgpu::reduce_lists({&a, &b}); }));
    }
    // ---- like / append_instance / append_empty ----
    {
        const std::vector<Block> a = shard({{4, 4, 10.5, 1.0, 6.0}, {2, 1, 7.0, 7.0, 7.0}, {0, 0, 0, 0, 0}}, true);
        Block c = a[0].like();
        CHECK(c.n == 0 && c.keyed == 1 && c.subs.size() == 2 && c.nbuckets() == 0);
        c.append_instance(a[0], 0);
        CHECK(c.nbuckets() == 3 && c.rfrom.empty() && c.subs[0].n == 3 && c.term(2) == "_other_");
        CHECK(esgpu::to_json({c}) == esgpu::to_json(a));
    }
    std::puts("filters_check ok");
    return 0;
}
