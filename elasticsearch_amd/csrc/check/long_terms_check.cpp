// long_terms_check.cpp — a stand-alone exercise of the host code behind terms over long fields, meant to be built with
// -fsanitize=address,undefined (make -C elasticsearch_amd/csrc check-long-terms): the numeric dictionary merge of an
// ordinal map, the reduce keyed by long values, the version 5 / version 6 shard-stream reader (every truncation of a
// valid stream included) and the "lterms" transport writer.  Needs no GPU and links esgpu_results.cpp alone.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../esgpu_results.hpp"

using esgpu::Block;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

static Block avg_shell() {
    Block a;
    a.type = ESGPU_AGG_AVG;
    a.name = "rt";
    return a;
}

// a shard-level LongTerms (or, longs == false, StringTerms over the decimal text) with an avg per bucket
static Block terms_block(const std::vector<std::pair<int64_t, int64_t>>& buckets, bool longs, int order, int size, int shard_size) {
    Block t;
    t.type = ESGPU_AGG_TERMS;
    t.name = "st";
    t.order = order;
    t.required_size = size;
    t.shard_size = shard_size;
    t.show_err = 1;
    t.terms_kind = longs ? 1 : 0;
    t.n = 1;
    t.doc_count_error.push_back(0);
    t.other_doc_count.push_back(3);
    t.boff = {0, buckets.size()};
    t.term_off.push_back(0);
    Block a = avg_shell();
    for (size_t i = 0; i < buckets.size(); ++i) {
        t.key.push_back((int64_t)i);
        t.term_pool += std::to_string((long long)buckets[i].first);
        t.term_off.push_back(t.term_pool.size());
        if (longs) t.term_long.push_back(buckets[i].first);
        t.bcount.push_back(buckets[i].second);
        t.berr.push_back(0);
        ++a.n;
        a.count.push_back(buckets[i].second);
        a.sum.push_back(2.5 * (double)buckets[i].second);
        a.min.push_back(0);
        a.max.push_back(0);
        a.sumsq.push_back(0);
    }
    t.subs.push_back(std::move(a));
    return t;
}

int main() {
    // ---- numeric dictionary merge ----
    {
        const std::vector<int64_t> a = {INT64_MIN, -1, 0, 7}, b = {}, c = {-1, 8, INT64_MAX};
        std::vector<int64_t> g;
        std::vector<std::vector<uint32_t>> maps;
        esgpu::merge_long_dicts({&a, nullptr, &b, &c}, g, maps);
        CHECK((g == std::vector<int64_t>{INT64_MIN, -1, 0, 7, 8, INT64_MAX}));
        CHECK((maps[0] == std::vector<uint32_t>{0, 1, 2, 3}) && maps[1].empty() && maps[2].empty());
        CHECK((maps[3] == std::vector<uint32_t>{1, 4, 5}));
    }
    // ---- reduce by long value, numeric tie-break, version 6 round trip ----
    const int orders[] = {ESGPU_ORDER_COUNT_DESC, ESGPU_ORDER_COUNT_ASC, ESGPU_ORDER_TERM_ASC, ESGPU_ORDER_TERM_DESC};
    for (int order : orders) {
        std::vector<Block> s0, s1, s2;
        s0.push_back(terms_block({{10, 5}, {9, 5}, {INT64_MIN, 1}}, true, order, 3, 3));
        s1.push_back(terms_block({{9, 2}, {INT64_MAX, 4}, {-1, 4}}, true, order, 3, 3));
        s2.push_back(terms_block({}, false, order, 3, 3));  // a shard without the field: empty string terms
        const std::vector<Block> red = esgpu::reduce_lists({&s2, &s0, &s1});
        CHECK(red.size() == 1 && red[0].terms_kind == 1 && red[0].nbuckets() == 3 && red[0].term_long.size() == 3);
        if (order == ESGPU_ORDER_COUNT_DESC) CHECK(red[0].term_long[0] == 9 && red[0].bcount[0] == 7 && red[0].term_long[1] == 10);
        if (order == ESGPU_ORDER_TERM_ASC) CHECK(red[0].term_long[0] == INT64_MIN && red[0].term_long[1] == -1);
        if (order == ESGPU_ORDER_TERM_DESC) CHECK(red[0].term_long[0] == INT64_MAX && red[0].term_long[1] == 10);
        std::string blob, again;
        esgpu::serialize(red, blob);
        CHECK(blob.size() > 8 && blob[4] == 6);
        std::vector<Block> back;
        CHECK(esgpu::deserialize((const uint8_t*)blob.data(), blob.size(), back));
        esgpu::serialize(back, again);
        CHECK(again == blob);
        CHECK(esgpu::to_xcontent(back) == esgpu::to_xcontent(red) && esgpu::to_json(back) == esgpu::to_json(red));
        // every truncation is refused without reading past the buffer
        for (size_t n = 0; n < blob.size(); ++n) {
            std::vector<uint8_t> cut(blob.begin(), blob.begin() + n);  // its own allocation: an overread is caught
            std::vector<Block> out;
            bool ok = false;
            try {
                ok = esgpu::deserialize(cut.data(), cut.size(), out);
            } catch (const std::exception&) {
                ok = false;
            }
            CHECK(!ok);
        }
        // the transport bytes: "lterms" ... writeLong(term)
        std::string wire;
        esgpu::to_es_stream(red, wire);
        CHECK(wire.size() > 8 && wire.substr(1, 7) == std::string("\x06lterms", 7));
    }
    // ---- string terms with buckets beside long terms: the reduce fails, in either shard order, at any level ----
    {
        std::vector<Block> ls, ss;
        ls.push_back(terms_block({{10, 5}, {9, 5}}, true, ESGPU_ORDER_COUNT_DESC, 3, 3));
        ss.push_back(terms_block({{10, 1}}, false, ESGPU_ORDER_COUNT_DESC, 3, 3));
        for (int flip = 0; flip < 2; ++flip) {
            bool threw = false;
            try {
                if (flip) esgpu::reduce_lists({&ss, &ls}); else esgpu::reduce_lists({&ls, &ss});
            } catch (const std::invalid_argument&) {
                threw = true;
            }
            CHECK(threw);
        }
    }
    // ---- version 5 stays what it was ----
    {
        std::vector<Block> s;
        s.push_back(terms_block({{3, 1}, {20, 1}}, false, ESGPU_ORDER_COUNT_DESC, 10, 10));
        std::string blob;
        esgpu::serialize(s, blob);
        CHECK(blob[4] == 5);
        std::vector<Block> back;
        CHECK(esgpu::deserialize((const uint8_t*)blob.data(), blob.size(), back));
        CHECK(back[0].terms_kind == 0 && back[0].term_long.empty());
        const std::vector<Block> red = esgpu::reduce_lists({&back});
        CHECK(red[0].term(0) == "20");  // string terms tie on count: "20" < "3" as bytes
        std::string wire;
        esgpu::to_es_stream(red, wire);
        CHECK(wire.substr(1, 7) == std::string("\x06sterms", 7));
    }
    std::puts("long_terms_check ok");
    return 0;
}
