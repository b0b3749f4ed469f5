// range_check.cpp — a stand-alone exercise of the host code behind the range blocks, meant to be built with
// -fsanitize=address,undefined (make -C elasticsearch_amd/csrc check-range): the buckets of a spec (sorted order, keys,
// refusals), range blocks with stats / max children through the reduce by position (an empty shard, a mismatching
// shard), the shard record written, read back (every truncation of it included) and reduced again, the transport bytes
// and the XContent, keyed and not.  Needs no GPU and links esgpu_results.cpp alone.
#include <cmath>
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
// one instance of the range [(-inf, 10) [5, 20) [20, +inf)] with a stats and a max child per bucket
static std::vector<Block> shard(const std::vector<Row>& rows, bool keyed) {
    const char* keys[] = {"*-10.0", "5.0-20.0", "20.0-*"};
    const double from[] = {-INFINITY, 5.0, 20.0}, to[] = {10.0, 20.0, INFINITY};
    Block r = shell(ESGPU_AGG_RANGE, "r");
    r.keyed = keyed;
    r.n = 1;
    r.doc_count_error.push_back(0);
    r.other_doc_count.push_back(0);
    r.boff = {0, rows.size()};
    r.term_off.push_back(0);
    Block s = shell(ESGPU_AGG_STATS, "s"), m = shell(ESGPU_AGG_MAX, "m");
    for (size_t k = 0; k < rows.size(); ++k) {
        r.key.push_back((int64_t)k);
        r.term_pool += keys[k];
        r.term_off.push_back(r.term_pool.size());
        r.rfrom.push_back(from[k]);
        r.rto.push_back(to[k]);
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
    CHECK(blob.size() > 8 && blob[4] == 7);  // a result with a range block: record version 7
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
}

template <class E, class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const E&) {
        return true;
    }
    return false;
}

int main() {
    // ---- the buckets of a spec: stable sort by (from, to), generated and given keys, refusals ----
    {
        const esgpu_range rs[] = {{nullptr, 100, 500}, {"tail", 100, INFINITY}, {"dup", 100, 500}, {nullptr, -INFINITY, 50},
                                  {nullptr, 0.0, 1e7}, {nullptr, -0.0, 100.5}, {nullptr, 1e7, INFINITY}};
        esgpu_agg_spec sp{};
        sp.type = ESGPU_AGG_RANGE;
        sp.ranges = rs;
        sp.n_ranges = 7;
        const std::vector<esgpu::RangeBucket> b = esgpu::range_buckets(sp);
        const int order[] = {3, 5, 4, 0, 2, 1, 6};
        const char* keys[] = {"*-50.0", "-0.0-100.5", "0.0-1.0E7", "100.0-500.0", "dup", "tail", "1.0E7-*"};
        CHECK(b.size() == 7);
        for (size_t k = 0; k < 7; ++k) CHECK(b[k].src == order[k] && b[k].key == keys[k]);
        sp.value_format = ESGPU_FORMAT_DATE_TIME;
        sp.format = "strict_date_optional_time||epoch_millis";
        const esgpu_range ds[] = {{nullptr, 1441065600000.0, INFINITY}};
        sp.ranges = ds;
        sp.n_ranges = 1;
        CHECK(esgpu::range_buckets(sp)[0].key == "2015-09-01T00:00:00.000Z-*");
        sp.format = "yyyy";
        CHECK(throws<std::domain_error>([&] { esgpu::range_buckets(sp); }));
        sp.value_format = ESGPU_FORMAT_NUMBER;
        CHECK(throws<std::domain_error>([&] { esgpu::range_buckets(sp); }));
        sp.value_format = ESGPU_FORMAT_RAW;
        sp.n_ranges = 0;
        CHECK(throws<std::invalid_argument>([&] { esgpu::range_buckets(sp); }));
        const esgpu_range bad[] = {{nullptr, NAN, 1.0}};
        sp.ranges = bad;
        sp.n_ranges = 1;
        CHECK(throws<std::invalid_argument>([&] { esgpu::range_buckets(sp); }));
        std::vector<esgpu_range> many(65, esgpu_range{nullptr, 0.0, 1.0});
        sp.ranges = many.data();
        sp.n_ranges = 65;
        CHECK(throws<std::domain_error>([&] { esgpu::range_buckets(sp); }));
        sp.n_ranges = 64;
        CHECK(esgpu::range_buckets(sp).size() == 64);
    }
    // ---- reduce by position over three shards, one of them empty; record, transport bytes, XContent ----
    for (const bool keyed : {false, true}) {
        const std::vector<Block> a = shard({{4, 4, 10.5, 1.0, 6.0}, {2, 1, 7.0, 7.0, 7.0}, {0, 0, 0, 0, 0}}, keyed),
                                 e = shard({{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}}, keyed),
                                 b = shard({{1, 1, -3.0, -3.0, -3.0}, {5, 5, 60.25, 5.0, 19.5}, {9, 8, 800.0, 20.0, 300.0}}, keyed);
        const std::vector<Block> red = esgpu::reduce_lists({&a, &e, &b});
        CHECK(red.size() == 1 && red[0].nbuckets() == 3 && red[0].n == 1);
        CHECK(red[0].bcount[0] == 5 && red[0].bcount[1] == 7 && red[0].bcount[2] == 9);
        CHECK(red[0].subs[0].count[0] == 5 && red[0].subs[0].sum[0] == 7.5 && red[0].subs[0].min[0] == -3.0);
        CHECK(red[0].subs[0].sum[1] == 67.25 && red[0].subs[1].max[1] == 19.5 && red[0].subs[1].max[2] == 300.0);
        CHECK(red[0].term(1) == "5.0-20.0" && red[0].rfrom[1] == 5.0 && std::isinf(red[0].rto[2]));
        round_trip(red);
        const std::vector<Block> none = esgpu::reduce_lists({&e, &e});
        const std::string x = esgpu::to_xcontent(none);
        if (keyed)
            CHECK(x.find("{\"r\":{\"buckets\":{\"*-10.0\":{\"to\":10.0,\"to_as_string\":\"10.0\",\"doc_count\":0,\"s\":{\"count\":0,"
                         "\"min\":null,\"max\":null,\"avg\":null,\"sum\":null},\"m\":{\"value\":null}},\"5.0-20.0\":{\"from\":5.0,") == 0);
        else
            CHECK(x.find("{\"r\":{\"buckets\":[{\"key\":\"*-10.0\",\"to\":10.0,\"to_as_string\":\"10.0\",\"doc_count\":0,") == 0);
        round_trip(none);
        std::string wire;
        esgpu::to_es_stream(red, wire);
        // vInt 1, "range", name "r", null metadata, no pipeline aggregators, RAW formatter, keyed, 3 ranges, the first key
        std::string head("\x01\x05range\x01r\xff\x00\x01\x01", 13);
        head.push_back(keyed ? '\x01' : '\x00');
        head += std::string("\x03\x01\x06*-10.0\xff\xf0", 11);
        CHECK(wire.substr(0, head.size()) == head);
    }
    // ---- shards whose range counts differ are rejected ----
    {
        const std::vector<Block> a = shard({{1, 1, 1.0, 1.0, 1.0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}}, false),
                                 b = shard({{1, 1, 1.0, 1.0, 1.0}, {0, 0, 0, 0, 0}}, false);
        CHECK(throws<std::invalid_argument>([&] { esgpu::reduce_lists({&a, &b}); }));
    }
    // ---- like / append_instance keep the bounds ----
    {
        const std::vector<Block> a = shard({{4, 4, 10.5, 1.0, 6.0}, {2, 1, 7.0, 7.0, 7.0}, {0, 0, 0, 0, 0}}, true);
        Block c = a[0].like();
        CHECK(c.n == 0 && c.keyed == 1 && c.subs.size() == 2 && c.nbuckets() == 0);
        c.append_instance(a[0], 0);
        CHECK(c.nbuckets() == 3 && c.rfrom.size() == 3 && c.rto[0] == 10.0 && c.subs[0].n == 3 && c.term(2) == "20.0-*");
        CHECK(esgpu::to_json({c}) == esgpu::to_json(a));
    }
    std::puts("range_check ok");
    return 0;
}
