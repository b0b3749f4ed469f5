"""The reference's own expected values, asserted on results the GPU collected (VERDICT "What's missing" #3).

tests/golden/kat.json and tests/golden/long_terms.json hold the documents and the literal expected values of the
reference's own tests (extracted by tests/golden/make_golden.py; each entry cites file:line).  tests/test_oracle_kat.py
and tests/test_long_terms_host.py hold the oracle and the host reduce to them; here every fixture goes through
engine.upload_segment -> plan.collect -> build -> reduce, on the default layouts and at upload width.  The fixtures hold
2-20 docs per segment and integer data only, so counts, keys and metric doubles are all compared with ==.
"""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest

import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Order, QueryBuilders as QB
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from test_gpu_layouts import layout

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_terms.json")) as _f:
    LONG_TERMS = json.load(_f)

LAYOUT = pytest.mark.parametrize("name", ["default", "upload"])


def _layout(engine, name):
    return contextlib.nullcontext() if name == "default" else layout(engine, name)


def _i64(vals):
    return {"type": N.COL_I64, "values": np.array(vals, dtype=np.int64)}


def _multi_i64(lists):
    offs = np.zeros(len(lists) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in lists])
    return {"type": N.COL_I64, "values": np.array([v for x in lists for v in sorted(x)], dtype=np.int64), "offsets": offs}


def _terms_col(keys):
    terms = sorted(set(keys))
    return {"type": N.COL_ORD_U32, "values": np.array([terms.index(k) for k in keys], dtype=np.uint32), "terms": terms}


def gpu_reduced(engine, name, shards, aggs, **plan_kw):
    """[(columns, max_doc)] -- one segment per shard -- uploaded, collected, built and reduced: the reduced result tree"""
    results = []
    with _layout(engine, name):
        for cols, n in shards:
            seg = engine.upload_segment(cols, n)
            plan = engine.plan(aggs, number_of_shards=len(shards), **plan_kw)
            try:
                plan.collect(seg)
                results.append(plan.build())
            finally:
                plan.close()
                seg.close()
    return reduce(results).to_dict()


@LAYOUT
def test_extended_stats_1_to_10(engine, kat, name):  # ExtendedStatsTests.testSingleValuedField / testMultiValuedField
    st = kat["stats"]
    cols = {"value": _i64(st["docs"]["value"]), "values": _multi_i64(st["docs"]["values"])}
    res = gpu_reduced(engine, name, [(cols, 10)], [AB.extendedStats("s1").field("value"), AB.extendedStats("s2").field("values")])
    for agg, exp in (("s1", st["single"]), ("s2", st["multi"])):
        for k in ("count", "sum", "min", "max", "avg", "sum_of_squares", "variance"):
            assert res[agg][k] == exp[k], (agg, k, st["cite_expect"])


@LAYOUT
def test_empty_bucket_extended_stats(engine, kat, name):  # ExtendedStatsTests.testEmptyAggregation: bucket 1 is empty
    cols = {"value": _i64(kat["stats"]["empty_bucket_docs"])}
    agg = AB.histogram("histo").field("value").interval(1).minDocCount(0).subAggregation(AB.extendedStats("stats").field("value"))
    b = gpu_reduced(engine, name, [(cols, 2)], [agg])["histo"]["buckets"]
    assert [x["key"] for x in b] == [0, 1, 2] and [x["doc_count"] for x in b] == [1, 0, 1]
    s = b[1]["stats"]
    assert s["count"] == 0 and s["_internal"]["min"] == float("inf") and s["_internal"]["max"] == float("-inf")
    assert s["avg"] is None


@LAYOUT
def test_shard_size_terms(engine, kat, name):  # ShardSizeTermsIT.noShardSize_string / shardSizeEqualsSize_string
    fx = kat["shard_size_terms"]
    shards = []
    for counts in fx["shards"]:
        keys = [k for k, n in sorted(counts.items()) for _ in range(n)]
        shards.append(({"key": _terms_col(keys)}, len(keys)))
    for case in fx["cases"]:
        b = AB.terms("keys").field("key").size(case["size"]).order(Order.count(False))
        if case["shard_size"] is not None:
            b.shardSize(case["shard_size"])
        res = gpu_reduced(engine, name, shards, [b])["keys"]
        assert {x["key"]: x["doc_count"] for x in res["buckets"]} == case["expect"], case["cite"]


@LAYOUT
def test_histogram_rest_fixture(engine, kat, name):  # 10_histogram.yaml
    h = kat["rest"]["histogram"]
    b = gpu_reduced(engine, name, [({"number": _i64(h["numbers"])}, 4)],
                    [AB.histogram("histo").field("number").interval(h["interval"])])["histo"]["buckets"]
    assert [x["key"] for x in b] == h["keys"] and [x["doc_count"] for x in b] == h["doc_counts"], h["cite"]


@LAYOUT
def test_murmur3_cardinality_rest_fixture(engine, kat, name):  # mapper_murmur3/10_basic.yaml: cardinality on foo.hash
    L = O.lib()
    fx = kat["rest"]["murmur3_cardinality"]
    hashes = []
    for s in fx["foo"]:
        b = s.encode()
        h1, h2 = ctypes.c_uint64(), ctypes.c_uint64()
        L.oracle_murmur3_128(b, len(b), 0, ctypes.byref(h1), ctypes.byref(h2))
        hashes.append(h1.value)
    agg = [AB.cardinality("foo_count").field("foo.hash")]
    # a 1-doc segment whose field is absent (the yaml's first search: nothing indexed under foo yet)
    empty = gpu_reduced(engine, name, [({"other": _i64([7])}, 1)], agg)
    assert empty["foo_count"]["value"] == fx["empty_value"], fx["cite"]
    cols = {"foo.hash": {"type": N.COL_U64, "values": np.array(hashes, dtype=np.uint64)}}
    assert gpu_reduced(engine, name, [(cols, len(hashes))], agg)["foo_count"]["value"] == fx["value"], fx["cite"]


@LAYOUT
def test_date_histogram_fixture(engine, kat, name):  # DateHistogramTests.singleValuedField / _WithTimeZone / multiValuedField
    fx = kat["date_histogram"]
    shard = [({"date": _i64(fx["date"]), "dates": _multi_i64(fx["dates"])}, 6)]
    for field, exp in (("date", fx["monthly"]), ("dates", fx["monthly_multi"])):
        b = gpu_reduced(engine, name, shard, [AB.dateHistogram("histo").field(field).interval("month")])["histo"]["buckets"]
        assert [x["key"] for x in b] == exp["keys"] and [x["doc_count"] for x in b] == exp["doc_counts"], exp["cite"]
    tz = fx["daily_tz_plus1"]
    b = gpu_reduced(engine, name, shard, [AB.dateHistogram("histo").field("date").interval("day").minDocCount(1).timeZone("+01:00")])
    b = b["histo"]["buckets"]
    assert [x["key"] for x in b] == tz["keys"] and [x["doc_count"] for x in b] == tz["doc_counts"], tz["cite"]
    # the multi-valued field under the same daily rounding: each doc's two dates are a month and a day apart -- twelve
    # distinct days, one doc each, the single-valued keys among them
    b = gpu_reduced(engine, name, shard, [AB.dateHistogram("histo").field("dates").interval("day").minDocCount(1).timeZone("+01:00")])
    b = b["histo"]["buckets"]
    assert len(b) == 12 and all(x["doc_count"] == 1 for x in b) and set(tz["keys"]) <= {x["key"] for x in b}, tz["cite"]


@LAYOUT
@pytest.mark.parametrize("num_docs,num_tag1", [(5, 1), (12, 7), (20, 19)])
def test_filter_aggregation_fixture(engine, name, num_docs, num_tag1):  # FilterIT.simple / withSubAggregation (:95-146)
    """FilterIT's index: docs 0..numTag1Docs-1 {value: i+1, tag: tag1}, the rest {value: i, tag: tag2}.
    filter(termQuery(tag, tag1)) has doc_count numTag1Docs and avg(value) = sum(1..numTag1Docs) / numTag1Docs."""
    tags = ["tag1" if i < num_tag1 else "tag2" for i in range(num_docs)]
    vals = [i + 1 if i < num_tag1 else i for i in range(num_docs)]
    cols = {"tag": _terms_col(tags), "value": _i64(vals)}
    lookup = {"tag1": 0, "tag2": 1}
    aggs = [AB.filter("tag1", QB.termQuery("tag", "tag1")).subAggregation(AB.avg("avg_value").field("value")),
            AB.filter("plain", QB.termQuery("tag", "tag1"))]
    res = gpu_reduced(engine, name, [(cols, num_docs)], aggs, ord_lookup=lambda f, t: lookup.get(t, -1))
    assert res["tag1"]["doc_count"] == num_tag1 and res["plain"]["doc_count"] == num_tag1
    assert res["tag1"]["avg_value"]["value"] == sum(range(1, num_tag1 + 1)) / num_tag1
    assert list(res["plain"].keys()) == ["doc_count"]


@LAYOUT
def test_long_terms_five_docs(engine, name):  # LongTermsTests.java:79-101, :277-278
    g = LONG_TERMS["five_docs"]
    res = gpu_reduced(engine, name, [({"l_value": _i64(g["values"])}, len(g["values"]))], [AB.terms("terms").field("l_value")])
    assert [[b["key"], b["doc_count"]] for b in res["terms"]["buckets"]] == g["expected"], g["_cite"]


@LAYOUT
def test_long_terms_multi_sort(engine, name):  # LongTermsTests.java:125-230, :1204-1241
    """the sort_idx documents split into two shards as tests/test_long_terms_host.py does; terms(l_value) ordered by
    avg_l with an avg(l) child, collected on the GPU: the expected key order, and each bucket's count and average"""
    g = LONG_TERMS["multi_sort"]
    docs = g["docs"]
    shards = [({"l_value": _i64([d[0] for d in part]), "l": _i64([d[1] for d in part]), "d": _i64([d[2] for d in part])}, len(part))
              for part in (docs[0::2], docs[1::2])]
    for case in g["orders"]:
        asc = case["order"].startswith("avg_l asc")
        agg = AB.terms("terms").field("l_value").size(10).order(Order.aggregation("avg_l", asc)).subAggregation(AB.avg("avg_l").field("l"))
        got = gpu_reduced(engine, name, shards, [agg])["terms"]["buckets"]
        assert [b["key"] for b in got] == case["expected_keys"], case["order"]
        for b in got:
            want = g["buckets"][str(b["key"])]
            assert b["doc_count"] == want["count"] and b["avg_l"]["value"] == want["avg_l"], (case["order"], b["key"])
