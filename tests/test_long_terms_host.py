"""LongTerms on the host side, without a GPU: hand-built shard results in the version-6 shard stream
(tests/long_terms_stream.py) go through esgpu_result_deserialize -> esgpu_reduce -> JSON / XContent / transport bytes.

  * the reduce groups buckets by their long key and orders ties by Long.compare (LongTerms.java:86-88), not by the
    decimal text ("10" sorts before "9" as bytes);
  * the ordering cases of LongTermsTests.java (documents and expected bucket orders in tests/golden/long_terms.json);
  * a version-5 blob still deserialises, results without LongTerms are still written as version 5, and the ABI version
    stays 7.
"""
import json
import os
import struct

import pytest

import long_terms_stream as LT
import result_stream as RS
from elasticsearch_amd import ShardResult, reduce
from elasticsearch_amd import _native as N

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_terms.json")) as _f:
    GOLDEN = json.load(_f)


def _shard(name, pairs, size, shard_size, order, min_doc_count=1, show_err=0, total=None):
    """the shard-level LongTerms of (key, count) pairs under the restated selection rule"""
    keys, counts = [k for k, _ in pairs], [c for _, c in pairs]
    kept, other = LT.top_k(keys, counts, shard_size, order)
    return LT.long_terms(name, kept, size=size, shard_size=shard_size, order=order, min_doc_count=min_doc_count,
                         other=other, show_err=show_err), (kept, other)


SHARDS = [
    [(-5, 7), (9, 7), (10, 7), (100, 3), (1 << 40, 2), (-(1 << 63), 1)],
    [(9, 4), (10, 4), (11, 9), (-5, 1), ((1 << 63) - 1, 5)],
    [(10, 2), (100, 6), (7, 6), (-1, 6), (0, 1)],
]


@pytest.mark.parametrize("order", [N.ORDER_COUNT_DESC, N.ORDER_COUNT_ASC, N.ORDER_TERM_ASC, N.ORDER_TERM_DESC])
@pytest.mark.parametrize("size, shard_size", [(3, 4), (20, 20)])
def test_reduce_matches_the_restated_rule(order, size, shard_size):
    built = [_shard("t", s, size, shard_size, order, show_err=1) for s in SHARDS]
    results = [ShardResult.deserialize(LT.encode6([a])) for a, _ in built]
    want, err, other = LT.reduce_terms([x for _, x in built], size, shard_size, order)
    red = reduce(results)
    got = red.to_dict()["t"]
    assert [(b["key"], b["doc_count"], b["doc_count_error_upper_bound"]) for b in got["buckets"]] == want
    assert (got["doc_count_error_upper_bound"], got["sum_other_doc_count"]) == (err, other)
    # the reduced result survives its own serialisation (version 6) and renders alike
    again = ShardResult.deserialize(red.serialize())
    assert again.to_json() == red.to_json() and again.to_xcontent() == red.to_xcontent()
    assert struct.unpack_from("<II", red.serialize()) == (RS.MAGIC, 6)
    # transport bytes: "lterms", long keys
    dec = LT.decode(red.to_stream())[0]
    assert dec["stream_type"] == "lterms" and dec["formatter"] == ("raw",)
    assert [(b["key"], b["doc_count"], b["doc_count_error"]) for b in dec["buckets"]] == want
    assert (dec["doc_count_error"], dec["other_doc_count"]) == (err, other)


def test_numeric_tie_break_not_bytes():
    """9 and 10 tie on count: Long.compare puts 9 first, the bytes "10" < "9" would not"""
    a = LT.long_terms("t", [(10, 5), (9, 5)], order=N.ORDER_COUNT_DESC)
    got = reduce([ShardResult.deserialize(LT.encode6([a]))]).to_dict()["t"]["buckets"]
    assert [b["key"] for b in got] == [9, 10]


def test_long_terms_tests_ordering_cases():
    g = GOLDEN["multi_sort"]
    docs = g["docs"]
    halves = [docs[0::2], docs[1::2]]  # two shards
    shards = []
    for part in halves:
        keys = sorted({d[0] for d in part})
        rows = [(k, [d for d in part if d[0] == k]) for k in keys]
        shards.append(rows)
    for case in g["orders"]:
        asc = case["order"].startswith("avg_l asc")
        order = N.ORDER_AGG_ASC if asc else N.ORDER_AGG_DESC
        results = []
        for rows in shards:
            subs = [[LT.avg("avg_l", len(ds), sum(d[1] for d in ds))] for _, ds in rows]
            a = LT.long_terms("terms", [(k, len(ds)) for k, ds in rows], size=10, shard_size=10, order=order,
                              order_path="avg_l", subs=subs)
            results.append(ShardResult.deserialize(LT.encode6([a])))
        got = reduce(results).to_dict()["terms"]["buckets"]
        assert [b["key"] for b in got] == case["expected_keys"], case["order"]
        for b in got:
            want = g["buckets"][str(b["key"])]
            assert b["doc_count"] == want["count"] and b["avg_l"]["value"] == want["avg_l"]


def test_five_doc_single_valued_case():
    g = GOLDEN["five_docs"]
    a = LT.long_terms("terms", [(v, 1) for v in g["values"]])
    r = reduce([ShardResult.deserialize(LT.encode6([a]))])
    assert [[b["key"], b["doc_count"]] for b in r.to_dict()["terms"]["buckets"]] == g["expected"]
    assert r.to_xcontent() == ('{"terms":{"doc_count_error_upper_bound":0,"sum_other_doc_count":0,"buckets":['
                               + ",".join('{"key":%d,"doc_count":1}' % v for v in g["values"]) + "]}}")


def test_key_as_string_on_a_date_field():
    a = LT.long_terms("t", [(1441065600000, 2), (0, 1)], value_format=N.FORMAT_DATE_TIME,
                      fmt="strict_date_optional_time||epoch_millis")
    r = ShardResult.deserialize(LT.encode6([a]))
    assert r.to_xcontent() == ('{"t":{"doc_count_error_upper_bound":0,"sum_other_doc_count":0,"buckets":['
                               '{"key":1441065600000,"key_as_string":"2015-09-01T00:00:00.000Z","doc_count":2},'
                               '{"key":0,"key_as_string":"1970-01-01T00:00:00.000Z","doc_count":1}]}}')
    dec = LT.decode(r.to_stream())[0]
    assert dec["formatter"] == ("date_time", "strict_date_optional_time||epoch_millis", "UTC")


def test_stream_bytes_of_a_hand_built_block():
    """LongTerms.doWriteTo (:214-227) and Bucket.writeTo (:129-136) field by field"""
    a = LT.long_terms("st", [(200, 3), (-404, 1)], size=10, shard_size=10, show_err=1,
                      subs=[[LT.avg("rt", 3, 30.0)], [LT.avg("rt", 1, 7.5)]])
    got = ShardResult.deserialize(LT.encode6([a])).to_stream()
    want = LT.w_vint(1) + LT.w_header("lterms", "st")
    want += struct.pack(">q", 0)                                     # docCountError
    want += b"\xff" + LT.w_vint(2) + b"\x01" + b"\x04"                # CompoundOrder(_count desc, _term asc)
    want += b"\x01\x01"                                              # optional formatter: present, RAW
    want += LT.w_vint(10) + LT.w_vint(10) + b"\x01" + LT.w_vlong(1) + LT.w_vlong(0) + LT.w_vint(2)
    for key, count, n, total in ((200, 3, 3, 30.0), (-404, 1, 1, 7.5)):
        want += struct.pack(">q", key) + LT.w_vlong(count) + struct.pack(">q", 0)
        want += LT.w_vint(1) + LT.w_header("avg", "rt") + b"\x01\x01" + struct.pack(">d", total) + LT.w_vlong(n)
    assert got == want


def test_unmapped_shard_reduces_into_long_terms():
    """a shard whose segments lack the field builds empty string terms: the reduce still yields LongTerms"""
    empty = RS.string_terms("t", [])
    full = LT.long_terms("t", [(10, 2), (9, 2)])
    results = [ShardResult.deserialize(RS.encode([empty])), ShardResult.deserialize(LT.encode6([full]))]
    got = reduce(results).to_dict()["t"]["buckets"]
    assert [(b["key"], b["doc_count"]) for b in got] == [(9, 2), (10, 2)]


@pytest.mark.parametrize("long_first", [True, False])
def test_string_terms_with_buckets_beside_long_terms_fail_the_reduce(long_first):
    """a field mapped as keyword on one shard and as long on another (or an old result): an error, not a crash"""
    strings = ShardResult.deserialize(RS.encode([RS.string_terms("t", [("10", 1)])]))
    longs = ShardResult.deserialize(LT.encode6([LT.long_terms("t", [(10, 2), (9, 2)])]))
    with pytest.raises(N.EsGpuError) as e:
        reduce([longs, strings] if long_first else [strings, longs])
    assert "differ across shards" in str(e.value)


def test_long_terms_fields_on_a_metric_block_are_refused():
    assert ShardResult.deserialize(LT.encode6([LT.avg("a", 1, 2.0)])).to_dict()["a"]["value"] == 2.0
    with pytest.raises(Exception):
        ShardResult.deserialize(LT.encode6([dict(LT.avg("a", 1, 2.0), terms_kind=1)]))


def test_version_5_still_reads_and_writes():
    blob = RS.encode([RS.string_terms("hosts", [("a", 3), ("b", 1)])])
    r = ShardResult.deserialize(blob)
    assert [b["key"] for b in r.to_dict()["hosts"]["buckets"]] == ["a", "b"]
    assert struct.unpack_from("<II", r.serialize()) == (RS.MAGIC, 5)  # no LongTerms inside: version 5 as before
    assert r.serialize() == blob


def test_truncated_long_terms_block_is_refused():
    blob = LT.encode6([LT.long_terms("t", [(1, 1), (2, 1)])])
    assert len(ShardResult.deserialize(blob).to_dict()["t"]["buckets"]) == 2
    with pytest.raises(Exception):
        ShardResult.deserialize(blob[:-60])


def test_abi_version_stays_7():
    assert N.lib().esgpu_abi_version() == 7
