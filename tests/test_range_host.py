"""The range aggregation on the CPU: builder lowering, esgpu_range_buckets (sorted order and keys), transport bytes and
XContent of hand-built blocks, their reduce (in process, through the shard record, across two gloo ranks), the record
versions and the plan-create refusals.

Hand-derived bytes follow InternalAggregation.writeTo (A/InternalAggregation.java:212-221), InternalRange.doWriteTo
(A/bucket/range/InternalRange.java:323-337), ValueFormatterStreams.writeOptional and StreamOutput's encodings; the
XContent strings InternalRange.doXContentBody (:339-355) and Bucket.toXContent (:166-190).
"""
import ctypes
import json
import math
import struct

import pytest

import range_ref as RR
import single_metric_stream as SM
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import ShardResult
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from elasticsearch_amd.aggs import flatten, flatten_filters

INF = math.inf
HEAD = b"\xff\x00"       # writeGenericValue(null metaData), 0 pipeline aggregators
RAW = b"\x01\x01"        # formatter present, ValueFormatter.Raw id 1
DATE_FMT = "strict_date_optional_time||epoch_millis"


def _d(v):
    return struct.pack(">d", v)


def _result(aggs):
    return ShardResult.deserialize(RR.record(aggs))


def _mx(v=None):
    return RR.stats(N.AGG_MAX, "m") if v is None else RR.stats(N.AGG_MAX, "m", max=v)


# ---- 1. lowering ---------------------------------------------------------------------------------------------------
def test_builder_lowers_to_type_13_in_request_order():
    r = (AB.range("lat").field("response_time_ms").addRange(100, 500).addUnboundedTo("fast", 100)
         .addUnboundedFrom(500).addRange("mid", 99.5, 100.5).keyed(True).subAggregation(AB.stats("b").field("bytes")))
    specs, n, _keep = flatten([r, AB.range("when").field("@timestamp").addUnboundedFrom(1441065600000)])
    assert n == 3 and [specs[i].type for i in range(n)] == [13, N.AGG_STATS, 13] and N.AGG_RANGE == 13
    assert [specs[i].parent for i in range(n)] == [-1, 0, -1]
    s = specs[0]
    assert (s.n_ranges, s.keyed, s.field, s.value_format) == (4, 1, b"response_time_ms", N.FORMAT_RAW)
    got = [(s.ranges[k].key, s.ranges[k].from_, s.ranges[k].to) for k in range(4)]
    assert got == [(None, 100.0, 500.0), (b"fast", -INF, 100.0), (None, 500.0, INF), (b"mid", 99.5, 100.5)]
    d = specs[2]  # a date field carries its formatter (ValuesSourceParser.resolveFormat)
    assert (d.n_ranges, d.keyed, d.value_format, d.format, d.time_zone) == (1, 0, N.FORMAT_DATE_TIME, DATE_FMT.encode(), b"UTC")
    assert specs[1].n_ranges == 0 and not specs[1].ranges


# ---- 2. esgpu_range_buckets ----------------------------------------------------------------------------------------
def _buckets(builder):
    specs, _n, _keep = flatten([builder])
    order = (ctypes.c_int32 * max(specs[0].n_ranges, 1))()
    need = ctypes.c_size_t()
    rc = N.lib().esgpu_range_buckets(ctypes.byref(specs[0]), order, None, 0, ctypes.byref(need))
    if rc != N.OK:
        return rc, None, None
    buf = ctypes.create_string_buffer(need.value + 1)
    N.check(N.lib().esgpu_range_buckets(ctypes.byref(specs[0]), order, buf, need.value, ctypes.byref(need)))
    keys = buf.raw[: need.value].split(b"\0")[:-1]
    return rc, list(order)[: specs[0].n_ranges], [k.decode() for k in keys]


def test_range_buckets_sort_is_stable_by_from_then_to():
    b = (AB.range("r").field("f").addRange("a", 100, 500).addUnboundedFrom("b", 100).addRange("c", 100, 500)
         .addUnboundedTo("d", 50).addRange("e", -INF, INF).addRange("f", 100, 200).addRange("g", 0.0, 1).addRange("h", -0.0, 1))
    rc, order, keys = _buckets(b)
    # (-inf, 50) (-inf, +inf) | -0.0 before 0.0 (Double.compare) | [100, 200) [100, 500) a before c (stable) [100, +inf)
    assert rc == N.OK and keys == ["d", "e", "h", "g", "f", "a", "c", "b"] and order == [3, 4, 7, 6, 5, 0, 2, 1]
    want = RR.buckets(b._ranges)
    assert [w[0] for w in want] == order and [w[1] for w in want] == keys


def test_range_buckets_generated_and_given_keys():
    b = (AB.range("r").field("f").addRange(50, 100.5).addUnboundedTo(50).addUnboundedFrom(1e7).addRange("given", 1, 2)
         .addRange(-INF, INF).addRange(-2.5, 1e-4))
    rc, order, keys = _buckets(b)
    assert rc == N.OK and keys == ["*-50.0", "*-*", "-2.5-1.0E-4", "given", "50.0-100.5", "1.0E7-*"]
    assert keys == [w[1] for w in RR.buckets(b._ranges)]
    d = AB.range("when").field("@timestamp").addUnboundedFrom(1441065600000).addRange(0, 1441065600123.9)
    rc, order, keys = _buckets(d)
    assert rc == N.OK and order == [1, 0]
    assert keys == ["1970-01-01T00:00:00.000Z-2015-09-01T00:00:00.123Z", "2015-09-01T00:00:00.000Z-*"]


def test_range_buckets_refuses_invalid_input():
    assert _buckets(AB.range("r").field("f"))[0] == N.ERR_INVALID                                # no ranges
    assert _buckets(AB.range("r").field("f").addRange(math.nan, 3))[0] == N.ERR_INVALID
    assert _buckets(AB.range("r").field("f").addRange(0, math.nan))[0] == N.ERR_INVALID
    many = AB.range("r").field("f")
    for k in range(65):
        many.addRange(k, k + 1)
    assert _buckets(many)[0] == N.ERR_UNSUPPORTED
    assert _buckets(AB.range("r").field("f").addRange(0, 1).format("0.00"))[0] == N.ERR_UNSUPPORTED       # DecimalFormat
    assert _buckets(AB.range("r").field("@timestamp").addRange(0, 1).format("yyyy/MM"))[0] == N.ERR_UNSUPPORTED
    specs, _n, _keep = flatten([AB.stats("s").field("f")])
    assert N.lib().esgpu_range_buckets(ctypes.byref(specs[0]), None, None, 0, None) == N.ERR_INVALID  # not a range spec


# ---- 3. transport bytes --------------------------------------------------------------------------------------------
def _two(keyed):
    return RR.range_agg("r", [{"key": "*-100.0", "from": -INF, "to": 100.0, "doc_count": 300, "subs": [_mx(7.0)]},
                              {"key": "big", "from": 100.0, "to": INF, "doc_count": 0, "subs": [_mx()]}], keyed=keyed)


@pytest.mark.parametrize("keyed", [False, True])
def test_range_with_a_max_child_bytes_by_hand(keyed):
    got = _result([_two(keyed)]).to_stream()
    want = (b"\x01" + b"\x05range" + b"\x01r" + HEAD
            + RAW + (b"\x01" if keyed else b"\x00") + b"\x02"                 # formatter, keyed, 2 ranges
            + b"\x01" + b"\x07*-100.0"                                        # writeOptionalString(key)
            + b"\xff\xf0\x00\x00\x00\x00\x00\x00" + _d(100.0)                 # an unbounded side: the raw -Infinity
            + b"\xac\x02"                                                     # writeVLong(300)
            + b"\x01" + b"\x03max\x01m" + HEAD + RAW + _d(7.0)
            + b"\x01" + b"\x03big" + _d(100.0) + b"\x7f\xf0\x00\x00\x00\x00\x00\x00" + b"\x00"
            + b"\x01" + b"\x03max\x01m" + HEAD + RAW + b"\xff\xf0\x00\x00\x00\x00\x00\x00")
    assert got == want


def test_date_formatter_bytes_by_hand():
    r = RR.range_agg("w", [{"key": "k", "from": 0.0, "to": 5.0, "doc_count": 1, "subs": []}],
                     value_format=N.FORMAT_DATE_TIME, format=DATE_FMT)
    want = (b"\x01\x05range\x01w" + HEAD + b"\x01\x02" + bytes([len(DATE_FMT)]) + DATE_FMT.encode() + b"\x03UTC"
            + b"\x00\x01" + b"\x01\x01k" + _d(0.0) + _d(5.0) + b"\x01" + b"\x00")
    assert _result([r]).to_stream() == want


# ---- 4. XContent ---------------------------------------------------------------------------------------------------
def test_xcontent_unkeyed_and_keyed():
    assert _result([_two(False)]).to_xcontent() == (
        '{"r":{"buckets":[{"key":"*-100.0","to":100.0,"to_as_string":"100.0","doc_count":300,"m":{"value":7.0}},'
        '{"key":"big","from":100.0,"from_as_string":"100.0","doc_count":0,"m":{"value":null}}]}}')
    assert _result([_two(True)]).to_xcontent() == (
        '{"r":{"buckets":{"*-100.0":{"to":100.0,"to_as_string":"100.0","doc_count":300,"m":{"value":7.0}},'
        '"big":{"from":100.0,"from_as_string":"100.0","doc_count":0,"m":{"value":null}}}}}')


def test_xcontent_empty_stats_children_and_both_bounds():
    r = RR.range_agg("r", [{"key": "0.5-1.0E7", "from": 0.5, "to": 1e7, "doc_count": 0,
                            "subs": [RR.stats(N.AGG_STATS, "s"), RR.stats(N.AGG_AVG, "a")]},
                           {"key": "*-*", "from": -INF, "to": INF, "doc_count": 2,
                            "subs": [RR.stats(N.AGG_STATS, "s", 2, 5.0, 1.0, 4.0), RR.stats(N.AGG_AVG, "a", 2, 5.0)]}])
    assert _result([r]).to_xcontent() == (
        '{"r":{"buckets":[{"key":"0.5-1.0E7","from":0.5,"from_as_string":"0.5","to":1.0E7,"to_as_string":"1.0E7","doc_count":0,'
        '"s":{"count":0,"min":null,"max":null,"avg":null,"sum":null},"a":{"value":null}},'
        '{"key":"*-*","doc_count":2,"s":{"count":2,"min":1.0,"max":4.0,"avg":2.5,"sum":5.0},"a":{"value":2.5}}]}}')
    d = _result([r]).to_dict()["r"]["buckets"]
    assert set(d[0]) == {"key", "from", "to", "doc_count", "s", "a"} and set(d[1]) == {"key", "doc_count", "s", "a"}
    assert (d[0]["from"], d[0]["to"], d[0]["doc_count"], d[1]["key"]) == (0.5, 1e7, 0, "*-*")


def test_xcontent_date_bounds_as_strings():
    r = RR.range_agg("w", [{"key": "2015-09-01T00:00:00.000Z-*", "from": 1441065600000.0, "to": INF, "doc_count": 4,
                            "subs": []}], value_format=N.FORMAT_DATE_TIME, format=DATE_FMT)
    assert _result([r]).to_xcontent() == ('{"w":{"buckets":[{"key":"2015-09-01T00:00:00.000Z-*","from":1.4410656E12,'
                                          '"from_as_string":"2015-09-01T00:00:00.000Z","doc_count":4}]}}')


# ---- 5. reduce -----------------------------------------------------------------------------------------------------
def _shard(rows):
    """rows: per bucket (doc_count, (count, sum, min, max) or None)"""
    defs = [("*-10.0", -INF, 10.0), ("5.0-20.0", 5.0, 20.0), ("20.0-*", 20.0, INF)]
    bks = []
    for (key, lo, hi), (dc, st) in zip(defs, rows):
        sub = RR.stats(N.AGG_STATS, "s") if st is None else RR.stats(N.AGG_STATS, "s", *st)
        bks.append({"key": key, "from": lo, "to": hi, "doc_count": dc, "subs": [sub]})
    return RR.record([RR.range_agg("r", bks)])


def _three_shards():
    return [_shard([(4, (4, 10.5, 1.0, 6.0)), (2, (1, 7.0, 7.0, 7.0)), (0, None)]),
            _shard([(0, None), (0, None), (0, None)]),                                   # a shard that collected nothing
            _shard([(1, (1, -3.0, -3.0, -3.0)), (5, (5, 60.25, 5.0, 19.5)), (9, (8, 800.0, 20.0, 300.0))])]


def _summary(d):
    return [(b["key"], b["doc_count"], b["s"]["_internal"]["count"], b["s"]["_internal"]["sum"], b["s"]["_internal"]["min"],
             b["s"]["_internal"]["max"]) for b in d["r"]["buckets"]]


HAND_SUMS = [("*-10.0", 5, 5, 7.5, -3.0, 6.0), ("5.0-20.0", 7, 6, 67.25, 5.0, 19.5), ("20.0-*", 9, 8, 800.0, 20.0, 300.0)]


def test_reduce_three_shards_by_position():
    red = reduce([ShardResult.deserialize(b) for b in _three_shards()])
    assert _summary(red.to_dict()) == HAND_SUMS
    a = red.aggregation(0)
    assert (a.type, a.n_buckets, a.nsubs) == (N.AGG_RANGE, 3, 1)
    assert [a.range_from[k] for k in range(3)] == [-INF, 5.0, 20.0] and [a.range_to[k] for k in range(3)] == [10.0, 20.0, INF]
    assert [a.doc_counts[k] for k in range(3)] == [5, 7, 9] and [a.bucket_offsets[k] for k in range(2)] == [0, 3]
    keys = bytes(a.term_bytes[: a.term_offsets[3]])
    assert [keys[a.term_offsets[k]: a.term_offsets[k + 1]] for k in range(3)] == [b"*-10.0", b"5.0-20.0", b"20.0-*"]
    empty = reduce([ShardResult.deserialize(_three_shards()[1])] * 2).to_dict()
    assert [(b["doc_count"], b["s"]["count"], b["s"]["min"]) for b in empty["r"]["buckets"]] == [(0, 0, None)] * 3


def test_reduce_through_the_record_round_trip():
    blobs = _three_shards()
    for b in blobs:
        assert ShardResult.deserialize(b).serialize() == b  # version 7, field for field
    again = [ShardResult.deserialize(ShardResult.deserialize(b).serialize()) for b in blobs]
    assert _summary(reduce(again).to_dict()) == HAND_SUMS


def test_reduce_rejects_shards_with_different_range_counts():
    two = RR.record([RR.range_agg("r", [{"key": "a", "from": 0.0, "to": 1.0, "doc_count": 1, "subs": [RR.stats(N.AGG_STATS, "s")]},
                                        {"key": "b", "from": 1.0, "to": 2.0, "doc_count": 1, "subs": [RR.stats(N.AGG_STATS, "s")]}])])
    with pytest.raises(N.EsGpuError) as e:
        reduce([ShardResult.deserialize(_three_shards()[0]), ShardResult.deserialize(two)])
    assert e.value.code == N.ERR_INVALID and "different numbers of ranges" in str(e.value)


# ---- 6. record versions --------------------------------------------------------------------------------------------
def test_results_without_a_range_keep_their_record_version():
    assert N.lib().esgpu_abi_version() == 7
    v5 = SM.record([SM.single(N.AGG_SUM, "s", 3.5), SM.single(N.AGG_VALUE_COUNT, "c", 12)])
    assert struct.unpack_from("<II", v5) == (0x45534750, 5)
    assert ShardResult.deserialize(v5).serialize() == v5                      # byte for byte, still version 5
    v7 = _three_shards()[0]
    assert struct.unpack_from("<II", v7) == (0x45534750, 7)
    assert struct.unpack_from("<II", ShardResult.deserialize(v7).serialize()) == (0x45534750, 7)
    mixed = reduce([ShardResult.deserialize(v5)]).serialize()                 # a reduce of old blobs stays old
    assert struct.unpack_from("<II", mixed) == (0x45534750, 5)


def test_reader_rejects_inconsistent_range_bounds():
    good = RR.record([RR.stats(N.AGG_STATS, "s", 1, 2.0, 2.0, 2.0)])          # version 7 without a range: readable
    assert ShardResult.deserialize(good).to_dict()["s"]["count"] == 1
    blob = bytearray(_three_shards()[0])
    at = blob.index(struct.pack("<Qddd", 3, -INF, 5.0, 20.0))                 # the `from` vector: length 3 -> 2
    blob[at: at + 8] = struct.pack("<Q", 2)
    del blob[at + 8 + 16: at + 8 + 24]
    with pytest.raises(N.EsGpuError):
        ShardResult.deserialize(bytes(blob))


# ---- 7. two ranks over gloo ----------------------------------------------------------------------------------------
def test_two_rank_gloo_comm_reduce():
    from test_comm_reduce import _run
    blobs = _three_shards() + [_shard([(2, (2, 1.0, 0.25, 0.75)), (0, None), (1, (1, 21.0, 21.0, 21.0))])]
    ref = reduce([ShardResult.deserialize(b) for b in blobs]).to_dict()
    assert _summary(ref) == [("*-10.0", 7, 7, 8.5, -3.0, 6.0), ("5.0-20.0", 7, 6, 67.25, 5.0, 19.5),
                             ("20.0-*", 10, 9, 821.0, 20.0, 300.0)]
    out = _run(2, blobs)
    for r in range(2):
        got, again, _ex = out[r]
        assert json.dumps(got, sort_keys=True) == json.dumps(ref, sort_keys=True) and again == got, f"rank {r}"


# ---- 8. the plan-create contract (validation only: no device call is reached) ------------------------------------------
def _create(aggs, filters=None):
    specs, n, _keep = flatten(aggs)
    flt, nf, _fk = flatten_filters(filters, None, aggs)
    ctx = ctypes.create_string_buffer(1 << 16)  # never read: the checks below throw before any use of the context
    plan = ctypes.c_void_p()
    lib = N.lib()
    rc = lib.esgpu_plan_create(ctypes.cast(ctx, ctypes.c_void_p), specs, n, flt, nf, ctypes.byref(plan))
    buf = ctypes.create_string_buffer(1024)
    lib.esgpu_last_error(buf, 1024)
    return rc, buf.value.decode()


def test_plan_create_refusals():
    ok = lambda: AB.range("r").field("response_time_ms").addRange(0, 100)  # noqa: E731
    assert _create([AB.range("r").field("f")])[0] == N.ERR_INVALID
    assert _create([AB.range("r").field("f").addRange(math.nan, 1)])[0] == N.ERR_INVALID
    many = AB.range("r").field("f")
    for k in range(65):
        many.addRange(k, k + 1)
    assert _create([many])[0] == N.ERR_UNSUPPORTED
    for parent in (AB.terms("t").field("host"), AB.dateHistogram("h").field("@timestamp").interval("1h"),
                   AB.filter("f", QB.termQuery("status", 200)), ok()):
        rc, msg = _create([parent.subAggregation(ok())])
        assert rc == N.ERR_UNSUPPORTED, msg
    for child in (AB.cardinality("c").field("client_ip.hash"), AB.terms("t").field("host"),
                  AB.histogram("h").field("bytes").interval(10), AB.filter("f", QB.termQuery("status", 200))):
        rc, msg = _create([ok().subAggregation(child)])
        assert rc == N.ERR_UNSUPPORTED, msg
    assert _create([ok().format("0.0")])[0] == N.ERR_UNSUPPORTED
