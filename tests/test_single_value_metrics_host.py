"""sum / min / max / value_count on the CPU: transport bytes and XContent of hand-built blocks, their reduce (in process,
through the shard record, across two gloo ranks), the plan-create contract and the builder lowering.

Hand-derived bytes follow line by line from InternalAggregation.writeTo (A/InternalAggregation.java:212-221), the four
doWriteTo methods (InternalSum.java:97-100, InternalMin.java:97-100, InternalMax.java:96-99, InternalValueCount.java:
97-100), ValueFormatterStreams.writeOptional and StreamOutput's encodings, as in test_wire_stream.py.
"""
import ctypes
import json
import math
import struct

import pytest

import single_metric_stream as SM
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Order, ShardResult
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from elasticsearch_amd.aggs import flatten

SUM, MIN, MAX, COUNT = N.AGG_SUM, N.AGG_MIN, N.AGG_MAX, N.AGG_VALUE_COUNT


def _result(aggs):
    return ShardResult.deserialize(SM.record(aggs))


def _d(v):
    return struct.pack(">d", v)


HEAD = b"\xff\x00"       # writeGenericValue(null metaData), 0 pipeline aggregators
RAW = b"\x01\x01"        # formatter present, ValueFormatter.Raw id 1


# ---- 1. transport bytes --------------------------------------------------------------------------------------------
def test_top_level_bytes_by_hand():
    got = _result([SM.single(SUM, "s", 3.5), SM.single(MIN, "lo", -2.0), SM.single(MAX, "hi", 1e300),
                   SM.single(COUNT, "c", 300)]).to_stream()
    want = (b"\x04"
            + b"\x03sum" + b"\x01s" + HEAD + RAW + _d(3.5)                    # writeDouble(sum)
            + b"\x03min" + b"\x02lo" + HEAD + RAW + _d(-2.0)
            + b"\x03max" + b"\x02hi" + HEAD + RAW + _d(1e300)
            + b"\x0bvalue_count" + b"\x01c" + HEAD + RAW + b"\xac\x02")       # writeVLong(300) = ac 02
    assert got == want


def test_empty_instances_bytes_by_hand():
    got = _result([SM.single(SUM, "s"), SM.single(MIN, "lo"), SM.single(MAX, "hi"), SM.single(COUNT, "c")]).to_stream()
    want = (b"\x04"
            + b"\x03sum\x01s" + HEAD + RAW + _d(0.0)
            + b"\x03min\x02lo" + HEAD + RAW + b"\x7f\xf0\x00\x00\x00\x00\x00\x00"   # +Infinity
            + b"\x03max\x02hi" + HEAD + RAW + b"\xff\xf0\x00\x00\x00\x00\x00\x00"   # -Infinity
            + b"\x0bvalue_count\x01c" + HEAD + RAW + b"\x00")
    assert got == want


def test_number_pattern_formatter_bytes_by_hand():
    got = _result([SM.single(SUM, "s", 2.0, value_format=N.FORMAT_NUMBER, format="0.00")]).to_stream()
    want = (b"\x01" + b"\x03sum\x01s" + HEAD
            + b"\x01\x04" + b"\x040.00"                                       # Number.Pattern id 4, writeString(pattern)
            + _d(2.0))
    assert got == want


def test_nested_under_string_terms_bytes_by_hand():
    t = {"type": N.AGG_TERMS, "name": "t", "required_size": 2, "shard_size": 5, "other_doc_count": 4,
         "buckets": [{"term": "b", "doc_count": 5, "subs": [SM.single(MAX, "m", 7.0), SM.single(COUNT, "c", 5)]}]}
    got = _result([t]).to_stream()
    want = (b"\x01" + b"\x06sterms" + b"\x01t" + HEAD
            + struct.pack(">q", 0)                                            # docCountError
            + b"\xff\x02\x01\x04"                                             # CompoundOrder[_count desc, _term asc]
            + b"\x02\x05" + b"\x00" + b"\x01" + b"\x04"                       # sizes, showError, minDocCount, other
            + b"\x01" + b"\x01b" + b"\x05"                                    # 1 bucket: term, docCount
            + b"\x02"                                                         # its 2 sub-aggregations
            + b"\x03max\x01m" + HEAD + RAW + _d(7.0)
            + b"\x0bvalue_count\x01c" + HEAD + RAW + b"\x05")
    assert got == want


# ---- 2. XContent ---------------------------------------------------------------------------------------------------
def test_xcontent_strings():
    r = _result([SM.single(SUM, "s", 3.5), SM.single(MIN, "lo"), SM.single(MAX, "hi"), SM.single(COUNT, "c", 12),
                 SM.single(MIN, "lo2", -0.0), SM.single(SUM, "nan", math.nan)])
    assert r.to_xcontent() == ('{"s":{"value":3.5},"lo":{"value":null},"hi":{"value":null},"c":{"value":12},'
                               '"lo2":{"value":-0.0},"nan":{"value":NaN}}')
    for kind, v in ((SUM, 3.5), (MIN, math.inf), (MAX, -math.inf), (COUNT, 12), (MIN, -0.0)):
        assert _result([SM.single(kind, "x", v)]).to_xcontent() == '{"x":%s}' % SM.xcontent_single(kind, v)


def test_xcontent_value_as_string_with_date_formatter():
    fmt = dict(value_format=N.FORMAT_DATE_TIME, format="strict_date_optional_time||epoch_millis")
    r = _result([SM.single(MAX, "last", 1441065600123.0, **fmt), SM.single(MAX, "none", **fmt),
                 SM.single(COUNT, "c", 0, **fmt)])
    assert r.to_xcontent() == ('{"last":{"value":1.441065600123E12,"value_as_string":"2015-09-01T00:00:00.123Z"},'
                               '"none":{"value":null},'                      # no value: no value_as_string either
                               '"c":{"value":0,"value_as_string":"1970-01-01T00:00:00.000Z"}}')
    d = r.to_dict()
    assert d["last"] == {"value": 1441065600123.0, "value_as_string": "2015-09-01T00:00:00.123Z"}
    assert d["none"] == {"value": -math.inf} and d["c"]["value"] == 0 and isinstance(d["c"]["value"], int)


# ---- 3. reduce -----------------------------------------------------------------------------------------------------
def _shards():
    """three shards; the third collected nothing"""
    vals = [(10.5, 3.0, 9.0, 4), (0.25, -1.0, 2.0, 2), (None, None, None, None)]
    return [SM.record([SM.single(SUM, "s", s), SM.single(MIN, "lo", lo), SM.single(MAX, "hi", hi), SM.single(COUNT, "c", c)])
            for s, lo, hi, c in vals]


def test_reduce_operators_over_three_shards():
    red = reduce([ShardResult.deserialize(b) for b in _shards()])
    assert red.to_dict() == {"s": {"value": 10.75}, "lo": {"value": -1.0}, "hi": {"value": 9.0}, "c": {"value": 6}}
    a = red.aggregation
    assert (a(0).sum[0], a(1).min[0], a(2).max[0], a(3).count[0]) == (10.75, -1.0, 9.0, 6)
    # the arrays a block does not fill hold the empty aggregation's values
    assert (a(0).count[0], a(0).min[0], a(0).max[0]) == (0, math.inf, -math.inf)
    assert (a(3).sum[0], a(1).sum[0], a(1).count[0]) == (0.0, 0.0, 0)
    empty = reduce([ShardResult.deserialize(_shards()[2])] * 2).to_dict()
    assert empty == {"s": {"value": 0.0}, "lo": {"value": math.inf}, "hi": {"value": -math.inf}, "c": {"value": 0}}


def test_nan_propagates_through_min_and_max():
    blobs = [SM.record([SM.single(MIN, "lo", v), SM.single(MAX, "hi", v)]) for v in (1.0, math.nan, -5.0)]
    d = reduce([ShardResult.deserialize(b) for b in blobs]).to_dict()
    assert math.isnan(d["lo"]["value"]) and math.isnan(d["hi"]["value"])  # Math.min / Math.max


def test_record_round_trip_then_reduce():
    blobs = _shards()
    for b in blobs:
        assert ShardResult.deserialize(b).serialize() == b  # version 5: the layout did not change
    again = [ShardResult.deserialize(ShardResult.deserialize(b).serialize()) for b in blobs]
    assert reduce(again).to_dict() == {"s": {"value": 10.75}, "lo": {"value": -1.0}, "hi": {"value": 9.0}, "c": {"value": 6}}


def test_reader_rejects_a_bucket_payload_on_a_single_value_block():
    for kind in (SUM, MIN, MAX, COUNT):
        ShardResult.deserialize(SM.record([SM.single(kind, "x", 1)]))
        bad = SM.record([SM.single(kind, "x", 1, buckets=[{"term": "b", "doc_count": 1, "subs": []}])])
        with pytest.raises(N.EsGpuError, match="bucket payload on a single-value metric block"):
            ShardResult.deserialize(bad)


def test_reduce_under_terms_orders_by_the_reduced_value():
    def shard(rows):
        return SM.record([{"type": N.AGG_TERMS, "name": "t", "order": N.ORDER_AGG_DESC, "order_path": "m", "required_size": 2,
                           "shard_size": 3, "buckets": [{"term": k, "doc_count": n, "subs": [SM.single(SUM, "m", v)]}
                                                        for k, n, v in rows]}])
    red = reduce([ShardResult.deserialize(shard([("a", 1, 5.0), ("b", 2, 4.0), ("c", 1, 1.0)])),
                  ShardResult.deserialize(shard([("b", 1, 3.0), ("c", 9, 0.5)]))]).to_dict()["t"]
    assert [(b["key"], b["doc_count"], b["m"]["value"]) for b in red["buckets"]] == [("b", 3, 7.0), ("a", 1, 5.0)]
    assert red["doc_count_error_upper_bound"] == -1


def test_two_rank_gloo_comm_reduce():
    from test_comm_reduce import _run
    blobs = _shards() + [SM.record([SM.single(SUM, "s", 1.0), SM.single(MIN, "lo", -7.5), SM.single(MAX, "hi", 0.0),
                                    SM.single(COUNT, "c", 1)])]
    ref = reduce([ShardResult.deserialize(b) for b in blobs]).to_dict()
    assert ref == {"s": {"value": 11.75}, "lo": {"value": -7.5}, "hi": {"value": 9.0}, "c": {"value": 7}}
    out = _run(2, blobs)
    for r in range(2):
        got, again, _ex = out[r]
        assert json.dumps(got, sort_keys=True) == json.dumps(ref, sort_keys=True) and again == got, f"rank {r}"


# ---- 4. the plan-create contract through the C-ABI (validation only: no device call is reached) ----------------------
def _create(aggs):
    specs, n, _keep = flatten(aggs)
    ctx = ctypes.create_string_buffer(1 << 16)  # never read: the checks below throw before any use of the context
    plan = ctypes.c_void_p()
    lib = N.lib()
    rc = lib.esgpu_plan_create(ctypes.cast(ctx, ctypes.c_void_p), specs, n, None, 0, ctypes.byref(plan))
    buf = ctypes.create_string_buffer(1024)
    lib.esgpu_last_error(buf, 1024)
    return rc, buf.value.decode()


def test_plan_create_contract():
    assert N.lib().esgpu_abi_version() == 7
    s = AB.sum("s").field("bytes")
    s.subs.append(AB.max("m").field("bytes"))  # (the builder refuses subAggregation on a metric: lowered by hand)
    rc, msg = _create([AB.terms("t").field("host").subAggregation(s)])
    assert rc == N.ERR_INVALID and "metrics aggregations cannot have sub-aggregations" in msg
    for kind in (AB.sum, AB.min, AB.max, AB.count):
        t = AB.terms("t").field("host").order(Order.aggregation("s.sum", True)).subAggregation(kind("s").field("bytes"))
        rc, msg = _create([t])
        assert rc == N.ERR_INVALID and "Ordering on a single-value metrics aggregation can only be done on its value" in msg


# ---- 5. builder lowering -------------------------------------------------------------------------------------------
def test_builders_flatten_to_types_8_to_11():
    t = AB.terms("t").field("host").order(Order.aggregation("s.value", False))
    for b in (AB.sum("s").field("bytes").format("0.0"), AB.min("lo").field("bytes"), AB.max("hi").field("@timestamp"),
              AB.count("c").field("host")):
        t.subAggregation(b)
    specs, n, _keep = flatten([t, AB.count("all").field("url")])
    assert n == 6
    assert [specs[i].type for i in range(n)] == [N.AGG_TERMS, 8, 9, 10, 11, 11]
    assert [specs[i].parent for i in range(n)] == [-1, 0, 0, 0, 0, -1]
    assert [specs[i].field for i in range(1, 6)] == [b"bytes", b"bytes", b"@timestamp", b"host", b"url"]
    assert (specs[1].value_format, specs[1].format) == (N.FORMAT_NUMBER, b"0.0")
    assert specs[2].value_format == N.FORMAT_RAW and specs[3].value_format == N.FORMAT_DATE_TIME
    assert specs[0].order == N.ORDER_AGG_DESC and specs[0].order_path == b"s.value"
    with pytest.raises(ValueError):
        AB.sum("s").subAggregation(AB.max("m"))
