"""The filters aggregation on the CPU: builder lowering (spec fields, clause owners and slots, the builder's errors),
transport bytes and XContent of hand-built blocks, their reduce by position (in process, through the shard record, across
two gloo ranks), the record versions and the plan-create refusals.

Hand-derived bytes follow InternalAggregation.writeTo (A/InternalAggregation.java:212-221), InternalFilters.doWriteTo
(A/bucket/filters/InternalFilters.java:245-251), Bucket.writeTo (:153-157) and StreamOutput's encodings; the XContent
strings InternalFilters.doXContentBody (:254-268) and Bucket.toXContent (:133-143).
"""
import ctypes
import json
import struct

import pytest

import filters_ref as FR
import long_terms_stream as LT
import range_ref as RR
import single_metric_stream as SM
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import ShardResult
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from elasticsearch_amd.aggs import flatten, flatten_filters

HEAD = b"\xff\x00"       # writeGenericValue(null metaData), 0 pipeline aggregators
RAW = b"\x01\x01"        # formatter present, ValueFormatter.Raw id 1


def _d(v):
    return struct.pack(">d", v)


def _result(aggs):
    return ShardResult.deserialize(FR.record(aggs))


def _mx(v=None):
    return FR.stats(N.AGG_MAX, "m") if v is None else FR.stats(N.AGG_MAX, "m", max=v)


# ---- 1. lowering ---------------------------------------------------------------------------------------------------
def test_builder_lowers_to_type_14_with_owners_and_slots():
    f = (AB.filters("cls").filter("ok", QB.termQuery("status", 200))
         .filter("slow", [QB.rangeQuery("response_time_ms").gte(500), QB.rangeQuery("bytes").lt(1000)])
         .filter("all", []).filter("ok", QB.termQuery("status", 404))     # a repeated key: new query, old position
         .otherBucket(True).subAggregation(AB.stats("b").field("bytes")))
    anon = AB.filters("anon").filter(QB.termQuery("status", 500)).filter([]).otherBucketKey("rest")
    aggs = [AB.stats("s").field("bytes"), f, anon]
    specs, n, _keep = flatten(aggs)
    assert N.AGG_FILTERS == 14 and [specs[i].type for i in range(n)] == [N.AGG_STATS, 14, N.AGG_STATS, 14]
    assert [specs[i].parent for i in range(n)] == [-1, -1, 1, -1]
    s = specs[1]
    assert (s.n_filters, s.keyed, s.other_bucket, s.other_bucket_key) == (3, 1, 1, None)
    assert [s.filter_keys[k] for k in range(3)] == [b"ok", b"slow", b"all"]
    a = specs[3]
    assert (a.n_filters, a.keyed, a.other_bucket, a.other_bucket_key) == (2, 0, 1, b"rest")  # a key implies the bucket
    assert [a.filter_keys[k] for k in range(2)] == [b"0", b"1"]
    assert specs[0].n_filters == 0 and not specs[0].filter_keys and specs[0].other_bucket == 0
    flt, nf, _fk = flatten_filters([QB.termQuery("status", 200)], None, aggs)
    got = [(flt[k].owner, flt[k].slot, flt[k].field, flt[k].type) for k in range(nf)]
    assert got == [(0, 0, b"status", N.FILTER_TERM),                       # the query clause
                   (2, 0, b"status", N.FILTER_TERM),                       # cls / ok (owner = spec index + 1)
                   (2, 1, b"response_time_ms", N.FILTER_RANGE), (2, 1, b"bytes", N.FILTER_RANGE),
                   (4, 0, b"status", N.FILTER_TERM)]                       # anon / 0; the match_all filters have no clause
    assert flt[1].term == 404 and (flt[2].has_lower, flt[2].include_lower, flt[2].lo_i, flt[2].has_upper) == (1, 1, 500, 0)
    assert (flt[3].has_upper, flt[3].include_upper, flt[3].hi_i) == (1, 0, 1000)


def test_snake_case_aliases_and_infinite_bounds():
    f = AB.filters("f").filter("a", QB.rangeQuery("price").gt(float("inf"))).other_bucket(True).other_bucket_key("o")
    specs, _n, _keep = flatten([f])
    assert (specs[0].other_bucket, specs[0].other_bucket_key) == (1, b"o")
    assert AB.filters("f").filter("a", []).other_bucket_key("o")._other is True
    flt, nf, _fk = flatten_filters(None, None, [f])
    assert nf == 1 and flt[0].lo_d == float("inf") and flt[0].lo_i == (1 << 63) - 1 and flt[0].include_lower == 0
    with pytest.raises(ValueError):  # a NaN bound is refused, as before
        flatten_filters([QB.rangeQuery("bytes").gte(float("nan"))])


def test_builder_errors():
    with pytest.raises(ValueError):
        flatten([AB.filters("f")])                                                   # no filter at all
    with pytest.raises(ValueError):
        flatten([AB.filters("f").filter("a", []).filter(QB.termQuery("status", 1))])  # keyed and anonymous mixed
    with pytest.raises(ValueError):
        flatten_filters(None, None, [AB.filters("f").otherBucket(True)])
    with pytest.raises(TypeError):
        AB.filters("f").filter()


# ---- 2. transport bytes --------------------------------------------------------------------------------------------
def _small(keyed=True):
    return FR.filters_agg("f", [{"key": "errors", "doc_count": 300, "subs": [_mx(7.0)]},
                                {"key": "all", "doc_count": 2, "subs": [_mx(0.5)]},
                                {"key": "_other_", "doc_count": 0, "subs": [_mx()]}], keyed=keyed)


def test_keyed_block_with_an_other_bucket_bytes_by_hand():
    got = _result([_small()]).to_stream()
    want = (b"\x01" + b"\x07filters" + b"\x01f" + HEAD
            + b"\x01" + b"\x03"                                               # keyed, 3 buckets (no formatter)
            + b"\x01" + b"\x06errors" + b"\xac\x02"                           # writeOptionalString(key), writeVLong(300)
            + b"\x01" + b"\x03max\x01m" + HEAD + RAW + _d(7.0)
            + b"\x01" + b"\x03all" + b"\x02"
            + b"\x01" + b"\x03max\x01m" + HEAD + RAW + _d(0.5)
            + b"\x01" + b"\x07_other_" + b"\x00"
            + b"\x01" + b"\x03max\x01m" + HEAD + RAW + b"\xff\xf0\x00\x00\x00\x00\x00\x00")
    assert got == want
    dec = FR.decode_stream(got)
    assert dec[0]["stream_type"] == "filters" and dec[0]["keyed"] is True
    assert [(b["key"], b["doc_count"], b["aggs"][0]["value"]) for b in dec[0]["buckets"]] == [
        ("errors", 300, 7.0), ("all", 2, 0.5), ("_other_", 0, float("-inf"))]


def test_anonymous_block_bytes_by_hand():
    a = FR.filters_agg("f", [{"key": "0", "doc_count": 1, "subs": []}, {"key": "1", "doc_count": 128, "subs": []}], keyed=False)
    want = (b"\x01\x07filters\x01f" + HEAD + b"\x00\x02" + b"\x01\x010\x01\x00" + b"\x01\x011\x80\x01\x00")
    assert _result([a]).to_stream() == want


# ---- 3. XContent ---------------------------------------------------------------------------------------------------
def test_xcontent_keyed_and_anonymous():
    assert _result([_small(True)]).to_xcontent() == (
        '{"f":{"buckets":{"errors":{"doc_count":300,"m":{"value":7.0}},"all":{"doc_count":2,"m":{"value":0.5}},'
        '"_other_":{"doc_count":0,"m":{"value":null}}}}}')
    anon = FR.filters_agg("f", [{"key": "0", "doc_count": 300, "subs": [FR.stats(N.AGG_STATS, "s", 2, 5.0, 1.0, 4.0)]},
                                {"key": "1", "doc_count": 0, "subs": [FR.stats(N.AGG_STATS, "s")]}], keyed=False)
    assert _result([anon]).to_xcontent() == (
        '{"f":{"buckets":[{"doc_count":300,"s":{"count":2,"min":1.0,"max":4.0,"avg":2.5,"sum":5.0}},'
        '{"doc_count":0,"s":{"count":0,"min":null,"max":null,"avg":null,"sum":null}}]}}')
    d = _result([anon]).to_dict()["f"]["buckets"]
    assert [(b["key"], b["doc_count"]) for b in d] == [("0", 300), ("1", 0)] and set(d[0]) == {"key", "doc_count", "s"}


# ---- 4. reduce -----------------------------------------------------------------------------------------------------
KEYS = ("fast", "slow", "_other_")


def _shard(rows, keys=KEYS):
    """rows: per bucket (doc_count, (count, sum, min, max) or None)"""
    bks = []
    for key, (dc, st) in zip(keys, rows):
        sub = FR.stats(N.AGG_STATS, "s") if st is None else FR.stats(N.AGG_STATS, "s", *st)
        bks.append({"key": key, "doc_count": dc, "subs": [sub]})
    return FR.record([FR.filters_agg("f", bks)])


def _three_shards():
    return [_shard([(4, (4, 10.5, 1.0, 6.0)), (2, (1, 7.0, 7.0, 7.0)), (0, None)]),
            _shard([(0, None), (0, None), (0, None)]),                                   # a shard that collected nothing
            _shard([(1, (1, -3.0, -3.0, -3.0)), (5, (5, 60.25, 5.0, 19.5)), (9, (8, 800.0, 20.0, 300.0))])]


def _summary(d):
    return [(b["key"], b["doc_count"], b["s"]["_internal"]["count"], b["s"]["_internal"]["sum"], b["s"]["_internal"]["min"],
             b["s"]["_internal"]["max"]) for b in d["f"]["buckets"]]


HAND_SUMS = [("fast", 5, 5, 7.5, -3.0, 6.0), ("slow", 7, 6, 67.25, 5.0, 19.5), ("_other_", 9, 8, 800.0, 20.0, 300.0)]


def test_reduce_three_shards_by_position():
    red = reduce([ShardResult.deserialize(b) for b in _three_shards()])
    assert _summary(red.to_dict()) == HAND_SUMS
    a = red.aggregation(0)
    assert (a.type, a.n_buckets, a.nsubs, a.keyed) == (N.AGG_FILTERS, 3, 1, 1)
    assert [a.doc_counts[k] for k in range(3)] == [5, 7, 9] and [a.bucket_offsets[k] for k in range(2)] == [0, 3]
    keys = bytes(a.term_bytes[: a.term_offsets[3]])
    assert [keys[a.term_offsets[k]: a.term_offsets[k + 1]] for k in range(3)] == [b"fast", b"slow", b"_other_"]
    empty = reduce([ShardResult.deserialize(_three_shards()[1])] * 2).to_dict()
    assert [(b["doc_count"], b["s"]["count"], b["s"]["min"]) for b in empty["f"]["buckets"]] == [(0, 0, None)] * 3


def test_record_round_trip_is_version_8_byte_for_byte():
    blobs = _three_shards()
    for b in blobs:
        assert struct.unpack_from("<II", b) == (0x45534750, 8)
        assert ShardResult.deserialize(b).serialize() == b
    again = [ShardResult.deserialize(ShardResult.deserialize(b).serialize()) for b in blobs]
    assert _summary(reduce(again).to_dict()) == HAND_SUMS
    assert struct.unpack_from("<II", reduce(again).serialize()) == (0x45534750, 8)


def test_reduce_rejects_shards_with_different_bucket_counts():
    two = _shard([(1, None), (1, None)], keys=("fast", "slow"))
    with pytest.raises(N.EsGpuError) as e:
        reduce([ShardResult.deserialize(_three_shards()[0]), ShardResult.deserialize(two)])
    assert e.value.code == N.ERR_INVALID and "different numbers of buckets" in str(e.value)


# ---- 5. record versions --------------------------------------------------------------------------------------------
def test_results_without_a_filters_block_keep_their_record_version():
    assert N.lib().esgpu_abi_version() == 7
    v5 = SM.record([SM.single(N.AGG_SUM, "s", 3.5), SM.single(N.AGG_VALUE_COUNT, "c", 12)])
    assert struct.unpack_from("<II", v5) == (0x45534750, 5)
    assert ShardResult.deserialize(v5).serialize() == v5
    v6 = LT.encode6([LT.long_terms("t", [(10, 5), (9, 5), (-3, 1)])])                   # a LongTerms block: version 6
    assert struct.unpack_from("<II", v6) == (0x45534750, 6)
    assert ShardResult.deserialize(v6).serialize() == v6                       # byte for byte, still version 6
    assert struct.unpack_from("<II", reduce([ShardResult.deserialize(v6)] * 2).serialize()) == (0x45534750, 6)
    v7 = RR.record([RR.range_agg("r", [{"key": "a", "from": 0.0, "to": 1.0, "doc_count": 1, "subs": []}])])
    assert struct.unpack_from("<II", v7) == (0x45534750, 7)
    assert ShardResult.deserialize(v7).serialize() == v7
    stats8 = FR.record([FR.stats(N.AGG_STATS, "s", 1, 2.0, 2.0, 2.0)])       # version 8 without a filters block: readable,
    r = ShardResult.deserialize(stats8)                                        # and written back as what it holds
    assert r.to_dict()["s"]["count"] == 1 and struct.unpack_from("<II", r.serialize())[1] == 5
    for bad in (4, 9):
        with pytest.raises(N.EsGpuError):
            ShardResult.deserialize(FR.record([_small()], version=bad))


# ---- 6. two ranks over gloo ----------------------------------------------------------------------------------------
def test_two_rank_gloo_comm_reduce():
    from test_comm_reduce import _run
    blobs = _three_shards() + [_shard([(2, (2, 1.0, 0.25, 0.75)), (0, None), (1, (1, 21.0, 21.0, 21.0))])]
    ref = reduce([ShardResult.deserialize(b) for b in blobs]).to_dict()
    assert _summary(ref) == [("fast", 7, 7, 8.5, -3.0, 6.0), ("slow", 7, 6, 67.25, 5.0, 19.5),
                             ("_other_", 10, 9, 821.0, 20.0, 300.0)]
    out = _run(2, blobs)
    for r in range(2):
        got, again, _ex = out[r]
        assert json.dumps(got, sort_keys=True) == json.dumps(ref, sort_keys=True) and again == got, f"rank {r}"


# ---- 7. the plan-create contract (validation only: no device call is reached) ------------------------------------------
def _create_raw(specs, n, flt, nf):
    ctx = ctypes.create_string_buffer(1 << 16)  # never read: the checks below throw before any use of the context
    plan = ctypes.c_void_p()
    lib = N.lib()
    rc = lib.esgpu_plan_create(ctypes.cast(ctx, ctypes.c_void_p), specs, n, flt, nf, ctypes.byref(plan))
    buf = ctypes.create_string_buffer(1024)
    lib.esgpu_last_error(buf, 1024)
    return rc, buf.value.decode()


def _create(aggs, filters=None):
    specs, n, _keep = flatten(aggs)
    flt, nf, _fk = flatten_filters(filters, None, aggs)
    return _create_raw(specs, n, flt, nf)


def _many(n, other=False):
    f = AB.filters("f").otherBucket(other)
    for k in range(n):
        f.filter("k%d" % k, QB.termQuery("status", k))
    return f


def test_plan_create_refusals():
    ok = lambda: AB.filters("f").filter("a", QB.termQuery("status", 200))  # noqa: E731
    specs, n, _keep = flatten([ok()])
    specs[0].n_filters = 0                                                    # no filter (the builder itself raises)
    rc, msg = _create_raw(specs, n, None, 0)
    assert rc == N.ERR_INVALID, msg
    assert _create([_many(65)])[0] == N.ERR_UNSUPPORTED
    assert _create([_many(64, other=True)])[0] == N.ERR_UNSUPPORTED
    for parent in (AB.terms("t").field("host"), AB.dateHistogram("h").field("@timestamp").interval("1h"),
                   AB.filter("p", QB.termQuery("status", 200)), ok(),
                   AB.range("r").field("bytes").addRange(0, 1)):
        rc, msg = _create([parent.subAggregation(AB.filters("g").filter("a", QB.termQuery("status", 200)))])
        assert rc == N.ERR_UNSUPPORTED, msg
    for child in (AB.cardinality("c").field("client_ip.hash"), AB.terms("t").field("host"),
                  AB.histogram("h").field("bytes").interval(10), AB.filter("p", QB.termQuery("status", 200)),
                  AB.range("r").field("bytes").addRange(0, 1)):
        rc, msg = _create([ok().subAggregation(child)])
        assert rc == N.ERR_UNSUPPORTED, msg
    specs, n, _keep = flatten([ok()])
    flt, nf, _fk = flatten_filters(None, None, [ok()])
    flt[0].slot = 1                                                           # a slot that is no filter of its owner
    rc, msg = _create_raw(specs, n, flt, nf)
    assert rc == N.ERR_INVALID, msg
