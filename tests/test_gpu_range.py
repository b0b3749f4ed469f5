"""The range aggregation on the GPU (collect path 11, esgpu_range.hip) against two references that never run the code
under test: tests/range_ref.py's numpy restatement of RangeAggregator (masks over (double) values, counts, min / max,
integer sums exact in int64, math.fsum for doubles) and the filter twin -- every range with integral bounds as a
top-level filter aggregation with rangeQuery(f).gte(from).lt(to) and the same children, run through the oracle.

Counts, keys and integer-valued metrics are compared bit-exactly, non-integer doubles within the project's 1e-12 of the
exact sum (math.fsum) or of the oracle's (helpers.assert_same).  Shards are 3 * 8192 + 17 docs (a partial last zone block
plus padding) unless a case says otherwise.
"""
import math

import numpy as np
import pytest

import oracle as O
import range_ref as RR
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from helpers import REL_TOL, assert_same, bits_from_mask, synthetic_columns
from test_gpu_multivalued import csr_sorted

pytestmark = pytest.mark.gpu

INF = math.inf
NDOCS = 3 * 8192 + 17
FIELDS = ("status", "response_time_ms", "bytes", "price")
LATENCY = [(None, -INF, 100), (None, 100, 500), (None, 500, INF), (None, 0, 1000), (None, 250, 250), (None, 600, 300),
           (None, 100, 500)]
CLASSES = [("fast", -INF, 100), (None, 100, 500), ("slow", 500, INF), (None, 0, 1000)]  # integral bounds: twin-able


@pytest.fixture(scope="module")
def cols():
    """the synthetic shard on the host: computed once, shared, never modified"""
    return synthetic_columns(FIELDS, NDOCS)


@pytest.fixture(scope="module")
def seg(engine):
    s = engine.synthetic_segment(NDOCS, fields=FIELDS)
    yield s
    s.close()


def rng_agg(name, field, ranges, subs=(), keyed=False):
    b = AB.range(name).field(field).keyed(keyed)
    for key, lo, hi in ranges:
        b.addRange(lo, hi) if key is None else b.addRange(key, lo, hi)
    for s in subs:
        b.subAggregation(s)
    return b


def run(engine, segs, aggs, filters=None, accept=None):
    plan = engine.plan(aggs, filters=filters)
    for i, s in enumerate(segs):
        plan.collect(s, accept_bits=None if accept is None else accept[i])
    res = plan.build()
    stats = plan.last_collect_stats()
    plan.close()
    return res, stats


def check_buckets(got, bks, masks):
    """keys, bounds and doc counts of a rendered range against the reference buckets and doc masks"""
    assert [b["key"] for b in got["buckets"]] == [k for _i, k, _lo, _hi in bks]
    for b, (_i, _k, lo, hi), m in zip(got["buckets"], bks, masks):
        assert ("from" in b) == (not math.isinf(lo)) and ("to" in b) == (not math.isinf(hi)), b
        assert b.get("from", lo) == lo and b.get("to", hi) == hi, b
        assert b["doc_count"] == int(m.sum()), (b["key"], b["doc_count"], int(m.sum()))


def close(a, b, exact):
    if exact or math.isinf(b) or b == 0:
        return a == b
    return abs(a - b) <= REL_TOL * max(abs(a), abs(b))


def check_leaf(leaf, kind, want, exact=True, path=""):
    """a rendered metric leaf against (count, exact sum, min, max)"""
    cnt, s, mn, mx = want
    if kind == N.AGG_SUM:
        assert close(leaf["value"], s, exact), (path, leaf, s)
    elif kind == N.AGG_MIN:
        assert leaf["value"] == mn, (path, leaf, mn)
    elif kind == N.AGG_MAX:
        assert leaf["value"] == mx, (path, leaf, mx)
    elif kind == N.AGG_VALUE_COUNT:
        assert leaf["value"] == cnt and isinstance(leaf["value"], int), (path, leaf, cnt)
    else:
        st = leaf["_internal"]
        assert st["count"] == cnt and close(st["sum"], s, exact), (path, st, want)
        if kind != N.AGG_AVG:
            assert st["min"] == mn and st["max"] == mx, (path, st, want)
            assert leaf["count"] == cnt and leaf["min"] == (mn if cnt else None) and leaf["max"] == (mx if cnt else None)


def check_metrics(got, masks, leaves, exact=True):
    """leaves: (name, kind, values, present or None)"""
    for k, (b, m) in enumerate(zip(got["buckets"], masks)):
        for name, kind, vals, pres in leaves:
            check_leaf(b[name], kind, RR.metric(m, vals, pres), exact, "%s[%d].%s" % (got.get("name", "range"), k, name))


def check_twin(got, want_reduced, nb, exact=True):
    """bucket i of the range against filter aggregation f<i> of the twin's oracle result"""
    assert len(got["buckets"]) == nb
    for i, b in enumerate(got["buckets"]):
        w = want_reduced["f%d" % i]
        assert b["doc_count"] == w["doc_count"], (i, b["doc_count"], w["doc_count"])
        for name in w:
            if name != "doc_count":
                assert_same(b[name], w[name], "bucket[%d].%s" % (i, name), exact)


# ---- counts --------------------------------------------------------------------------------------------------------
def test_counts_only_overlapping_degenerate_and_duplicate_ranges(engine, seg, cols):
    res, stats = run(engine, [seg], [rng_agg("lat", "response_time_ms", LATENCY)])
    got = res.to_dict()["lat"]
    bks = RR.buckets(LATENCY)
    masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
    check_buckets(got, bks, masks)
    assert [b["key"] for b in got["buckets"]] == ["*-100.0", "0.0-1000.0", "100.0-500.0", "100.0-500.0", "250.0-250.0",
                                                  "500.0-*", "600.0-300.0"]
    counts = {(lo, hi): b["doc_count"] for b, (_i, _k, lo, hi) in zip(got["buckets"], bks)}
    assert counts[(250.0, 250.0)] == 0 and counts[(600.0, 300.0)] == 0
    assert all(c > 0 for (lo, hi), c in counts.items() if lo < hi) and counts[(0.0, 1000.0)] == NDOCS
    assert stats[2] == 11 and stats[1] == 8 * NDOCS  # the one column at the 8 bytes read


def _upload(engine, columns, n):
    return engine.upload_segment(columns, n)


def test_boundary_values_fractional_bounds_and_negatives(engine):
    lo, hi = -40, 100
    pat = np.array([lo - 1, lo, hi - 1, hi, 99, 100, 101, -100, 0, -1], dtype=np.int64)
    vals = np.resize(pat, 200)
    ranges = [(None, lo, hi), (None, 99.5, 100.5), (None, -INF, -40), (None, -0.5, 0.5), (None, 100, INF), (None, -100.5, -99.5)]
    s = _upload(engine, {"v": {"type": N.COL_I64, "values": vals}}, 200)
    res, _ = run(engine, [s], [rng_agg("r", "v", ranges)])
    s.close()
    bks = RR.buckets(ranges)
    masks = RR.doc_masks(vals, bks, 200)
    check_buckets(res.to_dict()["r"], bks, masks)
    by = {(b[2], b[3]): int(m.sum()) for b, m in zip(bks, masks)}
    assert by[(-40.0, 100.0)] == 100 and by[(99.5, 100.5)] == 40 and by[(-0.5, 0.5)] == 20  # {lo, hi-1, 99, 0, -1}, {hi, 100}, {0}


def test_long_values_compare_as_doubles_past_2_53(engine):
    big = 1 << 53
    vals = np.array([big + 1, big + 3, -(big + 3), big + 4, big + 5, -(big + 1), 0, (1 << 63) - 1, -(1 << 63)], dtype=np.int64)
    cut = float(big + 4)
    ranges = [(None, cut, INF), (None, -INF, cut), (None, -cut, cut), (None, -INF, -cut), (None, 9.3e18, INF), (None, -INF, -9.3e18)]
    s = _upload(engine, {"v": {"type": N.COL_I64, "values": vals}}, len(vals))
    res, _ = run(engine, [s], [rng_agg("r", "v", ranges)])
    s.close()
    bks = RR.buckets(ranges)
    masks = RR.doc_masks(vals, bks, len(vals))
    check_buckets(res.to_dict()["r"], bks, masks)
    m = {(b[2], b[3]): mk for b, mk in zip(bks, masks)}
    assert m[(cut, INF)].tolist() == [False, True, False, True, True, False, False, True, False]  # (double)(2^53+3) = 2^53+4
    assert m[(-INF, -cut)].tolist()[2] is False and m[(-cut, cut)].tolist()[2] is True            # -(2^53+3) -> -(2^53+4)


@pytest.mark.parametrize("nr", [1, 64])
def test_one_and_sixty_four_ranges(engine, seg, cols, nr):
    ranges = [(None, -INF, INF)] if nr == 1 else [(None, 15.625 * k, 15.625 * (k + 1)) for k in range(64)]
    res, _ = run(engine, [seg], [rng_agg("r", "response_time_ms", ranges, [AB.max("m").field("bytes")])])
    got = res.to_dict()["r"]
    bks = RR.buckets(ranges)
    masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
    check_buckets(got, bks, masks)
    check_metrics(got, masks, [("m", N.AGG_MAX, cols["bytes"]["values"], None)])
    assert len(got["buckets"]) == nr and got["buckets"][-1]["doc_count"] > 0  # (bit 63 is used)


def test_refused_shapes_stay_on_the_cpu_path(engine):
    ok = lambda: AB.range("r").field("response_time_ms").addRange(0, 100)  # noqa: E731
    many = AB.range("r").field("response_time_ms")
    for k in range(65):
        many.addRange(k, k + 1)
    for aggs in ([many], [AB.terms("t").field("status").subAggregation(ok())],
                 [AB.filter("f", QB.termQuery("status", 200)).subAggregation(ok())],
                 [ok().subAggregation(AB.cardinality("c").field("bytes"))]):
        with pytest.raises(N.UnsupportedOnGpu):
            engine.plan(aggs)
    with pytest.raises(N.EsGpuError) as e:
        engine.plan([AB.range("r").field("response_time_ms")])
    assert e.value.code == N.ERR_INVALID
    p = engine.plan([ok()])
    assert p.shard_mergeable()
    p.close()


# ---- field layouts of the range field ------------------------------------------------------------------------------
def test_sparse_range_field_counts_only_present_docs(engine, cols):
    rng = np.random.default_rng(11)
    pres = rng.random(NDOCS) < 0.6
    pres[-17:] = np.arange(17) % 2 == 0
    vals = cols["response_time_ms"]["values"].copy()
    vals[~pres] = 77  # stored values under absent docs are not values
    c = {"rt": {"type": N.COL_I64, "values": vals, "present": bits_from_mask(pres)}, "bytes": cols["bytes"]}
    ranges = [(None, -INF, INF), (None, 0, 100), (None, 77, 78)]
    s = _upload(engine, c, NDOCS)
    res, _ = run(engine, [s], [rng_agg("r", "rt", ranges, [AB.sum("b").field("bytes")])])
    s.close()
    got = res.to_dict()["r"]
    bks = RR.buckets(ranges)
    masks = RR.doc_masks(vals, bks, NDOCS, present=pres)
    check_buckets(got, bks, masks)
    check_metrics(got, masks, [("b", N.AGG_SUM, cols["bytes"]["values"], None)])
    assert got["buckets"][0]["doc_count"] == int(pres.sum()) < NDOCS


def test_multi_valued_range_field_counts_a_doc_once_per_range(engine, cols):
    rng = np.random.default_rng(5)
    cnt = rng.integers(0, 5, size=NDOCS)
    col = csr_sorted(cnt, rng.integers(0, 1000, size=cnt.sum()), np.int64, N.COL_I64)
    ranges = [(None, 0, 500), (None, 500, 1000), (None, 250, 750), (None, -INF, INF), (None, 990, INF)]
    c = {"codes": col, "bytes": cols["bytes"]}
    s = _upload(engine, c, NDOCS)
    res, stats = run(engine, [s], [rng_agg("r", "codes", ranges, [AB.stats("b").field("bytes")])])
    s.close()
    got = res.to_dict()["r"]
    bks = RR.buckets(ranges)
    masks = RR.doc_masks(col["values"], bks, NDOCS, offsets=col["offsets"])
    check_buckets(got, bks, masks)
    check_metrics(got, masks, [("b", N.AGG_STATS, cols["bytes"]["values"], None)])
    vm = RR.value_masks(col["values"], bks)
    by = {(b[2], b[3]): k for k, b in enumerate(bks)}
    k0, k1, kall = by[(0.0, 500.0)], by[(500.0, 1000.0)], by[(-INF, INF)]
    assert vm[k0].sum() > masks[k0].sum()                      # two values in one range count once
    assert (masks[k0] & masks[k1]).sum() > 0                   # values in two ranges count in both
    assert masks[kall].sum() == int((cnt > 0).sum()) < NDOCS   # a doc without a value is in no range
    assert stats[2] == 11


def test_double_range_field_with_fractional_bounds(engine, seg, cols):
    ranges = [(None, -INF, 250.25), (None, 250.25, 750.75), (None, 750.75, INF), (None, 0.5, 999.5), (None, -0.0, 0.0)]
    res, _ = run(engine, [seg], [rng_agg("p", "price", ranges, [AB.count("n").field("bytes")])])
    got = res.to_dict()["p"]
    bks = RR.buckets(ranges)
    masks = RR.doc_masks(cols["price"]["values"], bks, NDOCS)
    check_buckets(got, bks, masks)
    check_metrics(got, masks, [("n", N.AGG_VALUE_COUNT, cols["bytes"]["values"], None)])
    assert got["buckets"][0]["key"] == "*-250.25" and got["buckets"][0]["doc_count"] > 0


def test_double_special_values_in_the_range_field(engine):
    vals = np.array([math.nan, -0.0, 0.0, -INF, INF, 1e-300, -1e-300, 5.0, math.nan, 2.5], dtype=np.float64)
    ranges = [(None, -INF, INF), (None, 0.0, 5.0), (None, -INF, 0.0), (None, 5.0, INF), (None, -1.0, -0.0)]
    s = _upload(engine, {"v": {"type": N.COL_F64, "values": vals}}, len(vals))
    res, _ = run(engine, [s], [rng_agg("r", "v", ranges)])
    s.close()
    bks = RR.buckets(ranges)
    masks = RR.doc_masks(vals, bks, len(vals))
    check_buckets(res.to_dict()["r"], bks, masks)
    m = {(b[2], b[3]): int(mk.sum()) for b, mk in zip(bks, masks)}
    assert m[(-INF, INF)] == 7 and m[(0.0, 5.0)] == 4 and m[(-INF, 0.0)] == 2  # NaN and +inf (not < +inf) are in no range; both zeros >= 0.0


# ---- metric children -----------------------------------------------------------------------------------------------
def test_stats_and_sum_children_on_bytes(engine, seg, cols):
    subs = [AB.stats("b").field("bytes"), AB.sum("total").field("bytes")]
    res, stats = run(engine, [seg], [rng_agg("lat", "response_time_ms", LATENCY, subs)])
    got = res.to_dict()["lat"]
    bks = RR.buckets(LATENCY)
    masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
    check_buckets(got, bks, masks)
    bv = cols["bytes"]["values"]
    check_metrics(got, masks, [("b", N.AGG_STATS, bv, None), ("total", N.AGG_SUM, bv, None)])
    assert stats[2] == 11 and stats[1] == 16 * NDOCS  # both leaves share one pipeline: one pass over two columns


def test_children_against_the_filter_twin(engine, seg, cols):
    """extended_stats on the range field itself, stats on bytes and avg on price (three metric fields: three pipelines),
    rendered values included, against five filter aggregations run through the oracle"""
    subs = [AB.extendedStats("x").field("response_time_ms"), AB.stats("b").field("bytes"), AB.avg("a").field("price")]
    res, _ = run(engine, [seg], [rng_agg("lat", "response_time_ms", CLASSES, subs)])
    want = O.run([(cols, NDOCS)], RR.filter_twin("response_time_ms", CLASSES, subs))
    got = reduce([res]).to_dict()["lat"]
    assert [b["key"] for b in got["buckets"]] == ["fast", "0.0-1000.0", "100.0-500.0", "slow"]
    check_twin(got, want["reduced"], 4, exact=False)
    for i, b in enumerate(got["buckets"]):  # the integer-valued leaves are bit-exact
        w = want["reduced"]["f%d" % i]
        assert b["x"]["_internal"] == w["x"]["_internal"] and b["b"]["sum"] == w["b"]["sum"]


def test_avg_min_max_on_a_double_field(engine, seg, cols):
    subs = [AB.avg("a").field("price"), AB.min("lo").field("price"), AB.max("hi").field("price")]
    res, _ = run(engine, [seg], [rng_agg("lat", "response_time_ms", CLASSES, subs)])
    got = res.to_dict()["lat"]
    bks = RR.buckets(CLASSES)
    masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
    pv = cols["price"]["values"]
    check_buckets(got, bks, masks)
    check_metrics(got, masks, [("a", N.AGG_AVG, pv, None), ("lo", N.AGG_MIN, pv, None), ("hi", N.AGG_MAX, pv, None)], exact=False)
    want = O.run([(cols, NDOCS)], RR.filter_twin("response_time_ms", CLASSES, subs[:1]))
    for i, b in enumerate(got["buckets"]):
        assert_same(b["a"], want["reduced"]["f%d" % i]["a"], "a[%d]" % i, exact_floats=False)


def test_sparse_metric_field_and_value_count(engine, cols):
    rng = np.random.default_rng(3)
    pres = rng.random(NDOCS) < 0.5
    pres[:64] = False  # a whole bitset word of docs in a range without a metric value
    c = {"response_time_ms": cols["response_time_ms"],
         "sz": {"type": N.COL_I64, "values": cols["bytes"]["values"], "present": bits_from_mask(pres)}}
    subs = [AB.count("n").field("sz"), AB.stats("s").field("sz"), AB.min("lo").field("sz")]
    ranges = CLASSES + [(None, 995, 1000)]
    s = _upload(engine, c, NDOCS)
    res, _ = run(engine, [s], [rng_agg("lat", "response_time_ms", ranges, subs)])
    s.close()
    got = res.to_dict()["lat"]
    bks = RR.buckets(ranges)
    masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
    check_buckets(got, bks, masks)
    bv = cols["bytes"]["values"]
    check_metrics(got, masks, [("n", N.AGG_VALUE_COUNT, bv, pres), ("s", N.AGG_STATS, bv, pres), ("lo", N.AGG_MIN, bv, pres)])
    assert all(b["n"]["value"] < b["doc_count"] for b in got["buckets"] if b["doc_count"] > 100)


def test_refused_metric_fields(engine, cols):
    rng = np.random.default_rng(9)
    cnt = rng.integers(0, 3, size=1000)
    c = {"rt": {"type": N.COL_I64, "values": cols["response_time_ms"]["values"][:1000]},
         "multi": csr_sorted(cnt, rng.integers(0, 9, size=cnt.sum()), np.int64, N.COL_I64),
         "kw": {"type": N.COL_ORD_U32, "values": np.zeros(1000, np.uint32), "terms": ["a"]},
         "h": {"type": N.COL_U64, "values": np.arange(1000, dtype=np.uint64)}}
    s = _upload(engine, c, 1000)
    for aggs in ([rng_agg("r", "rt", CLASSES, [AB.stats("m").field("multi")])], [rng_agg("r", "rt", CLASSES, [AB.count("m").field("multi")])],
                 [rng_agg("r", "rt", CLASSES, [AB.count("m").field("kw")])], [rng_agg("r", "kw", CLASSES)], [rng_agg("r", "h", CLASSES)]):
        plan = engine.plan(aggs)
        with pytest.raises(N.UnsupportedOnGpu):
            plan.collect(s)
        plan.close()
    s.close()


# ---- filters -------------------------------------------------------------------------------------------------------
SUBS = [AB.stats("b").field("bytes")]


def test_term_and_range_query_filters(engine, seg, cols):
    filters = [QB.termQuery("status", 200), QB.rangeQuery("bytes").gte(1000).lt(500000)]
    res, stats = run(engine, [seg], [rng_agg("lat", "response_time_ms", CLASSES, SUBS)], filters=filters)
    want = O.run([(cols, NDOCS)], RR.filter_twin("response_time_ms", CLASSES, SUBS), filters=filters)
    got = res.to_dict()["lat"]
    check_twin(got, want["reduced"], 4)
    acc = (cols["status"]["values"] == 200) & (cols["bytes"]["values"] >= 1000) & (cols["bytes"]["values"] < 500000)
    bks = RR.buckets(CLASSES)
    check_buckets(got, bks, RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS, accept=acc))
    assert 0 < got["buckets"][1]["doc_count"] == int(acc.sum()) < NDOCS and stats[2] == 11


def test_accept_bits(engine, seg, cols):
    acc = np.random.default_rng(21).random(NDOCS) < 0.3
    acc[-17:] = True
    bits = bits_from_mask(acc)
    res, _ = run(engine, [seg], [rng_agg("lat", "response_time_ms", CLASSES, SUBS)], accept=[bits])
    got = res.to_dict()["lat"]
    bks = RR.buckets(CLASSES)
    masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS, accept=acc)
    check_buckets(got, bks, masks)
    check_metrics(got, masks, [("b", N.AGG_STATS, cols["bytes"]["values"], None)])
    want = O.run([(cols, NDOCS)], RR.filter_twin("response_time_ms", CLASSES, SUBS), accept=[bits])
    check_twin(got, want["reduced"], 4)


def test_more_than_four_clauses(engine, seg, cols):
    filters = [QB.rangeQuery("bytes").gte(500), QB.rangeQuery("bytes").lt(900000), QB.rangeQuery("response_time_ms").lt(990),
               QB.rangeQuery("price").gte(1.5), QB.rangeQuery("price").lt(998.0), QB.termQuery("status", 200)]
    res, _ = run(engine, [seg], [rng_agg("lat", "response_time_ms", CLASSES, SUBS)], filters=filters)
    want = O.run([(cols, NDOCS)], RR.filter_twin("response_time_ms", CLASSES, SUBS), filters=filters)
    got = res.to_dict()["lat"]
    check_twin(got, want["reduced"], 4)
    assert 0 < got["buckets"][1]["doc_count"] < NDOCS


# ---- segments and plans --------------------------------------------------------------------------------------------
def test_two_segments_one_without_the_field(engine, cols):
    n2 = 5000
    other = {"bytes": {"type": N.COL_I64, "values": cols["bytes"]["values"][:n2]}}
    a = _upload(engine, {k: cols[k] for k in ("response_time_ms", "bytes")}, NDOCS)
    b = _upload(engine, other, n2)
    for order in ((a, b), (b, a)):
        res, _ = run(engine, list(order), [rng_agg("lat", "response_time_ms", LATENCY, SUBS)])
        got = res.to_dict()["lat"]
        bks = RR.buckets(LATENCY)
        masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
        check_buckets(got, bks, masks)
        check_metrics(got, masks, [("b", N.AGG_STATS, cols["bytes"]["values"], None)])
    a.close()
    b.close()


def test_plan_without_a_collect_builds_empty_buckets(engine):
    subs = [AB.stats("b").field("bytes"), AB.max("m").field("price")]
    plan = engine.plan([rng_agg("lat", "response_time_ms", LATENCY, subs, keyed=True)])
    res = plan.build()
    plan.close()
    got = res.to_dict()["lat"]
    assert [b["key"] for b in got["buckets"]] == [k for _i, k, _lo, _hi in RR.buckets(LATENCY)]
    for b in got["buckets"]:
        assert b["doc_count"] == 0 and b["b"]["count"] == 0 and b["b"]["min"] is None and b["m"]["value"] == -INF
    assert res.to_xcontent().startswith('{"lat":{"buckets":{"*-100.0":{"to":100.0,"to_as_string":"100.0","doc_count":0,'
                                        '"b":{"count":0,"min":null,"max":null,"avg":null,"sum":null},"m":{"value":null}},')


def test_reset_and_reuse_and_two_shards_reduced(engine, seg, cols):
    cols1 = synthetic_columns(("response_time_ms", "bytes"), 9000, shard=1)
    seg1 = engine.synthetic_segment(9000, fields=("response_time_ms", "bytes"), shard=1)
    aggs = [rng_agg("lat", "response_time_ms", LATENCY, SUBS)]
    bks = RR.buckets(LATENCY)
    m0 = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
    m1 = RR.doc_masks(cols1["response_time_ms"]["values"], bks, 9000)
    plan = engine.plan(aggs)
    plan.collect(seg)
    r0 = plan.build()
    check_buckets(r0.to_dict()["lat"], bks, m0)
    plan.reset()
    plan.collect(seg1)
    r1 = plan.build()
    check_buckets(r1.to_dict()["lat"], bks, m1)
    check_metrics(r1.to_dict()["lat"], m1, [("b", N.AGG_STATS, cols1["bytes"]["values"], None)])
    plan.reset()
    plan.collect(seg)
    assert plan.build().to_dict() == r0.to_dict()
    plan.close()
    red = reduce([r0, r1]).to_dict()["lat"]
    both = np.concatenate([m0, m1], axis=1)
    check_buckets(red, bks, both)
    check_metrics(red, both, [("b", N.AGG_STATS, np.concatenate([cols["bytes"]["values"], cols1["bytes"]["values"]]), None)])
    seg1.close()


# ---- layouts -------------------------------------------------------------------------------------------------------
def test_layouts_and_released_wide_columns_give_the_same_result(engine, cols):
    s = engine.synthetic_segment(NDOCS, fields=FIELDS)
    aggs = [rng_agg("lat", "response_time_ms", LATENCY, [AB.stats("b").field("bytes"), AB.extendedStats("x").field("response_time_ms")])]
    try:
        engine.set_option("compact_columns", 0)
        wide = run(engine, [s], aggs)[0].to_dict()
        engine.set_option("compact_columns", 1)
        compact = run(engine, [s], aggs)[0].to_dict()
    finally:
        engine.set_option("compact_columns", 1)
    assert compact == wide
    bks = RR.buckets(LATENCY)
    masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
    check_buckets(wide["lat"], bks, masks)
    check_metrics(wide["lat"], masks, [("b", N.AGG_STATS, cols["bytes"]["values"], None)])
    # a filtered request builds the compact copies of the two long columns; their upload-width values are then released
    flt = [QB.rangeQuery("response_time_ms").gte(0), QB.rangeQuery("bytes").gte(0)]
    run(engine, [s], [AB.stats("all").field("price")], filters=flt)
    assert s.release_wide() >= 16 * NDOCS
    assert run(engine, [s], aggs)[0].to_dict() == wide
    s.close()


# ---- tiny segments -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 8191, 8193])
def test_tiny_segments(engine, n):
    f = ("response_time_ms", "bytes")
    c = synthetic_columns(f, n, shard=2)
    s = engine.synthetic_segment(n, fields=f, shard=2)
    res, _ = run(engine, [s], [rng_agg("lat", "response_time_ms", LATENCY, SUBS)])
    s.close()
    got = res.to_dict()["lat"]
    bks = RR.buckets(LATENCY)
    masks = RR.doc_masks(c["response_time_ms"]["values"], bks, n)
    check_buckets(got, bks, masks)
    check_metrics(got, masks, [("b", N.AGG_STATS, c["bytes"]["values"], None)])


# ---- stats and rendering -------------------------------------------------------------------------------------------
def test_stream_and_xcontent_rendering(engine, seg, cols):
    subs = [AB.stats("b").field("bytes"), AB.max("m").field("bytes")]
    res, stats = run(engine, [seg], [rng_agg("lat", "response_time_ms", CLASSES, subs, keyed=True)])
    assert stats[2] == 11 and stats[0] > 0
    dec = RR.decode_stream(res.to_stream())
    assert len(dec) == 1 and dec[0]["stream_type"] == "range" and dec[0]["name"] == "lat" and dec[0]["keyed"] is True
    assert dec[0]["formatter"] == ("raw",)
    bks = RR.buckets(CLASSES)
    masks = RR.doc_masks(cols["response_time_ms"]["values"], bks, NDOCS)
    for d, (_i, key, lo, hi), m in zip(dec[0]["buckets"], bks, masks):
        cnt, s, mn, mx = RR.metric(m, cols["bytes"]["values"])
        assert (d["key"], d["from"], d["to"], d["doc_count"]) == (key, lo, hi, int(m.sum()))
        st, mxa = d["aggs"]
        assert (st["stream_type"], st["count"], st["sum"], st["min"], st["max"]) == ("stats", cnt, s, mn, mx)
        assert (mxa["stream_type"], mxa["value"]) == ("max", mx)
    small = np.array([5, 150, 150, 700, 99], dtype=np.int64)
    sz = np.array([10, 20, 30, 40, 50], dtype=np.int64)
    s = _upload(engine, {"rt": {"type": N.COL_I64, "values": small}, "sz": {"type": N.COL_I64, "values": sz}}, 5)
    r2, _ = run(engine, [s], [rng_agg("lat", "rt", [("fast", -INF, 100), (None, 100, 500.5), (None, 1000, INF)],
                                     [AB.avg("a").field("sz"), AB.max("m").field("sz")])])
    s.close()
    assert r2.to_xcontent() == (
        '{"lat":{"buckets":[{"key":"fast","to":100.0,"to_as_string":"100.0","doc_count":2,"a":{"value":30.0},"m":{"value":50.0}},'
        '{"key":"100.0-500.5","from":100.0,"from_as_string":"100.0","to":500.5,"to_as_string":"500.5","doc_count":2,'
        '"a":{"value":25.0},"m":{"value":30.0}},'
        '{"key":"1000.0-*","from":1000.0,"from_as_string":"1000.0","doc_count":0,"a":{"value":null},"m":{"value":null}}]}}')
