"""Ranked terms (collect path 10): an unfiltered top-level terms aggregation in count order over a shard's only
segment collects its sub-aggregations for the top shard_size terms alone -- the winners and every term's doc_count are
known from the segment's cached term counts.  Every case compares the shard result and the reduced result with the CPU
oracle (helpers.assert_same: counts, keys and the integer-valued metric's sums bit-exact), and with the same request
collected over every term (context option ranked_terms = 0, path 2).

Whole-shard shapes: 31,461,003 synthetic docs give every workgroup 5 or 6 zone blocks, i.e. more than one group of 4
(test_gpu_zone_block_carry.py).  Edge cases upload at most 200,000 docs.
"""
import contextlib

import numpy as np
import pytest

import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Order, QueryBuilders as QB
from elasticsearch_amd import _native as N
from elasticsearch_amd import build_reduce, reduce
from helpers import assert_same, bits_from_mask, synthetic_columns

pytestmark = pytest.mark.gpu

N_DOCS = 31_461_000 + 3
FIELDS = ("host", "@timestamp", "response_time_ms")
T0 = 1_441_065_600_000
_cols = {}


def columns(jitter):
    """host copies of the synthetic shard at a timestamp displacement, generated once per module run"""
    if jitter not in _cols:
        _cols[jitter] = synthetic_columns(FIELDS, N_DOCS, ts_jitter_ms=jitter)
    return _cols[jitter]


def north_star(interval="1h", leaf=None, size=10, shard_size=None, order=None):
    t = AB.terms("hosts").field("host").size(size)
    if shard_size is not None:
        t = t.shardSize(shard_size)
    if order is not None:
        t = t.order(order)
    leaf = leaf if leaf is not None else AB.stats("rt").field("response_time_ms")
    return [t.subAggregation(AB.dateHistogram("per_hour").field("@timestamp").interval(interval).subAggregation(leaf))]


@contextlib.contextmanager
def ranked(engine, on):
    engine.set_option("ranked_terms", 1 if on else 0)
    try:
        yield
    finally:
        engine.set_option("ranked_terms", 1)


def run_once(engine, seg, aggs, **kw):
    """(shard dict, reduced dict, collect path) of one single-segment request"""
    plan = engine.plan(aggs, **kw)
    plan.collect(seg)
    path = plan.last_collect_stats()[2]
    res = plan.build()
    out = res.to_dict(), reduce([res]).to_dict(), path
    plan.close()
    return out


def check(engine, aggs, n, cols=None, jitter=0, path=10):
    """the request over the synthetic shard (device-generated, or `cols` uploaded): the ranked collect against the
    oracle, and against the collect over every term"""
    host = cols if cols is not None else columns(jitter)
    want = O.run([(host, n)], aggs)
    seg = engine.upload_segment(cols, n) if cols is not None else engine.synthetic_segment(n, fields=FIELDS, ts_jitter_ms=jitter)
    shard, red, got_path = run_once(engine, seg, aggs)
    if path is not None:
        assert got_path == path
    assert_same(shard, want["shards"][0], "shard")
    assert_same(red, want["reduced"], "reduced")
    with ranked(engine, False):
        shard0, red0, path0 = run_once(engine, seg, aggs)
    assert path0 != 10
    if path == 10 and cols is None:
        assert path0 == 2
    assert_same(shard0, shard, "every term vs ranked")
    assert_same(red0, red, "every term vs ranked, reduced")
    seg.close()


# ---- whole-shard shapes ----
# time-sorted; +-1 h (multi-pass groups unless the window holds a block's keys); +-1 min
@pytest.mark.parametrize("jitter", [0, 3_600_000, 60_000])
def test_north_star(engine, jitter):
    check(engine, north_star(), N_DOCS, jitter=jitter)


def test_one_minute_interval(engine):
    """the window slides at nearly every block in the first tenth of the docs; the rest of the timestamps are drawn
    together 64-fold (test_gpu_zone_block_carry.test_one_minute_interval)"""
    ts = columns(0)["@timestamp"]["values"]
    cut = N_DOCS // 10
    cols = {f: dict(columns(0)[f]) for f in FIELDS}
    cols["@timestamp"]["values"] = np.concatenate([ts[:cut], ts[cut] + (ts[cut:] - ts[cut]) // 64])
    check(engine, north_star("1m"), N_DOCS, cols=cols)


def test_avg_leaf(engine):
    check(engine, north_star(leaf=AB.avg("rt").field("response_time_ms")), N_DOCS)


# ---- edge cases ----
def small_shard(n, ords, nterms, seed=3, span_h=30, ts_present=None):
    rng = np.random.default_rng(seed)
    cols = {
        "host": {"type": N.COL_ORD_U32, "values": np.asarray(ords, dtype=np.uint32), "terms": ["h%04d" % i for i in range(nterms)]},
        "@timestamp": {"type": N.COL_I64, "values": np.sort(rng.integers(T0, T0 + span_h * 3_600_000, size=n)).astype(np.int64)},
        "response_time_ms": {"type": N.COL_I64, "values": rng.integers(1, 30_000, size=n).astype(np.int64)},
    }
    if ts_present is not None:
        cols["@timestamp"]["present"] = bits_from_mask(ts_present)
    return cols


def test_counts_tied_across_the_boundary(engine):
    """ranks K-1, K and K+1 hold equal counts (K = shard_size = 25): of the three only the smallest ordinal is collected"""
    nterms, K = 60, 25
    rng = np.random.default_rng(11)
    counts = np.full(nterms, 1_000)
    order = rng.permutation(nterms)              # order[r]: the ordinal of rank r, up to the ties
    counts[order[:K - 1]] = 5_000 - 10 * np.arange(K - 1)
    counts[order[K - 1:K + 2]] = 2_000           # the tie: one of the three is in the top K
    ords = rng.permutation(np.repeat(np.arange(nterms), counts))
    n = len(ords)
    assert n <= 200_000 and (counts > 2_000).sum() == K - 1 and (counts == 2_000).sum() == 3
    check(engine, north_star(size=10, shard_size=K), n, cols=small_shard(n, ords, nterms))


def test_fewer_terms_than_shard_size(engine):
    n = 120_001
    ords = np.random.default_rng(5).integers(0, 7, size=n)
    check(engine, north_star(), n, cols=small_shard(n, ords, 7))


def test_every_doc_on_one_term(engine):
    n = 100_003
    check(engine, north_star(), n, cols=small_shard(n, np.full(n, 3), 12))


def test_missing_ordinals(engine):
    n = 200_000
    rng = np.random.default_rng(7)
    ords = np.minimum(rng.zipf(1.2, size=n) - 1, 299).astype(np.uint32)
    ords[rng.random(n) < 0.15] = 0xFFFFFFFF
    check(engine, north_star(), n, cols=small_shard(n, ords, 300))


def test_missing_ordinals_and_blocks_without_a_timestamp(engine):
    """15 % of the ordinals missing, and timestamps missing in runs that hold whole zone blocks of 8,192 docs: the
    outer counts of such a request are counted per doc, so the request is collected over every term"""
    n = 200_000
    rng = np.random.default_rng(8)
    ords = np.minimum(rng.zipf(1.2, size=n) - 1, 299).astype(np.uint32)
    ords[rng.random(n) < 0.15] = 0xFFFFFFFF
    present = np.repeat(rng.random(-(-n // 20_011)) >= 0.3, 20_011)[:n]
    present &= rng.random(n) >= 0.015
    assert not present[: (n // 8192) * 8192].reshape(-1, 8192).any(axis=1).all()  # whole blocks missing
    check(engine, north_star(), n, cols=small_shard(n, ords, 300, ts_present=present), path=None)


def test_size_3_shard_size_40(engine):
    n = 180_000
    ords = np.minimum(np.random.default_rng(9).zipf(1.1, size=n) - 1, 499)
    check(engine, north_star(size=3, shard_size=40), n, cols=small_shard(n, ords, 500))


# ---- fallback: a second segment ----
def test_second_segment_falls_back(engine):
    n = 150_000
    rng = np.random.default_rng(21)
    parts = []
    for k in range(2):  # the two segments rank their terms differently
        ords = (np.minimum(rng.zipf(1.2, size=n) - 1, 199) * (7 if k else 1) + 13 * k) % 200
        parts.append(small_shard(n, ords, 200, seed=30 + k))
    one = {f: dict(parts[0][f], values=np.concatenate([p[f]["values"] for p in parts])) for f in parts[0]}
    aggs = north_star()
    want = O.run([(one, 2 * n)], aggs)
    want1 = O.run([(parts[0], n)], aggs)
    segs = [engine.upload_segment(p, n) for p in parts]
    plan = engine.plan(aggs)
    plan.collect(segs[0])
    assert plan.last_collect_stats()[2] == 10 and plan.deferred_segments() == 1
    plan.collect(segs[1])
    assert plan.last_collect_stats()[2] != 10
    res = plan.build()
    assert_same(res.to_dict(), want["shards"][0], "two segments")
    assert_same(reduce([res]).to_dict(), want["reduced"], "two segments reduced")
    plan.reset()
    assert plan.deferred_segments() == 0
    # the plan stays off the ranked path from its next request's first segment on
    plan.collect(segs[0])
    assert plan.last_collect_stats()[2] != 10 and plan.deferred_segments() == 0
    assert_same(plan.build().to_dict(), want1["shards"][0], "third request")
    plan.close()
    # a plan that only ever sees one segment per request takes the path again after its reset
    plan = engine.plan(aggs)
    for _ in range(2):
        plan.collect(segs[0])
        assert plan.last_collect_stats()[2] == 10
        assert_same(plan.build().to_dict(), want1["shards"][0], "single segment")
        plan.reset()
        assert plan.deferred_segments() == 0
    plan.close()
    for s in segs:
        s.close()


def test_sticky_fallback_reports_the_window_path_on_a_whole_shard(engine):
    """after the fallback, a whole-shard request on that plan reports path 2 from its first segment"""
    n = 2_000_003
    seg = engine.synthetic_segment(n, fields=FIELDS)
    seg2 = engine.synthetic_segment(n, fields=FIELDS, shard=1)
    plan = engine.plan(north_star())
    plan.collect(seg)
    assert plan.last_collect_stats()[2] == 10
    plan.collect(seg2)
    plan.reset()
    plan.collect(seg)
    assert plan.last_collect_stats()[2] == 2
    want = O.run([(synthetic_columns(FIELDS, n), n)], north_star())
    assert_same(plan.build().to_dict(), want["shards"][0], "shard")
    plan.close()
    seg.close()
    seg2.close()


# ---- ineligible requests ----
def test_ineligible_requests_keep_their_path(engine):
    n = 200_000
    rng = np.random.default_rng(13)
    ords = np.minimum(rng.zipf(1.2, size=n) - 1, 99)
    cols = small_shard(n, ords, 100)
    seg = engine.upload_segment(cols, n)
    # a request filter
    flt = [QB.rangeQuery("response_time_ms").gte(100)]
    want = O.run([(cols, n)], north_star(), filters=flt)
    shard, _, path = run_once(engine, seg, north_star(), filters=flt)
    assert path != 10
    assert_same(shard, want["shards"][0], "filter")
    # accept bits
    mask = rng.random(n) < 0.8
    want = O.run([(cols, n)], north_star(), accept=[bits_from_mask(mask)])
    plan = engine.plan(north_star())
    plan.collect(seg, accept_bits=bits_from_mask(mask))
    assert plan.last_collect_stats()[2] != 10 and plan.deferred_segments() == 0
    assert_same(plan.build().to_dict(), want["shards"][0], "accept bits")
    plan.close()
    # count ascending
    aggs = north_star(order=Order.count(True))
    want = O.run([(cols, n)], aggs)
    shard, _, path = run_once(engine, seg, aggs)
    assert path != 10
    assert_same(shard, want["shards"][0], "count ascending")
    seg.close()
    # a multi-valued host column
    counts = rng.integers(0, 3, size=n)
    vals = np.minimum(rng.zipf(1.2, size=int(counts.sum())) - 1, 99)
    doc = np.repeat(np.arange(n), counts)
    o = np.lexsort((vals, doc))
    doc, vals = doc[o], vals[o]
    keep = np.ones(len(vals), dtype=bool)
    keep[1:] = (doc[1:] != doc[:-1]) | (vals[1:] != vals[:-1])
    doc, vals = doc[keep], vals[keep]
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(doc, minlength=n), out=offs[1:])
    mcols = dict(cols, host={"type": N.COL_ORD_U32, "values": vals.astype(np.uint32), "offsets": offs, "terms": cols["host"]["terms"]})
    want = O.run([(mcols, n)], north_star())
    seg = engine.upload_segment(mcols, n)
    shard, _, path = run_once(engine, seg, north_star())
    assert path != 10
    assert_same(shard, want["shards"][0], "multi-valued")
    seg.close()


# ---- co-located reduce ----
def test_build_reduce_over_8_plans(engine):
    n, shards = 2_000_003, 8
    aggs = north_star()
    segs = [engine.synthetic_segment(n, fields=FIELDS, shard=s) for s in range(shards)]
    plans = [engine.plan(aggs, number_of_shards=shards) for _ in segs]
    for p, s in zip(plans, segs):
        p.collect(s)
        assert p.last_collect_stats()[2] == 10
    fused = build_reduce(plans).to_dict()
    for p, s in zip(plans, segs):
        p.reset()
        p.collect(s)
    plain = reduce([p.build() for p in plans]).to_dict()
    assert_same(fused, plain, "fused vs builds")
    want = O.run([(synthetic_columns(FIELDS, n, shard=s), n) for s in range(shards)], aggs, number_of_shards=shards)
    assert_same(fused, want["reduced"], "fused vs oracle")
    for p in plans:
        p.close()
    for s in segs:
        s.close()
