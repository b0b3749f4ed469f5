"""A date_histogram under a filters or a range aggregation on the GPU (collect path 13, esgpu_mask_hist.hip).

The reference never runs the code under test: bucket i's histogram subtree must equal the oracle's result for the same
date_histogram spec at top level with accept = bucket i's doc mask (tests/filters_ref.doc_masks / range_ref.doc_masks,
ANDed with the test's own accept bits; the query goes to the oracle as it goes to the plan).  That covers the other bucket
and overlapping buckets.  A bucket's doc_count is its mask's population -- docs without a timestamp included, which the
histogram leaves out.  Where the twin applies (N top-level filter{date_histogram} aggregations) it is compared too.
Counts and keys are exact, integer-valued sums exact, `price` within REL_TOL (helpers.assert_same).

Timestamps are crafted columns uploaded with engine.upload_segment; shards are at most 3 * 8192 + 17 docs.
"""
import copy
import json

import numpy as np
import pytest

import filters_ref as FR
import mask_hist_ref as MH
import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Order
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from helpers import assert_same, bits_from_mask, synthetic_columns
from test_gpu_multivalued import csr_sorted

pytestmark = pytest.mark.gpu

BLOCK = 8192
NDOCS = 3 * BLOCK + 17
FIELDS = ("status", "response_time_ms", "bytes", "price")
RT, TS = "response_time_ms", "@timestamp"
H = 3600000
T0 = 1441065600000  # 2015-09-01T00:00:00Z
CLASSES = [("c0", QB.rangeQuery(RT).lt(50)), ("c1", QB.rangeQuery(RT).gte(50).lt(100)), ("c2", QB.rangeQuery(RT).gte(100).lt(250)),
           ("c3", QB.rangeQuery(RT).gte(250).lt(500)), ("c4", QB.rangeQuery(RT).gte(500))]
MIXED = [("fast", QB.rangeQuery(RT).lt(100)), ("ok", QB.termQuery("status", 200)),
         ("big_ok", [QB.termQuery("status", 200), QB.rangeQuery("bytes").gte(100000)]), ("mid", QB.rangeQuery(RT).gte(50).lte(600))]
RANGES = [("lo", -np.inf, 100.0), ("mid", 50.0, 500.0), (None, 500.0, np.inf), ("empty", 300.0, 300.0)]  # overlapping, one empty
# the positions the kernel treats differently: inside a lane's four docs, a lane, a wave, a sweep, a round, a block
EDGES = (1, 3, 4, 255, 256, 1023, 1024, 2047, 2048, 8191, 8192, 8193)


# ---- columns ---------------------------------------------------------------------------------------------------------
def sorted_ts(n, edges, step=H, t0=T0):
    """[n] sorted timestamps whose key changes exactly at the doc positions `edges` (doc e is the first of a new key)"""
    key = np.searchsorted(np.asarray(sorted(edges)), np.arange(n), side="right")
    return (t0 + key * step + (np.arange(n) % 997) * 1000).astype(np.int64)


def with_ts(base, ts, n, present=None, fields=FIELDS):
    c = {f: {"type": base[f]["type"], "values": base[f]["values"][:n]} for f in fields}
    c[TS] = {"type": N.COL_I64, "values": np.ascontiguousarray(ts, dtype=np.int64)}
    if present is not None:
        c[TS]["present"] = bits_from_mask(present)
    return c


@pytest.fixture(scope="module")
def base():
    """the synthetic shard's non-time columns on the host: computed once, shared, never modified"""
    return synthetic_columns(FIELDS, NDOCS)


@pytest.fixture(scope="module")
def edge_cols(base):
    return with_ts(base, sorted_ts(NDOCS, EDGES + (NDOCS - 1,)), NDOCS)


@pytest.fixture(scope="module")
def edge_seg(engine, edge_cols):
    s = engine.upload_segment(edge_cols, NDOCS)
    yield s
    s.close()


# ---- builders --------------------------------------------------------------------------------------------------------
def dh(subs=(), name="h", interval="1h", **kw):
    h = AB.dateHistogram(name).field(TS).interval(interval)
    for k, v in kw.items():
        if k == "bounds":
            h.extendedBounds(*v)
        else:
            getattr(h, k)(v)
    for s in subs:
        h.subAggregation(copy.deepcopy(s))
    return h


def flt_root(filters, kids, other=None, name="f"):
    b = AB.filters(name)
    for key, q in filters:
        b.filter(key, q)
    if other:
        b.otherBucket(True)
    for k in kids:
        b.subAggregation(k)
    return b


def rng_root(ranges, kids, field=RT, name="r"):
    b = AB.range(name).field(field)
    for key, lo, hi in ranges:
        args = [] if key is None else [key]
        if np.isinf(lo) and np.isinf(hi):
            b.addRange(*args, -np.inf, np.inf)
        elif np.isinf(lo):
            b.addUnboundedTo(*args, hi)
        elif np.isinf(hi):
            b.addUnboundedFrom(*args, lo)
        else:
            b.addRange(*args, lo, hi)
    for k in kids:
        b.subAggregation(k)
    return b


def run(engine, segs, aggs, query=None, accept=None):
    plan = engine.plan(aggs, filters=query)
    for i, s in enumerate(segs):
        plan.collect(s, accept_bits=None if accept is None else bits_from_mask(accept[i]))
    res = plan.build()
    stats = plan.last_collect_stats()
    mergeable = plan.shard_mergeable()
    plan.close()
    assert mergeable
    return res, stats


def ts_bytes(cols, n, interval=H, offset=0):
    """what the statistics count for the timestamps: 8 bytes for every doc of a zone block that is not single-key, and
    the 16-byte zone-key words (numpy over the crafted column)"""
    ts = np.asarray(cols[TS]["values"])[:n]
    pres = np.ones(n, bool) if cols[TS].get("present") is None else FR.mask_from_bits(cols[TS]["present"], n)
    total = 0
    nb = (n + BLOCK - 1) // BLOCK
    for b in range(nb):
        sl = slice(b * BLOCK, min((b + 1) * BLOCK, n))
        k = np.unique((ts[sl][pres[sl]] - offset) // interval)
        if len(k) != 1:
            total += 8 * (sl.stop - sl.start)
    return total + 16 * nb


SINGLE = {"su": "sum", "mi": "min", "ma": "max", "vc": "count"}  # single-value leaves and the stats value they restate


def split_single(tree, twin="st"):
    """The oracle has no sum / min / max / value_count: a histogram bucket's leaves named in SINGLE are checked against
    the oracle's stats leaf `twin` of the same bucket (its _internal values: +-Infinity / 0.0 where no doc has a value)
    and taken out of the tree, which is then compared as it stands."""
    out = copy.deepcopy(tree)
    bks = out["buckets"].values() if isinstance(out["buckets"], dict) else out["buckets"]
    singles = []
    for b in bks:
        singles.append({k: b.pop(k) for k in list(b) if k in SINGLE})
    return out, singles


def check(engine, segs, root, masks, hists, query=None, accept=None, exact=True, keys=None, name=None, oracle_hists=None):
    """segs: [(segment, columns, n)].  root: the filters / range builder with the date_histogram children `hists` (and
    possibly metric children).  masks: per bucket, per segment, the [n] bool doc mask (accept included).  oracle_hists:
    the histograms the oracle runs when `hists` carry single-value leaves (split_single).  Returns the shard result's
    dict and the collect statistics."""
    res, stats = run(engine, [s for s, _c, _n in segs], [root], query, accept)
    name = name or root.name
    shard = res.to_dict()[name]
    red = reduce([res]).to_dict()[name]
    for d in (shard, red):
        assert len(d["buckets"]) == len(masks)
        if keys is not None:
            assert [b["key"] for b in d["buckets"]] == list(keys)
    for i, per_seg in enumerate(masks):
        dc = sum(int(m.sum()) for m in per_seg)
        assert shard["buckets"][i]["doc_count"] == dc and red["buckets"][i]["doc_count"] == dc, (i, dc)
        want = O.run([(c, n) for _s, c, n in segs], [copy.deepcopy(h) for h in (oracle_hists or hists)], filters=query,
                     accept=[bits_from_mask(m) for m in per_seg])
        for h in hists:
            pairs = [(red["buckets"][i][h.name], want["reduced"][h.name], "bucket[%d].%s" % (i, h.name))]
            if len(segs) == 1:
                pairs.append((shard["buckets"][i][h.name], want["shards"][0][h.name], "shard bucket[%d].%s" % (i, h.name)))
            for got, ref, path in pairs:
                if oracle_hists:
                    got, singles = split_single(got)
                    assert len(singles) == len(ref["buckets"]), path
                    for sg, rb in zip(singles, ref["buckets"]):
                        assert set(sg) == set(SINGLE), path
                        for leaf, stat in SINGLE.items():
                            assert_same(sg[leaf]["value"], rb["st"]["_internal"][stat], "%s.%s" % (path, leaf), exact)
                assert_same(got, ref, path, exact)
    assert stats[2] == 13
    return shard, stats


def flt_masks(segs, filters, other=False, accept=None):
    per = [MH.filters_masks(c, filters, n, other, None if accept is None else accept[i]) for i, (_s, c, n) in enumerate(segs)]
    return [[per[s][b] for s in range(len(segs))] for b in range(len(per[0]))]


def rng_masks(segs, ranges, field=RT, accept=None):
    per = [MH.range_masks(c, field, ranges, n, None if accept is None else accept[i]) for i, (_s, c, n) in enumerate(segs)]
    return per[0][0], [[per[s][1][b] for s in range(len(segs))] for b in range(len(per[0][0]))]


STATS = [AB.stats("s").field("bytes")]


# ---- key changes at every position the kernel treats differently ---------------------------------------------------------
@pytest.mark.parametrize("subs", [STATS, []], ids=["stats", "counts"])
def test_key_changes_at_every_edge_filters_partition_and_other(engine, edge_seg, edge_cols, subs):
    segs = [(edge_seg, edge_cols, NDOCS)]
    h = dh(subs)
    shard, stats = check(engine, segs, flt_root(CLASSES[:4], [h], other=True), flt_masks(segs, CLASSES[:4], True), [h],
                         keys=["c0", "c1", "c2", "c3", "_other_"])
    assert sum(b["doc_count"] for b in shard["buckets"]) == NDOCS
    assert sum(x["doc_count"] for b in shard["buckets"] for x in b["h"]["buckets"]) == NDOCS
    # one clause column and (stats) the metric column at 8 bytes, the timestamps of the multi-key blocks, the zone words
    assert stats[1] == (2 if subs else 1) * 8 * NDOCS + ts_bytes(edge_cols, NDOCS)
    assert ts_bytes(edge_cols, NDOCS) == 8 * (2 * BLOCK + 17) + 16 * 4  # blocks 0 (many edges), 1 (8193), 3 (the last doc)


@pytest.mark.parametrize("subs", [STATS, []], ids=["stats", "counts"])
def test_key_changes_at_every_edge_filters_overlapping(engine, edge_seg, edge_cols, subs):
    segs = [(edge_seg, edge_cols, NDOCS)]
    h = dh(subs)
    check(engine, segs, flt_root(MIXED, [h], other=True), flt_masks(segs, MIXED, True), [h])


@pytest.mark.parametrize("subs", [STATS, []], ids=["stats", "counts"])
def test_key_changes_at_every_edge_range(engine, edge_seg, edge_cols, subs):
    segs = [(edge_seg, edge_cols, NDOCS)]
    h = dh(subs)
    keys, masks = rng_masks(segs, RANGES)
    shard, stats = check(engine, segs, rng_root(RANGES, [h]), masks, [h], keys=keys)
    assert stats[1] == (2 if subs else 1) * 8 * NDOCS + ts_bytes(edge_cols, NDOCS)
    assert [b["h"]["buckets"] for b in shard["buckets"] if b["key"] == "empty"] == [[]]


def test_twin_of_five_filter_date_histograms(engine, edge_seg, edge_cols):
    subs = STATS
    res, _ = run(engine, [edge_seg], [flt_root(CLASSES, [dh(subs)])])
    want = O.run([(edge_cols, NDOCS)], FR.filter_twin([q for _k, q in CLASSES], [dh(subs)]))
    got = reduce([res]).to_dict()["f"]
    for i, b in enumerate(got["buckets"]):
        w = want["reduced"]["f%d" % i]
        assert b["doc_count"] == w["doc_count"]
        assert_same(b["h"], w["h"], "bucket[%d].h" % i)


# ---- one key, shuffled keys ----------------------------------------------------------------------------------------------
def test_one_key_for_the_whole_segment_reads_no_timestamp(engine, base):
    c = with_ts(base, sorted_ts(NDOCS, ()), NDOCS)
    s = engine.upload_segment(c, NDOCS)
    segs = [(s, c, NDOCS)]
    h = dh(STATS)
    shard, stats = check(engine, segs, flt_root(CLASSES, [h], other=True), flt_masks(segs, CLASSES, True), [h])
    keys, masks = rng_masks(segs, RANGES)
    _r, rstats = check(engine, segs, rng_root(RANGES, [h]), masks, [h], keys=keys)
    s.close()
    assert all(len(b["h"]["buckets"]) == (1 if b["doc_count"] else 0) for b in shard["buckets"])
    assert stats[1] == 16 * NDOCS + 16 * 4 and rstats[1] == 16 * NDOCS + 16 * 4  # no timestamp at all


def test_fully_shuffled_timestamps_over_700_keys(engine, base):
    rng = np.random.default_rng(17)
    ts = T0 + rng.integers(0, 700, size=NDOCS) * H + rng.integers(0, H, size=NDOCS)
    c = with_ts(base, ts, NDOCS)
    s = engine.upload_segment(c, NDOCS)
    segs = [(s, c, NDOCS)]
    for subs in (STATS, []):
        h = dh(subs)
        shard, stats = check(engine, segs, flt_root(MIXED, [h], other=True), flt_masks(segs, MIXED, True), [h])
        assert stats[1] == (3 + (1 if subs else 0)) * 8 * NDOCS + 8 * NDOCS + 16 * 4  # rt, status, bytes clauses; every timestamp
        keys, masks = rng_masks(segs, RANGES)
        check(engine, segs, rng_root(RANGES, [h]), masks, [h], keys=keys)
    s.close()
    assert max(len(b["h"]["buckets"]) for b in shard["buckets"]) > 600


# ---- missing timestamps ------------------------------------------------------------------------------------------------
def test_missing_timestamps_count_in_the_bucket_only(engine, base):
    rng = np.random.default_rng(23)
    pres = rng.random(NDOCS) < 0.7
    pres[BLOCK:2 * BLOCK] = False          # a block with no value at all
    pres[2 * BLOCK:2 * BLOCK + 64] = False  # a whole bitset word
    pres[-17:] = np.arange(17) % 2 == 0
    ts = sorted_ts(NDOCS, (5000, 2 * BLOCK + 100, 2 * BLOCK + 4000))
    ts[~pres] = T0 + 500 * H  # stored values under absent docs are not values
    c = with_ts(base, ts, NDOCS, present=pres)
    s = engine.upload_segment(c, NDOCS)
    segs = [(s, c, NDOCS)]
    for subs in (STATS, []):
        h = dh(subs)
        shard, stats = check(engine, segs, flt_root(CLASSES, [h], other=True), flt_masks(segs, CLASSES, True), [h])
        assert sum(b["doc_count"] for b in shard["buckets"]) == NDOCS
        assert sum(x["doc_count"] for b in shard["buckets"] for x in b["h"]["buckets"]) == int(pres.sum()) < NDOCS
        assert all(x["key"] < T0 + 10 * H for b in shard["buckets"] for x in b["h"]["buckets"])
        keys, masks = rng_masks(segs, RANGES)
        check(engine, segs, rng_root(RANGES, [h]), masks, [h], keys=keys)
    s.close()


# ---- metric kinds -------------------------------------------------------------------------------------------------------
KINDS = [("st", AB.stats), ("ex", AB.extendedStats), ("av", AB.avg), ("su", AB.sum), ("mi", AB.min), ("ma", AB.max), ("vc", AB.count)]


@pytest.mark.parametrize("field,exact", [("bytes", True), ("price", False), ("sz", True)])
def test_all_seven_metric_kinds(engine, base, field, exact):
    rng = np.random.default_rng(3)
    pres = rng.random(NDOCS) < 0.5
    pres[:64] = False  # a whole bitset word of docs in a bucket without a metric value
    c = with_ts(base, sorted_ts(NDOCS, (100, 5000, 9000, 20000)), NDOCS)
    c["sz"] = {"type": N.COL_I64, "values": base["bytes"]["values"], "present": bits_from_mask(pres)}
    s = engine.upload_segment(c, NDOCS)
    segs = [(s, c, NDOCS)]
    h = dh([mk(nm).field(field) for nm, mk in KINDS])
    oh = [dh([mk(nm).field(field) for nm, mk in KINDS[:3]])]  # (the oracle's kinds; the other four restate its stats)
    check(engine, segs, flt_root(MIXED, [h], other=True), flt_masks(segs, MIXED, True), [h], exact=exact, oracle_hists=oh)
    keys, masks = rng_masks(segs, RANGES)
    check(engine, segs, rng_root(RANGES, [h]), masks, [h], exact=exact, keys=keys, oracle_hists=oh)
    s.close()


def test_metric_field_turns_sparse_in_the_second_segment(engine, base):
    n2 = BLOCK + 300
    pres = np.random.default_rng(4).random(n2) < 0.6
    c1 = with_ts(base, sorted_ts(NDOCS, (7000, 16000)), NDOCS)
    c1["sz"] = {"type": N.COL_I64, "values": base["bytes"]["values"]}
    c2 = with_ts(base, sorted_ts(n2, (100,), t0=T0 + H), n2)
    c2["sz"] = {"type": N.COL_I64, "values": base["bytes"]["values"][:n2], "present": bits_from_mask(pres)}
    s1, s2 = engine.upload_segment(c1, NDOCS), engine.upload_segment(c2, n2)
    h = dh([AB.stats("s").field("sz"), AB.avg("a").field("sz")])
    for segs in ([(s1, c1, NDOCS), (s2, c2, n2)], [(s2, c2, n2), (s1, c1, NDOCS)]):
        check(engine, segs, flt_root(MIXED, [h], other=True), flt_masks(segs, MIXED, True), [h])
    s1.close()
    s2.close()


# ---- sixty-four buckets ---------------------------------------------------------------------------------------------
def test_sixty_four_buckets_every_doc_is_in(engine, base):
    c = with_ts(base, sorted_ts(NDOCS, tuple(range(800, NDOCS, 800))[:29]), NDOCS)  # 30 keys
    s = engine.upload_segment(c, NDOCS)
    segs = [(s, c, NDOCS)]
    filters = [("k%d" % k, QB.rangeQuery(RT).gte(-k)) for k in range(64)]
    h = dh([AB.avg("x").field("bytes")])
    shard, _ = check(engine, segs, flt_root(filters, [h]), flt_masks(segs, filters), [h])
    assert [b["doc_count"] for b in shard["buckets"]] == [NDOCS] * 64 and len(shard["buckets"][63]["h"]["buckets"]) == 30
    none = [("n%d" % k, QB.termQuery("status", 7000 + k)) for k in range(63)]
    shard, _ = check(engine, segs, flt_root(none, [h], other=True), flt_masks(segs, none, True), [h])
    s.close()
    assert [b["doc_count"] for b in shard["buckets"]] == [0] * 63 + [NDOCS]
    assert len(shard["buckets"][63]["h"]["buckets"]) == 30 and shard["buckets"][0]["h"]["buckets"] == []


# ---- roundings ----------------------------------------------------------------------------------------------------------
DAY = 24 * H
OCT25 = 1445731200000  # 2015-10-25T00:00:00Z: Europe/Berlin leaves DST at 01:00Z


@pytest.mark.parametrize("case", ["offset", "zone", "month", "berlin"])
def test_roundings(engine, base, case):
    n = 2 * BLOCK + 500
    rng = np.random.default_rng(31)
    if case == "offset":
        ts, h = sorted_ts(n, (3, 4000, 9000, 12000), step=2 * H), dh(STATS, offset="20m")
    elif case == "zone":
        ts, h = sorted_ts(n, (3, 4000, 9000, 12000), step=23 * H), dh(STATS, interval="1d", timeZone="+01:00")
    elif case == "month":
        ts, h = np.sort(T0 - 40 * DAY + rng.integers(0, 150 * DAY, size=n)), dh(STATS, interval="month")
    else:
        ts, h = np.sort(OCT25 - 2 * DAY + rng.integers(0, 5 * DAY, size=n)), dh(STATS, interval="1d", timeZone="Europe/Berlin")
    c = with_ts(base, ts, n)
    s = engine.upload_segment(c, n)
    segs = [(s, c, n)]
    shard, _ = check(engine, segs, flt_root(CLASSES[:3], [h], other=True), flt_masks(segs, CLASSES[:3], True), [h])
    keys, masks = rng_masks(segs, RANGES)
    check(engine, segs, rng_root(RANGES, [h]), masks, [h], keys=keys)
    s.close()
    got = shard["buckets"][3]["h"]["buckets"]
    assert len(got) >= 3 and all("key_as_string" in x for x in got)
    if case == "berlin":  # local midnights: 22:00Z before the change, 23:00Z after it (a 25-hour day between)
        assert [x["key"] - OCT25 for x in got][:4] == [-2 * DAY - 2 * H, -DAY - 2 * H, -2 * H, DAY - H]


# ---- histogram parameters --------------------------------------------------------------------------------------------
def test_histogram_parameters(engine, base):
    n = 2 * BLOCK + 9
    ts = sorted_ts(n, (40, 41, 9000, 9001, 9002, 16000))                # keys with 40, 1, 8959, 1, 1, 6998, 393 docs
    ts[9002:] += 3 * H                                                  # and a gap of three hours
    c = with_ts(base, ts, n)
    s = engine.upload_segment(c, n)
    segs = [(s, c, n)]
    masks = flt_masks(segs, MIXED, True)
    for kw in (dict(minDocCount=0, bounds=(T0 - 5 * H, T0 + 15 * H)), dict(minDocCount=0), dict(minDocCount=30),
               dict(minDocCount=1, order=Order.COUNT_DESC), dict(minDocCount=1, keyed=True),
               dict(minDocCount=0, bounds=(T0 - 2 * H, T0 + 12 * H), order=Order.COUNT_DESC, keyed=True)):
        h = dh(STATS, **kw)
        shard, _ = check(engine, segs, flt_root(MIXED, [h], other=True), masks, [h])
        red = reduce([run(engine, [s], [flt_root(MIXED, [h], other=True)])[0]]).to_dict()["f"]["buckets"][0]["h"]["buckets"]
        if kw.get("bounds") and not kw.get("keyed"):
            assert red[0]["key"] == kw["bounds"][0] and red[-1]["key"] == kw["bounds"][1] and red[0]["doc_count"] == 0
        if kw.get("minDocCount") == 30:
            assert red and all(x["doc_count"] >= 30 for x in red)
    keys, rmasks = rng_masks(segs, RANGES)
    h = dh(STATS, minDocCount=0, bounds=(T0 - 5 * H, T0 + 15 * H))
    check(engine, segs, rng_root(RANGES, [h]), rmasks, [h], keys=keys)
    s.close()


# ---- empty buckets --------------------------------------------------------------------------------------------------
def test_empty_buckets_carry_the_empty_histogram(engine, edge_seg, edge_cols):
    segs = [(edge_seg, edge_cols, NDOCS)]
    filters = [("none", QB.termQuery("status", 7777)), ("all", [])]
    for h in (dh(STATS), dh(STATS, minDocCount=0, bounds=(T0, T0 + 2 * H))):
        shard, _ = check(engine, segs, flt_root(filters, [h]), flt_masks(segs, filters), [h], keys=["none", "all"])
        assert shard["buckets"][0]["doc_count"] == 0 and shard["buckets"][0]["h"]["buckets"] == []
        ranges = [("never", 300.0, 300.0), ("back", 400.0, 300.0), ("all", -np.inf, np.inf)]
        keys, masks = rng_masks(segs, ranges)
        shard, _ = check(engine, segs, rng_root(ranges, [h]), masks, [h], keys=keys)
        assert [b["doc_count"] for b in shard["buckets"]][1:] == [0, 0] and shard["buckets"][1]["h"]["buckets"] == []
        # all docs rejected by the query
        query = [QB.termQuery("status", 7777)]
        zero = [[np.zeros(NDOCS, bool)] for _ in range(2)]
        shard, _ = check(engine, segs, flt_root(filters, [h]), zero, [h], query=query)
        assert all(b["doc_count"] == 0 and b["h"]["buckets"] == [] for b in shard["buckets"])


def test_plan_without_a_collect_builds_every_bucket_with_the_empty_histogram(engine):
    for root in (flt_root(MIXED, [dh(STATS), AB.max("m").field("price")], other=True), rng_root(RANGES, [dh(STATS), dh([], name="h2")])):
        plan = engine.plan([root])
        res = plan.build()
        plan.close()
        for d in (res.to_dict()[root.name], reduce([res]).to_dict()[root.name]):
            assert len(d["buckets"]) == (5 if root.name == "f" else 4)
            assert all(b["doc_count"] == 0 and b["h"]["buckets"] == [] for b in d["buckets"])
    x = res.to_xcontent()
    assert '"doc_count":0,"h":{"buckets":[]},"h2":{"buckets":[]}' in x


# ---- segments -------------------------------------------------------------------------------------------------------------
def _three_segments(engine, base):
    """a middle range of keys, one wider below and one wider above it"""
    out = []
    for n, t0, edges in ((NDOCS, T0 + 10 * H, (3000, 9000, 20000)), (BLOCK + 77, T0 - 30 * H, (100, 200, 300, 5000, 8000, 8100, 8200)),
                         (2 * BLOCK + 1, T0 + 40 * H, (10, 8192, 16384))):
        c = with_ts(base, sorted_ts(n, edges, t0=t0), n)
        out.append((engine.upload_segment(c, n), c, n))
    return out


def test_two_and_three_segments_in_both_orders_widen_the_key_range(engine, base):
    a, b, c = _three_segments(engine, base)
    h = dh(STATS)
    hz = dh(STATS, name="z", interval="1d", timeZone="Europe/Berlin")  # a key table that grows, too
    for segs in ([a, b], [b, a], [a, c], [c, a], [a, b, c], [c, b, a], [b, c, a]):
        check(engine, segs, flt_root(MIXED, [h, hz], other=True), flt_masks(segs, MIXED, True), [h, hz])
        keys, masks = rng_masks(segs, RANGES)
        check(engine, segs, rng_root(RANGES, [h]), masks, [h], keys=keys)
    for s, _c, _n in (a, b, c):
        s.close()


def test_segment_without_the_timestamp_field_and_without_the_range_field(engine, base):
    n2 = BLOCK + 5
    c1 = with_ts(base, sorted_ts(NDOCS, (5000, 17000)), NDOCS)
    c2 = {f: {"type": base[f]["type"], "values": base[f]["values"][:n2]} for f in FIELDS}   # no @timestamp
    s1, s2 = engine.upload_segment(c1, NDOCS), engine.upload_segment(c2, n2)
    h = dh(STATS)
    for order in ((0, 1), (1, 0)):
        segs = [[(s1, c1, NDOCS), (s2, c2, n2)][i] for i in order]
        res, stats = run(engine, [s for s, _c, _n in segs], [flt_root(MIXED, [h], other=True), rng_root(RANGES, [h])])
        assert stats[2] == 13
        d = reduce([res]).to_dict()
        m1 = MH.filters_masks(c1, MIXED, NDOCS, True)
        m2 = MH.filters_masks(c2, MIXED, n2, True)
        for i, b in enumerate(d["f"]["buckets"]):   # the second segment's docs count in the buckets and in no histogram bucket
            assert b["doc_count"] == int(m1[i].sum()) + int(m2[i].sum())
            want = O.run([(c1, NDOCS)], [dh(STATS)], accept=[bits_from_mask(m1[i])])
            assert_same(b["h"], want["reduced"]["h"], "f[%d]" % i)
        keys, r1 = MH.range_masks(c1, RT, RANGES, NDOCS)
        _k, r2 = MH.range_masks(c2, RT, RANGES, n2)
        for i, b in enumerate(d["r"]["buckets"]):
            assert b["key"] == keys[i] and b["doc_count"] == int(r1[i].sum()) + int(r2[i].sum())
            want = O.run([(c1, NDOCS)], [dh(STATS)], accept=[bits_from_mask(r1[i])])
            assert_same(b["h"], want["reduced"]["h"], "r[%d]" % i)
    # a segment without the range field contributes nothing, as the metric-only range collect treats it
    c3 = {f: v for f, v in c1.items() if f != RT}
    s3 = engine.upload_segment(c3, NDOCS)
    res, _ = run(engine, [s1, s3], [rng_root(RANGES, [h])])
    alone, _ = run(engine, [s1], [rng_root(RANGES, [h])])
    assert reduce([res]).to_dict() == reduce([alone]).to_dict()
    for s in (s1, s2, s3):
        s.close()


# ---- query clauses, accept bits, plans ------------------------------------------------------------------------------
def test_more_than_four_query_clauses_and_accept_bits(engine, edge_seg, edge_cols):
    query = [QB.rangeQuery("bytes").gte(500), QB.rangeQuery("bytes").lt(900000), QB.rangeQuery(RT).lt(990),
             QB.rangeQuery("price").gte(1.5), QB.rangeQuery("price").lt(998.0), QB.termQuery("status", 200)]
    acc = np.random.default_rng(5).random(NDOCS) < 0.7
    segs = [(edge_seg, edge_cols, NDOCS)]
    h = dh(STATS)
    # (the oracle applies the query itself: the masks carry the accept bits only, the doc counts both)
    res, stats = run(engine, [edge_seg], [flt_root(CLASSES, [h], other=True), rng_root(RANGES, [h])], query, [acc])
    d = reduce([res]).to_dict()
    qm = np.ones(NDOCS, bool)
    for q in query:
        qm &= FR.clause_mask(edge_cols, q, NDOCS)
    keys, rm = MH.range_masks(edge_cols, RT, RANGES, NDOCS, acc)
    for name, masks in (("f", MH.filters_masks(edge_cols, CLASSES, NDOCS, True, acc & qm)), ("r", [m & qm for m in rm])):
        for i, b in enumerate(d[name]["buckets"]):
            assert b["doc_count"] == int(masks[i].sum()), (name, i)
            want = O.run([(edge_cols, NDOCS)], [dh(STATS)], filters=query, accept=[bits_from_mask(masks[i])])
            assert_same(b["h"], want["reduced"]["h"], "%s[%d]" % (name, i))
    assert 0 < sum(b["doc_count"] for b in d["f"]["buckets"]) < int(acc.sum()) and stats[2] == 13


def test_reset_and_reuse_and_two_shards_reduced(engine, base, edge_seg, edge_cols):
    n1 = BLOCK + 900
    c1 = with_ts(base, sorted_ts(n1, (50, 4000, 8192), t0=T0 - 3 * H), n1)
    s1 = engine.upload_segment(c1, n1)
    h = dh(STATS, minDocCount=0)
    aggs = [flt_root(MIXED, [h, AB.avg("a").field(RT)], other=True), rng_root(RANGES, [h])]
    plan = engine.plan(aggs)
    assert plan.shard_mergeable()
    plan.collect(edge_seg)
    r0 = plan.build()
    plan.reset()
    plan.collect(s1)
    r1 = plan.build()
    plan.reset()
    plan.collect(edge_seg)
    assert plan.build().to_dict() == r0.to_dict()
    plan.close()
    red = reduce([r0, r1]).to_dict()
    m0, m1 = MH.filters_masks(edge_cols, MIXED, NDOCS, True), MH.filters_masks(c1, MIXED, n1, True)
    for i, b in enumerate(red["f"]["buckets"]):
        assert b["doc_count"] == int(m0[i].sum()) + int(m1[i].sum())
        want = O.run([(edge_cols, NDOCS), (c1, n1)], [dh(STATS, minDocCount=0)], accept=[bits_from_mask(m0[i]), bits_from_mask(m1[i])])
        assert_same(b["h"], want["reduced"]["h"], "f[%d]" % i)
    _k, q0 = MH.range_masks(edge_cols, RT, RANGES, NDOCS)
    _k, q1 = MH.range_masks(c1, RT, RANGES, n1)
    for i, b in enumerate(red["r"]["buckets"]):
        want = O.run([(edge_cols, NDOCS), (c1, n1)], [dh(STATS, minDocCount=0)], accept=[bits_from_mask(q0[i]), bits_from_mask(q1[i])])
        assert_same(b["h"], want["reduced"]["h"], "r[%d]" % i)
    s1.close()


# ---- tiny segments --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2049, 8191, 8193])
def test_tiny_segments(engine, base, n):
    c = with_ts(base, sorted_ts(n, (n // 2,) if n > 1 else ()), n)
    s = engine.upload_segment(c, n)
    segs = [(s, c, n)]
    h = dh(STATS)
    shard, _ = check(engine, segs, flt_root(MIXED, [h], other=True), flt_masks(segs, MIXED, True), [h])
    keys, masks = rng_masks(segs, RANGES)
    check(engine, segs, rng_root(RANGES, [h]), masks, [h], keys=keys)
    s.close()
    assert len({x["key"] for b in shard["buckets"] for x in b["h"]["buckets"]}) == (2 if n > 1 else 1)


# ---- layouts ---------------------------------------------------------------------------------------------------------
def test_layouts_and_released_wide_columns_give_the_same_result(engine, edge_cols):
    s = engine.upload_segment(edge_cols, NDOCS)
    aggs = [flt_root(MIXED, [dh(STATS), dh([AB.extendedStats("x").field(RT)], name="h2")], other=True), rng_root(RANGES, [dh(STATS)])]
    try:
        engine.set_option("compact_columns", 0)
        wide = run(engine, [s], aggs)[0].to_dict()
        engine.set_option("compact_columns", 1)
        compact = run(engine, [s], aggs)[0].to_dict()
    finally:
        engine.set_option("compact_columns", 1)
    assert compact == wide
    # requests that build the compact copies of the long columns (the timestamps included); their wide values are released
    flt = [QB.rangeQuery(RT).gte(0), QB.rangeQuery("bytes").gte(0), QB.rangeQuery("status").gte(0)]
    run(engine, [s], [AB.dateHistogram("t").field(TS).interval("1h").subAggregation(AB.stats("b").field("bytes"))], query=flt)
    beside = run(engine, [s], aggs)[0].to_dict()
    released = s.release_wide()
    assert released >= 8 * NDOCS
    again = run(engine, [s], aggs)[0].to_dict()
    s.close()
    assert beside == wide and again == wide
    segs = [(None, edge_cols, NDOCS)]
    masks = flt_masks(segs, MIXED, True)
    for i, b in enumerate(wide["f"]["buckets"]):
        want = O.run([(edge_cols, NDOCS)], [dh(STATS)], accept=[bits_from_mask(masks[i][0])])
        assert_same(b["h"], want["shards"][0]["h"], "f[%d]" % i)


# ---- rendering -----------------------------------------------------------------------------------------------------------
def _subtree_text(xcontent, name, i, nb):
    """the text of `"h":{...}` in bucket i of an XContent rendering whose buckets each hold exactly one such member"""
    parts = xcontent.split('"%s":' % name)
    assert len(parts) == nb + 1
    body = parts[i + 1]
    depth = 0
    for k, ch in enumerate(body):
        depth += ch in "{["
        depth -= ch in "}]"
        if depth == 0:
            return body[: k + 1]
    raise AssertionError("unbalanced")


def test_rendering_json_xcontent_and_stream(engine, base):
    n = 6000
    c = with_ts(base, sorted_ts(n, (10, 2048, 4097)), n)
    s = engine.upload_segment(c, n)
    h = dh([AB.stats("s").field("bytes"), AB.avg("m").field("bytes")])
    res, _ = run(engine, [s], [flt_root(CLASSES[:2], [h], other=True)])
    s.close()
    masks = MH.filters_masks(c, CLASSES[:2], n, True)
    x = res.to_xcontent()
    dec = MH.decode_stream(res.to_stream())
    assert dec[0]["stream_type"] == "filters" and len(dec[0]["buckets"]) == 3
    for i, m in enumerate(masks):
        want = O.run([(c, n)], [copy.deepcopy(h)], accept=[bits_from_mask(m)], streams=True)
        # XContent: the histogram member of bucket i is the oracle's rendering of its reference tree
        ref = json.loads(_subtree_text(x, "h", i, 3))
        shard = want["shards"][0]["h"]
        strip = lambda t: ({k: strip(v) for k, v in t.items() if k not in ("_internal", "_exact")} if isinstance(t, dict)  # noqa: E731
                           else [strip(v) for v in t] if isinstance(t, list) else t)
        assert ref == strip(shard), i
        assert_same(res.to_dict()["f"]["buckets"][i]["h"], shard, "json[%d]" % i)
        # the transport stream: bucket i's aggregations decode to what the oracle's own stream decodes to
        ref_stream = MH.decode_stream(want["streams"][0])
        assert dec[0]["buckets"][i]["doc_count"] == int(m.sum())
        assert dec[0]["buckets"][i]["aggs"] == ref_stream, i


# ---- refusals at collect ------------------------------------------------------------------------------------------------
def test_shapes_refused_at_collect_and_the_engine_stays_usable(engine, base):
    rng = np.random.default_rng(9)
    n = 1000
    cnt = rng.integers(0, 3, size=n)
    c = with_ts(base, sorted_ts(n, (500,)), n)
    c["multi"] = csr_sorted(cnt, rng.integers(0, 9, size=cnt.sum()), np.int64, N.COL_I64)
    c["dts"] = {"type": N.COL_F64, "values": c[TS]["values"].astype(np.float64)}
    s = engine.upload_segment(c, n)
    one = [("a", QB.rangeQuery(RT).lt(500))]
    h_on = lambda f: AB.dateHistogram("h").field(f).interval("1h")  # noqa: E731
    bad = ([flt_root(one, [h_on("multi")])], [flt_root(one, [h_on("dts")])], [rng_root(RANGES, [h_on("multi")])],
           [rng_root(RANGES, [h_on("dts")])], [flt_root(one, [dh([AB.stats("m").field("multi")])])],
           [rng_root(RANGES, [dh([AB.sum("m").field("multi")])])], [rng_root(RANGES, [dh()], field="multi")])
    for aggs in bad:
        plan = engine.plan(aggs)
        with pytest.raises(N.UnsupportedOnGpu):
            plan.collect(s)
        plan.close()
    segs = [(s, c, n)]
    h = dh(STATS)
    check(engine, segs, flt_root(one, [h], other=True), flt_masks(segs, one, True), [h])
    # the multi-valued range field still runs without the histogram child (path 11)
    res, stats = run(engine, [s], [rng_root(RANGES, [AB.stats("b").field("bytes")], field="multi")])
    s.close()
    assert stats[2] == 11 and len(res.to_dict()["r"]["buckets"]) == 4


def test_numeric_histogram_and_third_level_stay_refused_at_create(engine):
    ok = lambda: AB.filters("f").filter("a", QB.termQuery("status", 200))  # noqa: E731
    for aggs in ([ok().subAggregation(AB.histogram("h").field("bytes").interval(10))],
                 [ok().subAggregation(dh([AB.terms("t").field("status")]))],
                 [ok().subAggregation(dh([AB.cardinality("c").field("bytes")]))],
                 [rng_root(RANGES, [dh([dh(name="h2")])])],
                 [AB.terms("t").field("status").subAggregation(ok().subAggregation(dh()))]):
        with pytest.raises(N.UnsupportedOnGpu):
            engine.plan(aggs)
