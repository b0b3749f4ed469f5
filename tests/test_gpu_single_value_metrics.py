"""GPU parity of the single-value metrics sum / min / max / value_count (SumAggregator.java:74-100, MinAggregator.java:
78-113, MaxAggregator.java:79-114, ValueCountAggregator.java:75-98) in every place a numeric-metric leaf is accepted.

The oracle has no aggregator for the four.  The expected results come from two independent sources: the **stats twin**
(tests/single_metric_stream.py: each leaf as a stats leaf of the same name and field through the unchanged oracle,
mapped back to {"value": ...} and compared with helpers.assert_same under its own rules) and, for value_count over
keyword and multi-valued columns, which the twin cannot express, direct numpy counts per bucket.

Shards hold 3 * 8192 + 17 docs: a partial last block plus padding.
"""
import math

import numpy as np
import pytest

import es_stream as ES
import oracle as O
import single_metric_stream as SM
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Order, QueryBuilders as QB
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from helpers import assert_same, bits_from_mask, synthetic_columns
from test_gpu_multivalued import csr_sorted

pytestmark = pytest.mark.gpu

N_DOCS = 3 * 8192 + 17
FIELDS = ("host", "@timestamp", "response_time_ms", "bytes", "status", "price")

_COLS = {}


def shard_cols(shard=0, n=N_DOCS):
    """One synthetic shard's host columns (computed once, shared, never changed)."""
    if (shard, n) not in _COLS:
        _COLS[(shard, n)] = synthetic_columns(FIELDS, n, shard=shard)
    return _COLS[(shard, n)]


def sparse_cols(shard=0, n=N_DOCS):
    """The shard with response_time_ms present in 60 % of the docs; the last 17 docs alternate."""
    cols = dict(shard_cols(shard, n))
    present = np.random.default_rng(11 + shard).random(n) < 0.6
    present[-17:] = np.arange(17) % 2 == 0
    rt = cols["response_time_ms"]
    cols["response_time_ms"] = dict(rt, values=np.where(present, rt["values"], 0), present=bits_from_mask(present))
    return cols, present


def run(engine, aggs, shards, filters=None, exact=True, segments=None):
    """Every shard's result and their reduce against the stats twin.  shards: [(columns, max_doc)]; segments: per shard
    the column sets collected into its plan (default: the shard's columns as one segment).  Returns (results, reduced
    dict, collect stats of the last shard)."""
    want = O.run(shards, SM.twin(aggs), filters=filters, number_of_shards=len(shards))
    results, stats = [], None
    for s, (cols, n) in enumerate(shards):
        plan = engine.plan(aggs, filters=filters, number_of_shards=len(shards))
        segs = [engine.upload_segment(c, m) for c, m in (segments[s] if segments else [(cols, n)])]
        for seg in segs:
            plan.collect(seg)
        stats = plan.last_collect_stats()
        r = plan.build()
        assert_same(r.to_dict(), SM.untwin(want["shards"][s], aggs), f"shard{s}", exact)
        results.append(r)
        plan.close()
        for seg in segs:
            seg.close()
    red = reduce(results).to_dict()
    assert_same(red, SM.untwin(want["reduced"], aggs), "reduced", exact)
    return results, red, stats


def hour():
    return AB.dateHistogram("per_hour").field("@timestamp").interval("1h")


def four(field="response_time_ms"):
    return [AB.sum("s").field(field), AB.min("mn").field(field), AB.max("mx").field(field), AB.count("c").field(field)]


# ---- 1. histogram-only grids (run accumulators, integer runs) ------------------------------------------------------
def test_date_histogram_leaves(engine):
    h = hour().subAggregation(AB.sum("s").field("response_time_ms")).subAggregation(AB.max("mx").field("response_time_ms")) \
        .subAggregation(AB.min("mn").field("bytes")).subAggregation(AB.count("c").field("status"))
    _, red, _ = run(engine, [h], [(shard_cols(), N_DOCS)])
    assert sum(b["c"]["value"] for b in red["per_hour"]["buckets"]) == N_DOCS


def test_date_histogram_empty_buckets_render_empty_values(engine):
    ts = shard_cols()["@timestamp"]["values"]
    lo, hi = int(ts.min()) - 5 * 3_600_000, int(ts.max()) + 5 * 3_600_000
    h = hour().minDocCount(0).extendedBounds(lo, hi)
    for leaf in four():
        h.subAggregation(leaf)
    results, red, _ = run(engine, [h], [(shard_cols(), N_DOCS)])
    empty = [b for b in red["per_hour"]["buckets"] if b["doc_count"] == 0]
    assert len(empty) >= 10
    for b in empty:
        assert (b["s"]["value"], b["mn"]["value"], b["mx"]["value"], b["c"]["value"]) == (0.0, math.inf, -math.inf, 0)
    x = reduce(results).to_xcontent()
    assert '"s":{"value":0.0},"mn":{"value":null},"mx":{"value":null},"c":{"value":0}' in x


# ---- 2. terms grids ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", ["sum", "max"])
def test_terms_packed_integer_cells(engine, leaf):
    b = AB.sum("v") if leaf == "sum" else AB.max("v")
    run(engine, [AB.terms("hosts").field("host").size(20).subAggregation(b.field("response_time_ms"))], [(shard_cols(), N_DOCS)])


def test_terms_f64_cells_and_two_fields(engine):
    aggs = [AB.terms("hosts").field("host").size(20).subAggregation(AB.min("lo").field("price"))
            .subAggregation(AB.sum("total").field("price")),
            AB.terms("mixed").field("host").size(15).subAggregation(AB.max("mb").field("bytes"))
            .subAggregation(AB.stats("st").field("response_time_ms")).subAggregation(AB.sum("sr").field("response_time_ms"))
            .subAggregation(AB.count("cb").field("bytes"))]
    run(engine, aggs, [(shard_cols(), N_DOCS)], exact=False)


# ---- 3. the window kernel, 2 shards reduced ------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", ["sum", "max"])
def test_terms_date_histogram_window(engine, leaf):
    b = AB.sum("v") if leaf == "sum" else AB.max("v")
    aggs = [AB.terms("hosts").field("host").size(10).subAggregation(hour().subAggregation(b.field("response_time_ms")))]
    run(engine, aggs, [(shard_cols(0, 2 * N_DOCS), 2 * N_DOCS), (shard_cols(1, 2 * N_DOCS), 2 * N_DOCS)])


# ---- 4. sparse metric ----------------------------------------------------------------------------------------------
def test_sparse_metric_all_leaves(engine):
    cols, present = sparse_cols()
    t = AB.terms("hosts").field("host").size(20)
    for leaf in four():
        t.subAggregation(leaf)
    aggs = [t,
            hour().subAggregation(AB.count("lone").field("response_time_ms")),  # a lone count: the product
            AB.dateHistogram("h2").field("@timestamp").interval("1h")          # count beside sum: one shared pipeline
            .subAggregation(AB.count("c").field("response_time_ms")).subAggregation(AB.sum("s").field("response_time_ms")),
            AB.count("all").field("response_time_ms"),
            AB.terms("t2").field("host").size(5).subAggregation(AB.count("lone").field("response_time_ms"))]
    _, red, _ = run(engine, aggs, [(cols, N_DOCS)])
    assert red["all"]["value"] == int(present.sum()) != N_DOCS
    assert sum(b["lone"]["value"] for b in red["per_hour"]["buckets"]) == int(present.sum())
    assert any(b["c"]["value"] != b["doc_count"] for b in red["hosts"]["buckets"])


# ---- 5. multi-valued and keyword columns ---------------------------------------------------------------------------
def mv_cols(n=N_DOCS, seed=5):
    rng = np.random.default_rng(seed)
    cols = dict(shard_cols(0, n))
    cc = rng.integers(0, 4, size=n)                      # 0-3 values per doc, per-doc duplicates kept (SortedNumeric)
    cols["codes"] = csr_sorted(cc, rng.integers(0, 5, size=cc.sum()), np.int64, N.COL_I64)
    tc = rng.integers(0, 4, size=n)
    tags = csr_sorted(tc, rng.integers(0, 30, size=tc.sum()), np.uint32, N.COL_ORD_U32, unique=True)
    cols["tags"] = dict(tags, terms=["tag-%02d" % i for i in range(30)])
    kw = rng.integers(0, 12, size=n).astype(np.uint32)
    kw[rng.random(n) < 0.3] = 0xFFFFFFFF
    kw[-17:] = np.where(np.arange(17) % 2 == 0, 3, 0xFFFFFFFF)
    cols["kw"] = {"type": N.COL_ORD_U32, "values": kw, "terms": ["kw-%02d" % i for i in range(12)]}
    return cols


def test_multi_valued_long_all_leaves(engine):
    cols = mv_cols()
    t = AB.terms("hosts").field("host").size(20)
    for leaf in four("codes"):
        t.subAggregation(leaf)
    aggs = [t] + four("codes") + [AB.terms("t2").field("host").size(20).subAggregation(AB.count("lone").field("codes"))]
    _, red, _ = run(engine, aggs, [(cols, N_DOCS)])
    per_doc = np.diff(cols["codes"]["offsets"].astype(np.int64))
    assert red["c"]["value"] == int(per_doc.sum()) and per_doc.max() == 3
    host = cols["host"]["values"]
    for b in red["t2"]["buckets"]:
        assert b["lone"]["value"] == int(per_doc[host == int(b["key"][5:])].sum())


def test_value_count_over_keyword_columns_against_numpy(engine):
    cols = mv_cols()
    host = cols["host"]["values"].astype(np.int64)
    per_tags = np.diff(cols["tags"]["offsets"].astype(np.int64))
    per_kw = (cols["kw"]["values"] != 0xFFFFFFFF).astype(np.int64)
    aggs = [AB.terms("hosts").field("host").size(1000).subAggregation(AB.count("tags").field("tags"))
            .subAggregation(AB.count("kw").field("kw")),
            AB.count("all_tags").field("tags"), AB.count("all_kw").field("kw")]
    seg = engine.upload_segment(cols, N_DOCS)
    plan = engine.plan(aggs)
    plan.collect(seg)
    got = reduce([plan.build()]).to_dict()
    plan.close()
    seg.close()
    assert got["all_tags"] == {"value": int(per_tags.sum())} and got["all_kw"] == {"value": int(per_kw.sum())}
    want_tags = np.bincount(host, weights=per_tags, minlength=1000).astype(np.int64)
    want_kw = np.zeros(1000, dtype=np.int64)
    np.add.at(want_kw, host, per_kw)
    docs = np.bincount(host, minlength=1000)
    buckets = got["hosts"]["buckets"]
    assert len(buckets) == int((docs > 0).sum())
    for b in buckets:
        h = int(b["key"][5:])
        assert (b["doc_count"], b["tags"]["value"], b["kw"]["value"]) == (docs[h], want_tags[h], want_kw[h]), b["key"]


# ---- 6. dense shortcut ---------------------------------------------------------------------------------------------
def test_lone_count_over_dense_column_is_the_doc_count(engine):
    aggs = [AB.terms("hosts").field("host").size(20).subAggregation(AB.count("c").field("status")), AB.count("all").field("status")]
    _, red, _ = run(engine, aggs, [(shard_cols(), N_DOCS)])
    assert red["all"]["value"] == N_DOCS
    assert all(b["c"]["value"] == b["doc_count"] for b in red["hosts"]["buckets"])


# ---- 7. terms ordered by each of the four --------------------------------------------------------------------------
def few_hosts_cols(shard, n=N_DOCS):
    """hosts 0..39 only, in a 60-term dictionary: 20 terms never occur (min_doc_count 0 lists them, empty)"""
    cols, _ = sparse_cols(shard, n)
    cols = dict(cols)
    cols["host"] = {"type": N.COL_ORD_U32, "values": (cols["host"]["values"] % 40).astype(np.uint32),
                    "terms": ["host-%04d" % i for i in range(60)]}
    return cols


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("kind", ["sum", "min", "max", "count"])
def test_terms_ordered_by_single_value_metric(engine, kind, asc):
    leaf = {"sum": AB.sum, "min": AB.min, "max": AB.max, "count": AB.count}[kind]("m").field("response_time_ms")
    path = "m" if asc else "m.value"
    aggs = [AB.terms("hosts").field("host").size(50).shardSize(60).minDocCount(0).order(Order.aggregation(path, asc))
            .subAggregation(leaf)]
    shards = [(few_hosts_cols(s), N_DOCS) for s in range(3)]
    _, red, _ = run(engine, aggs, shards)
    assert red["hosts"]["doc_count_error_upper_bound"] == -1
    empty = [b for b in red["hosts"]["buckets"] if b["doc_count"] == 0]
    assert empty and all(b["m"]["value"] == {"sum": 0.0, "min": math.inf, "max": -math.inf, "count": 0}[kind] for b in empty)


def test_terms_ordered_by_max_one_level_down(engine):
    aggs = [AB.dateHistogram("per_day").field("@timestamp").interval("1d").subAggregation(
        AB.terms("hosts").field("host").size(5).order(Order.aggregation("mx", False))
        .subAggregation(AB.max("mx").field("response_time_ms")))]
    run(engine, aggs, [(few_hosts_cols(s), N_DOCS) for s in range(2)])


# ---- 8. depth ------------------------------------------------------------------------------------------------------
def depth_cols(shard=0, n=N_DOCS):
    cols = dict(shard_cols(shard, n))
    rng = np.random.default_rng(40 + shard)
    cols["dc"] = {"type": N.COL_ORD_U32, "values": rng.integers(0, 4, size=n).astype(np.uint32), "terms": ["dc-%d" % i for i in range(4)]}
    cols["svc"] = {"type": N.COL_ORD_U32, "values": rng.integers(0, 300, size=n).astype(np.uint32),
                   "terms": ["svc-%03d" % i for i in range(300)]}
    present = rng.random(n) < 0.6
    cols["rt_sparse"] = {"type": N.COL_I64, "values": np.where(present, cols["response_time_ms"]["values"], 0),
                         "present": bits_from_mask(present)}
    return cols


def test_three_levels_and_terms_under_terms(engine):
    aggs = [AB.terms("dc").field("dc").size(4).subAggregation(AB.terms("hosts").field("host").size(3).subAggregation(
                hour().subAggregation(AB.sum("s").field("response_time_ms")))),
            AB.terms("dc2").field("dc").size(4).subAggregation(AB.terms("svc").field("svc").size(5)
                                                             .subAggregation(AB.max("mx").field("bytes")))]
    run(engine, aggs, [(depth_cols(), N_DOCS)])


def test_breadth_first_replay_with_sum_leaf(engine, monkeypatch):
    monkeypatch.setenv("ESGPU_DEFER_CELLS", "1000")  # the replay forced onto a small grid (test_gpu_breadth_first.py)
    aggs = [AB.terms("hosts").field("host").size(5).subAggregation(
        AB.terms("svc").field("svc").size(4).subAggregation(AB.sum("s").field("response_time_ms"))
        .subAggregation(AB.count("c").field("response_time_ms"))),
        # a lone count over a sparse column in the replayed level: its product, collected by the replay
        AB.terms("hosts2").field("host").size(5).subAggregation(
            AB.terms("svc").field("svc").size(4).subAggregation(AB.count("lone").field("rt_sparse")))]
    cols = depth_cols()
    want = O.run([(cols, N_DOCS)], SM.twin(aggs))
    seg = engine.upload_segment(cols, N_DOCS)
    plan = engine.plan(aggs)
    plan.collect(seg)
    assert plan.deferred_segments() >= 1
    got = plan.build().to_dict()
    plan.close()
    seg.close()
    assert_same(got, SM.untwin(want["shards"][0], aggs), "replayed")


def test_filter_aggregation_children_under_terms_with_query_filter(engine):
    f = AB.filter("errors", [QB.rangeQuery("status").gte(400)]).subAggregation(AB.sum("s").field("response_time_ms")) \
        .subAggregation(AB.count("c").field("response_time_ms"))
    aggs = [AB.terms("hosts").field("host").size(10).subAggregation(f)]
    run(engine, aggs, [(shard_cols(), N_DOCS)], filters=[QB.rangeQuery("bytes").gte(1024).lte(1 << 20)])


@pytest.mark.parametrize("leaves", ["sum_max", "lone_sparse_count"])
def test_co_located_and_cross_rank_build_reduce(engine, leaves):
    """esgpu_plans_build_reduce and esgpu_comm_build_reduce (one RCCL rank, two local shards) over terms{date_histogram
    {...}}: sum + max ride the device merge like avg / stats leaves; a lone sparse value_count is built per shard and
    reduced.  Either way the result is the reduce of the shards' results."""
    import elasticsearch_amd as ea
    from elasticsearch_amd import build_reduce
    h = hour()
    if leaves == "sum_max":
        h.subAggregation(AB.sum("s").field("response_time_ms")).subAggregation(AB.max("mx").field("response_time_ms"))
        shards = [(shard_cols(s), N_DOCS) for s in range(2)]
    else:
        h.subAggregation(AB.count("c").field("response_time_ms"))
        shards = [(sparse_cols(s)[0], N_DOCS) for s in range(2)]
    aggs = [AB.terms("hosts").field("host").size(10).subAggregation(h)]
    want = SM.untwin(O.run(shards, SM.twin(aggs), number_of_shards=2)["reduced"], aggs)
    segs = [engine.upload_segment(c, n) for c, n in shards]
    plans = [engine.plan(aggs, number_of_shards=2) for _ in shards]
    comm = ea.Communicator(engine, 1, 0, ea.Communicator.unique_id())
    for fused in (build_reduce, lambda ps: comm.build_reduce(ps, root=0)):
        for p, seg in zip(plans, segs):
            p.reset()
            p.collect(seg)
        assert_same(fused(plans).to_dict(), want, leaves)
    if leaves == "sum_max":
        assert comm.last_build_reduce()[0] == 1  # the device-resident path
    comm.close()
    for p in plans:
        p.close()
    for seg in segs:
        seg.close()


# ---- 9. float edge values through the f64 path ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["inf", "inf_ninf", "nan", "subnormal", "mixed"])
def test_float_edge_values(engine, kind):
    from test_gpu_float_parity import SPECIAL, _special_column
    rng = np.random.default_rng(SPECIAL.index(kind) + 100)
    n = N_DOCS
    cols = dict(shard_cols(0, n))
    cols["host"] = {"type": N.COL_ORD_U32, "values": rng.integers(0, 50, n).astype(np.uint32), "terms": ["h%03d" % i for i in range(50)]}
    price = _special_column(rng, n, kind)
    if kind == "mixed":  # -0.0 against 0.0 inside one bucket, for min and max
        z = np.nonzero(cols["host"]["values"] == 7)[0]
        price[z] = 0.0
        price[z[::2]] = -0.0
    cols["price"] = {"type": N.COL_F64, "values": price}
    aggs = [AB.terms("hosts").field("host").size(50).subAggregation(AB.min("mn").field("price"))
            .subAggregation(AB.max("mx").field("price")).subAggregation(AB.sum("s").field("price")),
            hour().subAggregation(AB.min("mn").field("price")).subAggregation(AB.sum("s").field("price")),
            AB.min("mn").field("price"), AB.max("mx").field("price"), AB.sum("s").field("price")]
    _, red, _ = run(engine, aggs, [(cols, n)], exact=False)
    if kind == "mixed":
        b7 = [b for b in red["hosts"]["buckets"] if b["key"] == "h007"][0]
        assert math.copysign(1.0, b7["mn"]["value"]) == -1.0 and math.copysign(1.0, b7["mx"]["value"]) == 1.0
    if kind == "nan":
        assert math.isnan(red["mn"]["value"]) and math.isnan(red["mx"]["value"])


# ---- 10. two segments in one plan, an ordinal map on host, one segment lacking the metric field ---------------------
def test_two_segments_with_ordinal_map_one_lacking_the_field(engine):
    a, b = dict(shard_cols(0)), dict(shard_cols(1))
    a["host"] = {"type": N.COL_ORD_U32, "values": (a["host"]["values"] % 30).astype(np.uint32), "terms": ["host-%04d" % (2 * i) for i in range(30)]}
    b["host"] = {"type": N.COL_ORD_U32, "values": (b["host"]["values"] % 45).astype(np.uint32), "terms": ["host-%04d" % i for i in range(45)]}
    b_seg = {f: c for f, c in b.items() if f != "response_time_ms"}  # unmapped in this segment
    # the oracle's shard: both segments' docs over one dictionary, the second segment's metric values absent
    terms = sorted(set(a["host"]["terms"]) | set(b["host"]["terms"]))
    at = {t: i for i, t in enumerate(terms)}
    both = {}
    for f in FIELDS:
        both[f] = dict(a[f], values=np.concatenate([a[f]["values"], b[f]["values"]]))
    both["host"] = {"type": N.COL_ORD_U32, "terms": terms, "values": np.concatenate(
        [np.array([at[a["host"]["terms"][o]] for o in a["host"]["values"]], dtype=np.uint32),
         np.array([at[b["host"]["terms"][o]] for o in b["host"]["values"]], dtype=np.uint32)])}
    both["response_time_ms"]["present"] = bits_from_mask(np.arange(2 * N_DOCS) < N_DOCS)
    t = AB.terms("hosts").field("host").size(60)
    for leaf in four():
        t.subAggregation(leaf)
    aggs = [t, AB.terms("t2").field("host").size(60).subAggregation(AB.count("lone").field("response_time_ms"))] + four()
    want = O.run([(both, 2 * N_DOCS)], SM.twin(aggs))
    for order in ((a, b_seg), (b_seg, a)):  # the segment lacking the field first, and second
        segs = [engine.upload_segment(c, N_DOCS) for c in order]
        omap = engine.ordinal_map(segs, "host")
        plan = engine.plan(aggs)
        for seg in segs:
            plan.collect(seg)
        got = plan.build().to_dict()
        plan.close()
        omap.close()
        for seg in segs:
            seg.close()
        assert_same(got, SM.untwin(want["shards"][0], aggs), "two segments")


# ---- 11. bytes moved -----------------------------------------------------------------------------------------------
def collect_bytes(engine, aggs, cols, n=N_DOCS):
    seg = engine.upload_segment(cols, n)
    plan = engine.plan(aggs)
    plan.collect(seg)
    _ms, nbytes, _path = plan.last_collect_stats()
    plan.build()
    plan.close()
    seg.close()
    return nbytes


def test_bytes_moved(engine):
    """Deterministic figures of plan.last_collect_stats(): the bytes of the columns a launch reads, at the widths it
    reads them.  Per doc of this shard: host as 16-bit ordinals (2; 1,000 terms), @timestamp as 32-bit deltas over the
    column's minimum (4; 30 days over 24,593 docs leave every run of docs too wide for 16-bit block deltas),
    response_time_ms (0..999) as 16-bit deltas (2) where the launch takes integer cells or runs and as 32-bit deltas (4)
    where the column is sparse, the value-count product as 16-bit counts (2).  A present bitset is not charged."""
    cols = shard_cols()

    def nested(leaf):
        return [AB.terms("hosts").field("host").size(10).subAggregation(hour().subAggregation(leaf))]

    rt = "response_time_ms"
    b_sum, b_avg = collect_bytes(engine, nested(AB.sum("v").field(rt)), cols), collect_bytes(engine, nested(AB.avg("v").field(rt)), cols)
    b_max, b_stats = collect_bytes(engine, nested(AB.max("v").field(rt)), cols), collect_bytes(engine, nested(AB.stats("v").field(rt)), cols)
    b_none = collect_bytes(engine, [AB.terms("hosts").field("host").size(10).subAggregation(hour())], cols)
    b_dense = collect_bytes(engine, nested(AB.count("c").field("status")), cols)
    sp, _ = sparse_cols()
    h_sum = collect_bytes(engine, [hour().subAggregation(AB.sum("s").field(rt))], sp)
    h_cnt = collect_bytes(engine, [hour().subAggregation(AB.count("c").field(rt))], sp)
    print("bytes: sum %d avg %d max %d stats %d, no leaf %d, dense count %d, sparse sum %d, sparse count %d"
          % (b_sum, b_avg, b_max, b_stats, b_none, b_dense, h_sum, h_cnt))
    assert b_sum == b_avg == (2 + 4 + 2) * N_DOCS    # sum reads what avg reads
    assert b_max == b_stats == (2 + 4 + 2) * N_DOCS  # max reads what stats reads
    assert b_dense == b_none == (2 + 4) * N_DOCS     # a lone count over a dense column: no metric column
    assert h_sum == (4 + 4) * N_DOCS                 # timestamp + the sparse column's 32-bit deltas
    assert h_cnt == (4 + 2) * N_DOCS                 # timestamp + the 16-bit product
    assert h_cnt < h_sum


# ---- 12. transport bytes and XContent ------------------------------------------------------------------------------
def test_transport_bytes_and_xcontent(engine):
    north = [AB.terms("hosts").field("host").size(10).subAggregation(hour().subAggregation(AB.sum("s").field("response_time_ms")))]
    t = AB.terms("hosts").field("host").size(45).minDocCount(0)
    for leaf in four():
        t.subAggregation(leaf)
    for aggs, cols in ((north, shard_cols()), ([t], few_hosts_cols(0))):
        want = O.run([(cols, N_DOCS)], SM.twin(aggs), streams=True)
        seg = engine.upload_segment(cols, N_DOCS)
        plan = engine.plan(aggs)
        plan.collect(seg)
        r = plan.build()
        plan.close()
        seg.close()
        assert r.to_stream() == SM.write_stream(ES.decode(want["streams"][0]), aggs)
        tree = SM.untwin(O.run([(cols, N_DOCS)], SM.twin(aggs), exact=False)["shards"][0], aggs)
        assert r.to_xcontent() == SM.xcontent(tree, aggs)
    assert '"mn":{"value":null}' in r.to_xcontent()  # an empty bucket of the second request


# ---- 13. the product's cap -----------------------------------------------------------------------------------------
def test_product_cap_refuses_without_caching(engine):
    n = 8192 + 5
    counts = np.ones(n, dtype=np.int64)
    counts[100] = 65536
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(counts)
    cols = {"@timestamp": shard_cols(0, n)["@timestamp"],
            "big": {"type": N.COL_I64, "values": np.zeros(int(offs[-1]), dtype=np.int64), "offsets": offs},
            "ok": {"type": N.COL_I64, "values": np.zeros(n, dtype=np.int64), "offsets": np.arange(n + 1, dtype=np.uint64)}}
    seg = engine.upload_segment(cols, n)
    for _ in range(2):  # the refusal is not cached: the second request is refused the same way
        plan = engine.plan([AB.count("c").field("big")])
        with pytest.raises(N.EsGpuError) as e:
            plan.collect(seg)
        assert e.value.code == N.ERR_UNSUPPORTED
        plan.close()
    plan = engine.plan([AB.count("c").field("ok")])
    plan.collect(seg)
    assert plan.build().to_dict() == {"c": {"value": n}}
    plan.close()
    seg.close()


def test_sum_over_keyword_column_is_refused_at_collect(engine):
    seg = engine.upload_segment(shard_cols(), N_DOCS)
    plan = engine.plan([AB.sum("s").field("host")])
    with pytest.raises(N.EsGpuError, match="metric over non-numeric field"):
        plan.collect(seg)
    plan.close()
    seg.close()
