"""Terms over long / date fields on the GPU (LongTerms): the numeric ordinals of a long column (its sorted distinct values
and each doc's rank among them, built on the device on first use) feed every terms form keyword fields take.

Two independent references, since the oracle stays as it is:
  a. numpy -- np.unique for buckets, the selection rule restated in tests/long_terms_stream.py;
  b. the keyword twin -- the same docs with a keyword column whose terms are the 16 hex digits of value XOR 2^63 (their
     unsigned byte order is the longs' numeric order), run through the unchanged oracle and mapped back to longs.
"""
import struct

import numpy as np
import pytest

import long_terms_stream as LT
import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Order, QueryBuilders as QB
from elasticsearch_amd import _native as N
from elasticsearch_amd import build_reduce, reduce
from helpers import assert_same, bits_from_mask

pytestmark = pytest.mark.gpu

DOCS = 3 * 8192 + 17  # a partial last block plus padding
T0 = 1441065600000
LDS_BITS = 1 << 18    # spans below this are marked in the per-workgroup LDS bitmap (esgpu_kernels.hpp kNumOrdLdsBits)


def _col(values, present=None):
    c = {"type": N.COL_I64, "values": np.asarray(values, dtype=np.int64)}
    if present is not None:
        c["present"] = bits_from_mask(present)
    return c


def _all_buckets(engine, values, present=None):
    """terms over the column with size = all distinct values, _term asc -> (keys, counts, other)"""
    n = len(values)
    seg = engine.upload_segment({"v": _col(values, present)}, n)
    plan = engine.plan([AB.terms("t").field("v").size(0).order(Order.term(True))])
    try:
        plan.collect(seg)
        d = plan.build().to_dict()["t"]
    finally:
        plan.close()
        seg.close()
    return [b["key"] for b in d["buckets"]], [b["doc_count"] for b in d["buckets"]], d["sum_other_doc_count"]


def _check_numpy(engine, values, present=None):
    live = np.asarray(values)[present] if present is not None else np.asarray(values)
    keys, counts = np.unique(live, return_counts=True)
    got_k, got_c, other = _all_buckets(engine, values, present)
    assert got_k == keys.tolist()
    assert got_c == counts.tolist()
    assert other == 0


def _spread(rng, vmin, span, distinct, n=DOCS):
    """n values over [vmin, vmin + span] with about `distinct` distinct ones, both ends included"""
    pool = np.unique(np.concatenate([[0, span], rng.integers(0, span + 1, size=distinct, dtype=np.int64)]))
    v = pool[rng.integers(0, len(pool), size=n)]
    v[0], v[-1] = 0, span
    return v + vmin


# ---- the dense path against numpy ----
@pytest.mark.parametrize("k", [1, 3])
def test_dense_keys_on_every_word_boundary(engine, k):
    span = 64 * k + 1
    rng = np.random.default_rng(k)
    v = -130 + rng.integers(0, span + 1, size=DOCS)
    v[: span + 1] = -130 + np.arange(span + 1)  # every value of the span occurs
    _check_numpy(engine, v)


def test_dense_one_distinct_value(engine):
    _check_numpy(engine, np.full(DOCS, -7, dtype=np.int64))


def test_dense_present_bitset_with_holes(engine):
    rng = np.random.default_rng(5)
    v = rng.integers(-50, 900, size=DOCS)
    present = rng.random(DOCS) < 0.6
    present[-17:] = [i % 2 == 0 for i in range(17)]
    # the values of missing docs must not enter the dictionary: park them outside the live range
    v = np.where(present, v, 5000)
    _check_numpy(engine, v, present)


def test_all_missing_column(engine):
    keys, counts, other = _all_buckets(engine, np.zeros(DOCS, dtype=np.int64), np.zeros(DOCS, dtype=bool))
    assert (keys, counts, other) == ([], [], 0)


@pytest.mark.parametrize("span", [LDS_BITS - 2, LDS_BITS - 1, LDS_BITS, LDS_BITS + 1])
def test_dense_spans_around_the_lds_threshold(engine, span):
    _check_numpy(engine, _spread(np.random.default_rng(span), 1_000_003, span, 700))


def test_dense_widest_span(engine):
    _check_numpy(engine, _spread(np.random.default_rng(26), -(1 << 25), (1 << 26) - 1, 1000))


# ---- the wide path against numpy ----
SPECIALS = [-(1 << 63), (1 << 63) - 1, -1, 0]  # -1 is also the hash set's empty sentinel


def test_wide_full_range(engine):
    rng = np.random.default_rng(64)
    n = 200_000
    pool = np.concatenate([np.array(SPECIALS, dtype=np.int64),
                           rng.integers(-(1 << 63), (1 << 63) - 1, size=50_000, dtype=np.int64, endpoint=True)])
    v = pool[rng.integers(0, len(pool), size=n)]
    v[: len(SPECIALS)] = SPECIALS
    _check_numpy(engine, v)


def test_distinct_value_cap(engine):
    rng = np.random.default_rng(7)
    n = DOCS
    v = rng.integers(0, 5000, size=n, dtype=np.int64) * (1 << 40)
    v[:5000] = np.arange(5000, dtype=np.int64) * (1 << 40)
    kw = rng.integers(0, 9, size=n).astype(np.uint32)
    seg = engine.upload_segment({"v": _col(v), "kw": {"type": N.COL_ORD_U32, "values": kw,
                                                      "terms": ["k%d" % i for i in range(9)]}}, n)
    engine.set_option("numeric_terms_max_distinct", 1024)
    try:
        plan = engine.plan([AB.terms("t").field("v")])
        with pytest.raises(N.UnsupportedOnGpu) as e:
            plan.collect(seg)
        assert "more than 1024 distinct values" in str(e.value)
        plan.close()
        plan = engine.plan([AB.terms("t").field("kw").size(9).order(Order.term(True))])
        plan.collect(seg)
        got = plan.build().to_dict()["t"]["buckets"]
        assert [b["doc_count"] for b in got] == np.bincount(kw, minlength=9).tolist()
        plan.close()
    finally:
        engine.set_option("numeric_terms_max_distinct", 1 << 22)
        seg.close()
    assert engine.get_option("numeric_terms_max_distinct") == 1 << 22


@pytest.mark.parametrize("path", ["dense", "wide_without_overflow"])
def test_distinct_value_cap_other_branches(engine, path):
    """the cap where the hash set does not overflow: the dense path's distinct count, and a wide column whose 1,500
    distinct values fit the 2,048 slots of a cap of 1,024"""
    rng = np.random.default_rng(8)
    scale = 1 if path == "dense" else 1 << 40
    v = rng.integers(0, 1500, size=DOCS, dtype=np.int64) * scale
    v[:1500] = np.arange(1500, dtype=np.int64) * scale
    seg = engine.upload_segment({"v": _col(v)}, DOCS)
    engine.set_option("numeric_terms_max_distinct", 1024)
    try:
        plan = engine.plan([AB.terms("t").field("v")])
        with pytest.raises(N.UnsupportedOnGpu) as e:
            plan.collect(seg)
        assert "more than 1024 distinct values" in str(e.value)
        plan.close()
        engine.set_option("numeric_terms_max_distinct", 1500)  # exactly at the cap: accepted (the refusal is not cached)
        _check_numpy(engine, v)
    finally:
        engine.set_option("numeric_terms_max_distinct", 1 << 22)
        seg.close()


# ---- twin parity ----
def _twin_column(values, present=None):
    """the keyword twin of a long column: dictionary = the distinct values' twin terms, in numeric order"""
    values = np.asarray(values, dtype=np.int64)
    live = values if present is None else values[present]
    uniq = np.unique(live)
    ords = np.searchsorted(uniq, values).astype(np.uint32)
    if present is not None:
        ords[~present] = 0xFFFFFFFF
    return {"type": N.COL_ORD_U32, "values": ords, "terms": [LT.twin_term(x) for x in uniq]}


def _map_back(tree, names):
    """the twin result with the keys of the aggregations in `names` turned back into longs"""
    if isinstance(tree, dict):
        out = {}
        for k, v in tree.items():
            v = _map_back(v, names)
            if k in names and isinstance(v, dict) and "buckets" in v:
                for b in v["buckets"]:
                    b["key"] = LT.twin_long(b["key"])
            out[k] = v
        return out
    if isinstance(tree, list):
        return [_map_back(v, names) for v in tree]
    return tree


@pytest.fixture(scope="module")
def logs():
    rng = np.random.default_rng(2024)
    n = 200_000
    status = rng.choice([200, 200, 200, 304, 404, 500], size=n).astype(np.int64)
    rt = np.minimum(np.floor(rng.lognormal(4.0, 1.0, size=n)), 999).astype(np.int64)
    host = np.minimum(rng.zipf(1.3, size=n) - 1, 49).astype(np.uint32)
    ts = T0 + np.sort(rng.integers(0, 6 * 3_600_000, size=n)).astype(np.int64)
    cols = {
        "status": _col(status), "response_time_ms": _col(rt), "@timestamp": _col(ts),
        "host": {"type": N.COL_ORD_U32, "values": host, "terms": ["host-%02d" % i for i in range(50)]},
        "status_kw": _twin_column(status), "response_time_ms_kw": _twin_column(rt),
    }
    return cols, n


def _status_stats(F):
    return [AB.terms("st").field(F("status")).subAggregation(AB.stats("rt").field("response_time_ms"))]


def _hist_status(F):
    return [AB.dateHistogram("h").field("@timestamp").interval("1h").subAggregation(AB.terms("st").field(F("status")))]


def _host_status(F):
    return [AB.terms("hosts").field("host").size(8).subAggregation(
        AB.terms("st").field(F("status")).size(3).subAggregation(AB.avg("rt").field("response_time_ms")))]


def _rt_order(order, by_avg=False):
    def make(F):
        t = AB.terms("rt").field(F("response_time_ms")).size(5).order(order)
        if by_avg:
            t.subAggregation(AB.avg("b").field("status"))
        return [t]
    return make


def _three_levels(F):
    return [AB.terms("hosts").field("host").size(4).subAggregation(
        AB.terms("st").field(F("status")).size(3).subAggregation(
            AB.dateHistogram("h").field("@timestamp").interval("1h").subAggregation(AB.avg("a").field("response_time_ms"))))]


def _three_levels_long_outer(F):
    return [AB.terms("st").field(F("status")).size(3).subAggregation(
        AB.terms("hosts").field("host").size(4).subAggregation(AB.dateHistogram("h").field("@timestamp").interval("1h")))]


def _status_mdc0(F):
    return [AB.terms("st").field(F("status")).minDocCount(0).order(Order.term(True))]


TWIN_CASES = {
    "status_stats": (_status_stats, None, False),
    "hist_status": (_hist_status, None, False),
    "host_status_avg": (_host_status, None, False),
    "rt_count_asc": (_rt_order(Order.count(True)), None, False),
    "rt_term_desc": (_rt_order(Order.term(False)), None, False),
    "rt_by_avg": (_rt_order(Order.aggregation("b", False), True), None, False),
    "three_levels": (_three_levels, None, False),
    "three_levels_long_outer": (_three_levels_long_outer, None, False),
    "range_and_accept": (_status_stats, [QB.rangeQuery("response_time_ms").gte(20).lt(400)], True),
    "mdc0_under_term_filter": (_status_mdc0, [QB.termQuery("status", 404)], False),
}
TWIN_NAMES = {"st", "rt"}


@pytest.mark.parametrize("case", list(TWIN_CASES))
def test_twin_parity(engine, logs, case):
    cols, n = logs
    make, filters, with_accept = TWIN_CASES[case]
    accept = None
    if with_accept:
        accept = bits_from_mask(np.random.default_rng(3).random(n) < 0.7)
    twin = make(lambda f: f + "_kw")
    # the stats / avg leaves named "rt" / "b" carry no buckets: only terms keys are mapped back
    want = _map_back(O.run([(cols, n)], twin, filters=filters, accept=[accept] if with_accept else None), TWIN_NAMES)
    seg = engine.upload_segment({k: v for k, v in cols.items() if not k.endswith("_kw")}, n)
    plan = engine.plan(make(lambda f: f), filters=filters)
    try:
        plan.collect(seg, accept_bits=accept)
        res = plan.build()
        assert_same(res.to_dict(), want["shards"][0], "shard")
        assert_same(reduce([res]).to_dict(), want["reduced"], "reduced")
    finally:
        plan.close()
        seg.close()
    if case == "mdc0_under_term_filter":
        got = {b["key"]: b["doc_count"] for b in want["reduced"]["st"]["buckets"]}  # (== the GPU's, asserted above)
        assert set(got) == {200, 304, 404, 500} and got[200] == got[304] == got[500] == 0 and got[404] > 0


def test_breadth_first_replay_over_a_long_inner_field(engine, monkeypatch):
    """terms under terms collected breadth-first (the outer doc counts now, the inner buckets replayed at build for the
    outer winners) with a long inner field of more than 65,536 distinct values: the replay reads the numeric ordinals"""
    monkeypatch.setenv("ESGPU_DEFER_CELLS", "1")
    rng = np.random.default_rng(21)
    n = 200_000
    host = np.minimum(rng.zipf(1.3, size=n) - 1, 19).astype(np.uint32)
    big = np.minimum(rng.zipf(1.2, size=n) - 1, 69_999).astype(np.int64) * 3 - 1000
    big[:70_000] = np.arange(70_000, dtype=np.int64) * 3 - 1000
    cols = {"host": {"type": N.COL_ORD_U32, "values": host, "terms": ["host-%02d" % i for i in range(20)]},
            "big": _col(big), "big_kw": _twin_column(big)}
    make = lambda f: [AB.terms("hosts").field("host").size(5).subAggregation(AB.terms("rt").field(f).size(4))]  # noqa: E731
    want = _map_back(O.run([(cols, n)], make("big_kw")), {"rt"})
    seg = engine.upload_segment({k: cols[k] for k in ("host", "big")}, n)
    plan = engine.plan(make("big"))
    try:
        plan.collect(seg)
        assert plan.deferred_segments() == 1
        res = plan.build()
        assert_same(res.to_dict(), want["shards"][0], "shard")
        assert_same(reduce([res]).to_dict(), want["reduced"], "reduced")
    finally:
        plan.close()
        seg.close()


# ---- several segments ----
def test_multi_segment_needs_and_takes_an_ordinal_map(engine):
    rng = np.random.default_rng(11)
    sizes = [DOCS, 20_000, 9_000]
    sets = [np.array([-3, 0, 7, 1 << 33]), None, np.array([7, 8, 9, -(1 << 40)])]
    segs_cols, parts, masks = [], [], []
    for n, vs in zip(sizes, sets):
        m = rng.integers(0, 1000, size=n).astype(np.int64)
        c = {"m": _col(m)}
        if vs is not None:
            v = vs[rng.integers(0, len(vs), size=n)]
            c["v"] = _col(v)
            parts.append(v)
            masks.append(np.ones(n, dtype=bool))
        else:
            parts.append(np.zeros(n, dtype=np.int64))
            masks.append(np.zeros(n, dtype=bool))
        segs_cols.append((c, m))
    allv, allm = np.concatenate(parts), np.concatenate(masks)
    one = {"v_kw": _twin_column(allv, allm), "m": _col(np.concatenate([m for _, m in segs_cols]))}
    make = lambda f: [AB.terms("st").field(f).size(6).subAggregation(AB.avg("a").field("m"))]  # noqa: E731
    want = _map_back(O.run([(one, sum(sizes))], make("v_kw")), {"st"})
    segs = [engine.upload_segment(c, n) for (c, _), n in zip(segs_cols, sizes)]
    try:
        plan = engine.plan(make("v"))
        plan.collect(segs[0])
        plan.collect(segs[1])  # no such field: skipped
        with pytest.raises(N.EsGpuError) as e:
            plan.collect(segs[2])
        assert e.value.code == N.ERR_INVALID and "differently" in str(e.value) and "ordinal map" in str(e.value)
        plan.close()
        omap = engine.ordinal_map(segs, "v")
        assert omap.value_count == len(np.unique(allv[allm]))
        with pytest.raises(N.EsGpuError):
            omap.lookup("7")
        plan = engine.plan(make("v"))
        for sg in segs:
            plan.collect(sg)
        res = plan.build()
        assert_same(res.to_dict(), want["shards"][0], "shard")
        assert_same(reduce([res]).to_dict(), want["reduced"], "reduced")
        plan.close()
        omap.close()
    finally:
        for sg in segs:
            sg.close()


def test_three_shards_with_different_dictionaries(engine):
    rng = np.random.default_rng(12)
    n = DOCS
    shards = []
    for s in range(3):
        pool = np.unique(rng.integers(-40, 60, size=30)) * 1000 + 500
        w = 1.0 / (1.0 + np.arange(len(pool)))
        v = pool[rng.choice(len(pool), size=n, p=w / w.sum())]
        shards.append({"v": _col(v), "v_kw": _twin_column(v)})
    make = lambda f: [AB.terms("st").field(f).size(5).shardSize(8).showTermDocCountError(True)]  # noqa: E731
    want = _map_back(O.run([(c, n) for c in shards], make("v_kw"), number_of_shards=3), {"st"})
    segs = [engine.upload_segment({"v": c["v"]}, n) for c in shards]
    plans = [engine.plan(make("v"), number_of_shards=3) for _ in shards]
    try:
        for p, sg in zip(plans, segs):
            p.collect(sg)
        assert_same(build_reduce(plans).to_dict(), want["reduced"], "build_reduce")
        for p, sg in zip(plans, segs):
            p.reset()
            p.collect(sg)
        results = [p.build() for p in plans]
        for i, r in enumerate(results):
            assert_same(r.to_dict(), want["shards"][i], "shard %d" % i)
        red = reduce(results).to_dict()
        assert_same(red, want["reduced"], "reduced")
        assert red["st"]["sum_other_doc_count"] > 0 and red["st"]["doc_count_error_upper_bound"] > 0
    finally:
        for p in plans:
            p.close()
        for sg in segs:
            sg.close()


# ---- transport bytes and XContent ----
@pytest.mark.parametrize("show_err", [False, True])
def test_to_stream_bytes(engine, show_err):
    rng = np.random.default_rng(13)
    n = DOCS
    status = rng.choice([200, 200, 304, 404, 500], size=n).astype(np.int64)
    rt = rng.integers(0, 1000, size=n).astype(np.int64)
    seg = engine.upload_segment({"status": _col(status), "response_time_ms": _col(rt)}, n)
    plan = engine.plan([AB.terms("st").field("status").showTermDocCountError(show_err)
                        .subAggregation(AB.avg("rt").field("response_time_ms"))])
    try:
        plan.collect(seg)
        got = plan.build().to_stream()
    finally:
        plan.close()
        seg.close()
    keys, counts = np.unique(status, return_counts=True)
    kept, other = LT.top_k(keys, counts, 10, N.ORDER_COUNT_DESC)
    want = LT.w_vint(1) + LT.w_header("lterms", "st")
    want += struct.pack(">q", 0) + b"\xff" + LT.w_vint(2) + b"\x01\x04"  # docCountError, CompoundOrder(_count desc, _term asc)
    want += b"\x01\x01"                                                   # the field's formatter: RAW
    want += LT.w_vint(10) + LT.w_vint(10) + (b"\x01" if show_err else b"\x00") + LT.w_vlong(1) + LT.w_vlong(other)
    want += LT.w_vint(len(kept))
    for key, count in kept:
        want += struct.pack(">q", key) + LT.w_vlong(count) + (struct.pack(">q", 0) if show_err else b"")
        want += LT.w_vint(1) + LT.w_header("avg", "rt") + b"\x01\x01"
        want += struct.pack(">d", float(rt[status == key].sum())) + LT.w_vlong(count)
    assert got == want
    dec = LT.decode(got)[0]
    assert [b["key"] for b in dec["buckets"]] == [k for k, _ in kept]


def test_to_xcontent_five_docs(engine):
    ts = np.array([T0, T0 + 1000, T0, T0 + 86_400_000, T0 + 1000], dtype=np.int64)
    lv = np.array([3, 1, 3, 2, 3], dtype=np.int64)
    seg = engine.upload_segment({"@timestamp": _col(ts), "l": _col(lv)}, 5)
    plan = engine.plan([AB.terms("l").field("l"), AB.terms("ts").field("@timestamp")])
    try:
        plan.collect(seg)
        got = plan.build().to_xcontent()
    finally:
        plan.close()
        seg.close()
    head = '{"doc_count_error_upper_bound":0,"sum_other_doc_count":0,"buckets":['
    assert got == ('{"l":' + head + '{"key":3,"doc_count":3},{"key":1,"doc_count":1},{"key":2,"doc_count":1}]},"ts":' + head
                   + '{"key":1441065600000,"key_as_string":"2015-09-01T00:00:00.000Z","doc_count":2},'
                   '{"key":1441065601000,"key_as_string":"2015-09-01T00:00:01.000Z","doc_count":2},'
                   '{"key":1441152000000,"key_as_string":"2015-09-02T00:00:00.000Z","doc_count":1}]}}')


# ---- still refused ----
def test_refusals(engine):
    n = 1000
    rng = np.random.default_rng(14)
    offs = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    cols = {
        "multi": {"type": N.COL_I64, "values": np.sort(rng.integers(0, 50, size=(n, 2)), axis=1).reshape(-1).astype(np.int64),
                  "offsets": offs},
        "f": {"type": N.COL_F64, "values": rng.random(n)},
        "u": {"type": N.COL_U64, "values": rng.integers(0, 1 << 62, size=n, dtype=np.int64).astype(np.uint64)},
    }
    seg = engine.upload_segment(cols, n)
    try:
        for field, words in (("multi", "multi-valued long"), ("f", "double field"), ("u", "unsigned long")):
            plan = engine.plan([AB.terms("t").field(field)])
            with pytest.raises(N.UnsupportedOnGpu) as e:
                plan.collect(seg)
            assert words in str(e.value)
            plan.close()
    finally:
        seg.close()
