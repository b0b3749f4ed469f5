"""Request tables and column generators of the small-segment ladder (tests/test_gpu_small_segments.py runs them on the
GPU, tests/test_small_segment_cases_host.py pins the oracle at these sizes without one).

A refresh of a shard that is being written to leaves a segment of a handful of docs, which -- through global ordinals --
still carries the shard-wide dictionary.  Every column below is a pure function of (n, seed); nothing is a prefix of a
larger array, and the last doc is special: the tail of every sparse column alternates present / absent, so the last doc
is present at odd n and absent at even n.

The expected collect paths (include/esgpu.h:404-408) are restated from the gates of
elasticsearch_amd/csrc/esgpu_runtime.cpp; each function cites the lines it restates.
"""
from datetime import datetime, timedelta, timezone

import numpy as np

import long_terms_stream as LT
import oracle as O
import single_metric_stream as SM
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Order, QueryBuilders as QB
from elasticsearch_amd import _native as N
from helpers import bits_from_mask, synthetic_dict

# 4 and 8: docs per thread; 64: a bitset word and a wave; 256: the product kernels' workgroup; 2,048: kIterDocs and
# kB16Docs; 8,192: kBlockDocs; 16,384: two full blocks, 16,385 a third block holding one doc
LADDER = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 16384, 16385]
SEED = 20261020
T0 = 1441065600000  # 2015-09-01T00:00:00Z
HOUR = 3_600_000
DAY = 24 * HOUR
BOUNDARY = T0 + 5 * HOUR
MISSING = 0xFFFFFFFF
LAYOUTS = ("upload", "compact", "packed", "block")
HOST_TERMS = 1000
ORDERS = {"count_desc": Order.count(False), "count_asc": Order.count(True),
          "term_asc": Order.term(True), "term_desc": Order.term(False)}


def _rng(n, seed, tag):
    return np.random.default_rng([seed, n, tag])


def tail_mask(n, seed, tag, p):
    """present with probability p; the last min(17, n) docs alternate, doc n - 1 present exactly when n is odd"""
    m = _rng(n, seed, tag).random(n) < p
    k = min(17, n)
    m[n - k:] = np.arange(n - k, n) % 2 == 0
    return m


def mask_of(col, n):
    """the bool mask of a column's present bitset (all ones without one)"""
    if col.get("present") is None:
        return np.ones(n, dtype=bool)
    bits = np.unpackbits(np.ascontiguousarray(col["present"], dtype="<u8").view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


def timestamps(n, seed, wide=False):
    """sorted; dense: spread over min(4 h, 30 ms x n) centred on an hour boundary -- two hour keys from 2 docs up, and
    every run of 2,048 docs spans 2,048 x 30 ms + 30 ms < 2^16 ms (block deltas); wide: 40 days (32-bit deltas / i64 keys)"""
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    span = 40 * DAY if wide else min(4 * HOUR, 30 * n)
    start = BOUNDARY - span // 2
    ts = start + (np.arange(n, dtype=np.int64) * span) // n + _rng(n, seed, 1).integers(0, max(span // n, 1), size=n)
    ts[0] = start
    if n >= 2:
        ts[-1] = start + span - 1
    return ts.astype(np.int64)


def _sparse(values, mask):
    return {"type": N.COL_I64, "values": np.where(mask, values, 0).astype(np.int64), "present": bits_from_mask(mask)}


def _ords(values, mask=None):
    v = np.asarray(values).astype(np.uint32)
    if mask is not None:
        v = np.where(mask, v, MISSING).astype(np.uint32)
    return v


def csr(n, seed, tag, last, hi, unique):
    """0-3 values per doc (the last doc: `last`), ascending per doc; unique: a SortedSet (keyword ordinals)"""
    r = _rng(n, seed, tag)
    cnt = r.integers(0, 4, size=n)
    if n:
        cnt[-1] = last
    doc = np.repeat(np.arange(n), cnt)
    vals = r.integers(0, hi, size=int(cnt.sum()))
    order = np.lexsort((vals, doc))
    doc, vals = doc[order], vals[order]
    if unique and len(vals):
        keep = np.ones(len(vals), dtype=bool)
        keep[1:] = (doc[1:] != doc[:-1]) | (vals[1:] != vals[:-1])
        doc, vals = doc[keep], vals[keep]
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(doc, minlength=n), out=offs[1:])
    return vals, offs


def twin_column(values, mask=None):
    """the keyword twin of a long column (tests/test_gpu_long_terms.py): the oracle has no LongTerms"""
    values = np.asarray(values, dtype=np.int64)
    live = values if mask is None else values[mask]
    uniq = np.unique(live)
    ords = np.searchsorted(uniq, values).astype(np.uint32)
    if mask is not None:
        ords[~mask] = MISSING
    return {"type": N.COL_ORD_U32, "values": ords, "terms": [LT.twin_term(x) for x in uniq]}


SPECIAL_IDS = np.array([-(1 << 63), (1 << 63) - 1, -1, 0], dtype=np.int64)
_cols_cache = {}


def columns(n, seed=SEED, wide=False):
    """every column of the ladder's segment of n docs (cached: the reference and every layout share them)"""
    key = (n, seed, wide)
    if key in _cols_cache:
        return _cols_cache[key]
    r = _rng(n, seed, 2)
    ts = timestamps(n, seed, wide)
    host = ((np.minimum(r.zipf(1.2, size=n) - 1, HOST_TERMS - 1) * 37 + 11) % HOST_TERMS).astype(np.uint32)
    kw12 = r.integers(0, 12, size=n).astype(np.uint32)
    kw5 = r.integers(0, 5, size=n).astype(np.uint32)
    rt = r.integers(0, 1000, size=n).astype(np.int64)
    nbytes = r.integers(0, 100_000, size=n).astype(np.int64)
    status = r.choice([200, 200, 200, 304, 404, 500], size=n).astype(np.int64)
    price = np.round(r.random(n) * 500.0, 3)
    h = (r.integers(0, 1 << 62, size=n, dtype=np.int64).astype(np.uint64)) % np.uint64(1 << 40)
    pool = np.concatenate([SPECIAL_IDS, r.integers(-(1 << 63), (1 << 63) - 1, size=n // 3 + 1, dtype=np.int64, endpoint=True)])
    ids = pool[r.integers(0, len(pool), size=n)]
    ids[:min(n, len(SPECIAL_IDS))] = SPECIAL_IDS[:min(n, len(SPECIAL_IDS))]
    m_host, m_ts, m_rt = tail_mask(n, seed, 3, 0.7), tail_mask(n, seed, 4, 0.9), tail_mask(n, seed, 5, 0.6)
    none = np.zeros(n, dtype=bool)
    last = none.copy()
    last[n - 1:] = True
    host_dict, kw12_terms, kw5_terms = synthetic_dict("host"), ["k%02d" % i for i in range(12)], ["q%d" % i for i in range(5)]
    cols = {
        "host": {"type": N.COL_ORD_U32, "values": host, "terms_blob": host_dict},
        "kw12": {"type": N.COL_ORD_U32, "values": kw12, "terms": kw12_terms},
        "kw5": {"type": N.COL_ORD_U32, "values": kw5, "terms": kw5_terms},
        "@timestamp": {"type": N.COL_I64, "values": ts},
        "rt": {"type": N.COL_I64, "values": rt},
        "bytes": {"type": N.COL_I64, "values": nbytes},
        "status": {"type": N.COL_I64, "values": status},
        "price": {"type": N.COL_F64, "values": price},
        "h": {"type": N.COL_U64, "values": h},
        "ids": {"type": N.COL_I64, "values": ids},
        # sparse: 30 % missing ordinals, present bitsets on the timestamp and the metric
        "host_s": {"type": N.COL_ORD_U32, "values": _ords(host, m_host), "terms_blob": host_dict},
        "ts_s": _sparse(ts, m_ts),
        "rt_s": _sparse(rt, m_rt),
        # the two extremes: every doc missing the field, only the last doc present
        "host_none": {"type": N.COL_ORD_U32, "values": _ords(host, none), "terms_blob": host_dict},
        "host_last": {"type": N.COL_ORD_U32, "values": _ords(host, last), "terms_blob": host_dict},
        "kw12_none": {"type": N.COL_ORD_U32, "values": _ords(kw12, none), "terms": kw12_terms},
        "kw12_last": {"type": N.COL_ORD_U32, "values": _ords(kw12, last), "terms": kw12_terms},
        "ts_none": _sparse(ts, none), "ts_last": _sparse(ts, last),
        "rt_none": _sparse(rt, none), "rt_last": _sparse(rt, last),
        # the keyword twins of the long fields terms run over
        # value_count over a keyword column counts the docs that hold an ordinal: for the oracle, a long column present there
        "host_s_num": _sparse(np.zeros(n, dtype=np.int64), m_host),
        "status_kw": twin_column(status), "ids_kw": twin_column(ids), "@timestamp_kw": twin_column(ts),
    }
    for last_n in (0, 3):  # multi-valued: the last doc holds no value in one variant and three in the other
        tv, to = csr(n, seed, 6 + last_n, last_n, 60, True)
        cols["tags%d" % last_n] = {"type": N.COL_ORD_U32, "values": tv.astype(np.uint32), "offsets": to,
                                   "terms": ["t%02d" % i for i in range(60)]}
        nv, no = csr(n, seed, 16 + last_n, last_n, 1000, False)
        cols["nums%d" % last_n] = {"type": N.COL_I64, "values": nv.astype(np.int64), "offsets": no}
    _cols_cache[key] = cols
    return cols


_hc_dicts = {}


def hc_dict(T):
    """the term list of a high-cardinality dictionary, built once per module: (blob, offsets) of "u%07d" terms"""
    if T not in _hc_dicts:
        digits = np.arange(T)[:, None] // 10 ** np.arange(6, -1, -1) % 10
        out = np.empty((T, 8), dtype=np.uint8)
        out[:, 0] = ord("u")
        out[:, 1:] = digits + ord("0")
        _hc_dicts[T] = (out.reshape(-1), np.arange(0, 8 * (T + 1), 8, dtype=np.uint64))
    return _hc_dicts[T]


def hc_columns(n, T, seed=SEED):
    """few docs under a dictionary of T terms: spread ordinals (the first and the last term occur from 2 docs up), every
    doc missing, and all docs on one ordinal"""
    key = ("hc", n, T, seed)
    if key in _cols_cache:
        return _cols_cache[key]
    r = _rng(n, seed, 30 + T % 7)
    kw = r.integers(0, T, size=n).astype(np.uint32)
    kw[:1] = T - 1
    if n >= 2:
        kw[-1] = 0
    if n >= 4:
        kw[n // 2] = kw[n // 2 - 1]  # one term with two docs
    d = hc_dict(T)
    cols = {
        "kw": {"type": N.COL_ORD_U32, "values": kw, "terms_blob": d},
        "kw_none": {"type": N.COL_ORD_U32, "values": np.full(n, MISSING, dtype=np.uint32), "terms_blob": d},
        "kw_one": {"type": N.COL_ORD_U32, "values": np.full(n, T // 3, dtype=np.uint32), "terms_blob": d},
        "rt": {"type": N.COL_I64, "values": r.integers(0, 1000, size=n).astype(np.int64)},
    }
    _cols_cache[key] = cols
    return cols


def accept_mask(n, seed=SEED):
    """live docs: a quarter deleted, the tail alternating"""
    return tail_mask(n, seed, 9, 0.75)


# ---- the collect path a request takes, restated from esgpu_runtime.cpp -----------------------------------------------
LDS_PAIR, LDS_PI, LDS_MAX = 64 * 1024, 52 * 1024, 150 * 1024  # esgpu_runtime.cpp:3384-3390


def lds_bytes(T, W, met, vcnt=0, ocnt=None, pi=False):
    """collect_lds_bytes (esgpu_kernels.hip:128-148) with one copy"""
    r = lambda b: (b + 15) & ~15  # noqa: E731
    C = T * W
    if pi:
        b = r(8 * C) + (r(8 * C) if met >= 2 else 0)
        return b + (r(4 * T) if ocnt == "terms" else 0) + (r(4 * W) if ocnt == "hist" else 0) + 8 * 1024
    b = r(4 * C) + (r(4 * C) if vcnt else 0) + (r(8 * C) if met > 0 else 0) + (r(16 * C) if met >= 2 else 0)
    b += r(8 * C) if met >= 3 else 0
    return b + (r(4 * T) if ocnt == "terms" else 0) + (r(4 * W) if ocnt == "hist" else 0)


def grid_path(T, H, met, vcnt=0, ocnt=None, pi=False, key_window=True, zone_keys=0):
    """The single-valued grid kernel's form (esgpu_runtime.cpp:3415-3462, :3670): 1 the whole [T x H] grid in LDS, 2 a
    window over the key dimension (an affine key only, key_window; widened to the keys a zone block typically spans,
    zone_keys = zspan / interval, and no window at all once it holds every key), 0 the grid in global memory."""
    pair = LDS_PI if pi else LDS_PAIR
    f = lambda w: lds_bytes(T, w, met, vcnt, ocnt, pi)  # noqa: E731
    W, windowed = H, False
    if f(H) > pair:                       # :3429
        lds = f(H)
        if key_window and H >= 1:         # :3430-3437
            w = H
            while w > 1 and f(w) > pair:
                w = (w + 1) // 2
            W, windowed, lds = w, True, f(w)
        if lds > LDS_MAX:                 # :3438-3443
            return 0
    if windowed:                          # :3450-3461
        need = min(zone_keys + 2, H)
        if need > W:
            w2 = W
            while w2 < need and f(w2 + 1) <= LDS_MAX:
                w2 += 1
            if w2 >= H:
                windowed = False
    return 2 if windowed else 1


def key_count(values, mask, interval, offset=0):
    """keys of a fixed-interval histogram between the column's extremes (the grid's key dimension, :3098-3113)"""
    v = np.asarray(values)[mask] if mask is not None else np.asarray(values)
    if len(v) == 0:
        return 1
    return int((int(v.max()) - offset) // interval - (int(v.min()) - offset) // interval + 1)


def zone_keys(values, interval):
    """zspan / interval: the 90th percentile of the zone blocks' value ranges (build_zone_map, :441-452)"""
    v = np.asarray(values)
    if len(v) == 0:
        return 0
    rng = sorted(int(v[b:b + 8192].max()) - int(v[b:b + 8192].min()) for b in range(0, len(v), 8192))
    return rng[len(rng) * 9 // 10] // interval


def _packed(layout):
    return layout in ("packed", "block")


def path_const(p):
    return lambda n, layout, cols: p


def path_north_star(ranked, filtered, ts="@timestamp"):
    """terms(host){date_histogram(1h){stats}}: packed cells on the packed / block layouts (:3321-3345: a dense long metric
    spanning < 2^16 under 16-bit ordinals, over compact timestamps; a filter folds into one bitset); unfiltered, in count
    order and alone in the plan's first segment it is ranked (:3404-3413 -> 10); else the LDS grid or its key window"""
    def path(n, layout, cols):
        if _packed(layout) and ranked and not filtered:
            return 10
        v = cols[ts]["values"]
        return grid_path(HOST_TERMS, key_count(v, None, HOUR), 2, pi=_packed(layout), zone_keys=zone_keys(v, HOUR))
    return path


def path_sparse_grid(ords, ts, T=HOST_TERMS):
    """terms{date_histogram{stats}} with a present bitset on the metric (value counts split off: vcnt, :3104, :3115) and on
    the timestamps (outer counts per doc: OCNT_TERMS, :3106-3117); f64 cells whatever the layout (:3321-3322)"""
    def path(n, layout, cols):
        c = cols[ts]
        return grid_path(T, key_count(c["values"], mask_of(c, n), HOUR), 2, vcnt=1, ocnt="terms")
    return path


def path_long_terms(field):
    """terms(long field){stats}: T = the segment's distinct values (build_num_ords), no key dimension -- in LDS while the
    cells fit 150 KB (:3429-3443), in global memory above (terms over @timestamp from 5,486 distinct values up)"""
    def path(n, layout, cols):
        T = max(len(np.unique(cols[field]["values"])), 1)
        return grid_path(T, 1, 2, pi=_packed(layout), key_window=False)
    return path


def path_hotcold(field, shard_size, count_desc, filtered, accept):
    """A lone terms aggregation over more terms than LDS holds (:3498-3509, collect_hotcold :2432-2568).  Every ordinal
    that occurs is hot at these sizes (ensure_hc_stats :2176-2220: at most a few thousand distinct ordinals), so the
    request is settled by the hot slots -- 8 unfiltered, 9 under a filter or accept bits -- when it is in count order and
    shard_size terms occur (hc_defer_shape :2422-2431); else the postings form 7 without a filter (or with accept bits
    that clear few docs: sparse_dead, :4376-4380, always so within one bitset word) and the scatter form 6 with one."""
    def path(n, layout, cols):
        o = cols[field]["values"]
        distinct = len(np.unique(o[o != MISSING]))
        defer = count_desc and 1 <= shard_size <= distinct
        if defer:
            return 9 if (filtered or accept) else 8
        if filtered:
            return 6
        if accept:
            return 7 if n <= 64 else 6
        return 7
    return path


class Case:
    """One request of a group.  make(F): the request's builders with field names mapped through F (identity on the GPU;
    the oracle reads the keyword twin of the long fields in `long_fields`)."""

    def __init__(self, name, make, fields, path, filters=None, accept=False, wide=False, exact=True, ranked=True,
                 long_fields=(), long_names=(), sm=False, defer_env=False, hc=0, oracle_fields=None):
        self.name, self.make, self.fields, self.path = name, make, tuple(fields), path
        self.filters, self.accept, self.wide, self.exact, self.ranked = filters, accept, wide, exact, ranked
        self.long_fields, self.long_names, self.sm, self.defer_env, self.hc = set(long_fields), set(long_names), sm, defer_env, hc
        self.oracle_fields = dict(oracle_fields or {}, **{f: f + "_kw" for f in long_fields})

    def aggs(self):
        return self.make(lambda f: f)

    def twin_aggs(self):
        return self.make(lambda f: self.oracle_fields.get(f, f))

    def columns(self, n, seed=SEED):
        return hc_columns(n, self.hc, seed) if self.hc else columns(n, seed, self.wide)

    def upload_columns(self, n, seed=SEED):
        cols = self.columns(n, seed)
        return {f: cols[f] for f in self.fields}

    def accept_bits(self, n, seed=SEED):
        return bits_from_mask(accept_mask(n, seed)) if self.accept else None


def date_time(ms):
    """the default date format of a date field (strict_date_optional_time): 2015-09-01T00:00:00.000Z"""
    t = datetime(1970, 1, 1, tzinfo=timezone.utc) + timedelta(milliseconds=int(ms))
    return t.strftime("%Y-%m-%dT%H:%M:%S.") + "%03dZ" % (int(ms) % 1000)


def map_back(tree, names, dates=()):
    """a twin result with the keys of the terms aggregations in `names` turned back into longs; the buckets of those in
    `dates` (terms over a date field: LongTerms with the field's formatter) also carry key_as_string"""
    if isinstance(tree, dict):
        out = {}
        for k, v in tree.items():
            v = map_back(v, names, dates)
            if k in names and isinstance(v, dict) and "buckets" in v:
                for b in v["buckets"]:
                    b["key"] = LT.twin_long(b["key"])
                    if k in dates:
                        b["key_as_string"] = date_time(b["key"])
            out[k] = v
        return out
    if isinstance(tree, list):
        return [map_back(v, names, dates) for v in tree]
    return tree


_ref_cache = {}


def run_reference(case, segments, accept=None):
    """{"shards": [...], "reduced": ...} of the oracle over [(columns, n)] as one shard each, mapped back from the
    request's twins (stats for sum / min / max / value_count, keyword columns for long terms)"""
    aggs = case.twin_aggs()
    res = O.run(segments, SM.twin(aggs) if case.sm else aggs, filters=case.filters, accept=accept)
    if case.sm:
        res = {"shards": [SM.untwin(s, aggs) for s in res["shards"]], "reduced": SM.untwin(res["reduced"], aggs)}
    if case.long_names:
        dates = case.long_names if "@timestamp" in case.long_fields else ()
        res = {"shards": [map_back(s, case.long_names, dates) for s in res["shards"]],
               "reduced": map_back(res["reduced"], case.long_names, dates)}
    return res


def reference(case, n, seed=SEED):
    """the oracle's result of a case at n docs, computed once and shared by every layout"""
    key = (case.name, n, seed)
    if key not in _ref_cache:
        bits = case.accept_bits(n, seed)
        _ref_cache[key] = run_reference(case, [(case.columns(n, seed), n)], [bits] if bits is not None else None)
    return _ref_cache[key]


# ---- the request groups ------------------------------------------------------------------------------------------------
def _ns(F, ords="host", ts="@timestamp", rt="rt", leaf=None):
    leaf = leaf if leaf is not None else AB.stats("rt").field(F(rt))
    return [AB.terms("hosts").field(F(ords)).size(10).subAggregation(
        AB.dateHistogram("per_hour").field(F(ts)).interval("1h").subAggregation(leaf))]


def c5_filters():
    return [QB.termQuery("status", 200), QB.rangeQuery("bytes").gte(1024).lte(65536)]


NS_FIELDS = ("host", "@timestamp", "rt", "status", "bytes")


def group_a(wide=False):
    """(the 40-day variants build a [1,000 terms x 960 keys] grid per collect: one group each, so no test of the ladder
    runs much longer than its neighbours)"""
    w = "_40d" if wide else ""
    return [Case("a_ranked" + w, _ns, NS_FIELDS, path_north_star(True, False), wide=wide),
            Case("a_every_term" + w, _ns, NS_FIELDS, path_north_star(False, False), wide=wide, ranked=False),
            Case("a_filtered" + w, _ns, NS_FIELDS, path_north_star(True, True), wide=wide, filters=c5_filters())]


def _dh(F, ts="@timestamp"):
    return AB.dateHistogram("d").field(F(ts)).interval("1h")


def path_hist(ts="@timestamp", met=2, interval=HOUR, offset=0, vcnt=0):
    def path(n, layout, cols):
        c = cols[ts]
        return grid_path(1, key_count(c["values"], mask_of(c, n), interval, offset), met, vcnt=vcnt,
                         zone_keys=zone_keys(c["values"], interval))
    return path


def group_b():
    f = ("@timestamp", "rt")
    four = lambda F: [AB.sum("s").field(F("rt")), AB.min("mn").field(F("rt")), AB.max("mx").field(F("rt")),  # noqa: E731
                      AB.count("vc").field(F("rt"))]

    def with_four(F):
        d = _dh(F)
        for leaf in four(F):
            d.subAggregation(leaf)
        return [d]
    return [
        Case("b_extended_stats", lambda F: [_dh(F).subAggregation(AB.extendedStats("e").field(F("rt")))], f, path_hist(met=3)),
        Case("b_extended_stats_40d", lambda F: [_dh(F).subAggregation(AB.extendedStats("e").field(F("rt")))], f,
             path_hist(met=3), wide=True),
        Case("b_four_single_values", with_four, f, path_hist(met=2), sm=True),
        Case("b_histogram_avg", lambda F: [AB.histogram("h").field(F("rt")).interval(50).offset(7).subAggregation(
            AB.avg("a").field(F("bytes")))], ("rt", "bytes"), path_hist("rt", 1, 50, 7)),
        Case("b_min_doc_count_0", lambda F: [_dh(F).minDocCount(0).extendedBounds(BOUNDARY - 3 * HOUR, BOUNDARY + 3 * HOUR)
                                             .subAggregation(AB.stats("s").field(F("rt")))], f, path_hist(met=2)),
    ]


def group_c():
    out = []
    for field, T in (("kw12", 12), ("host", HOST_TERMS)):
        out.append(Case("c_%s_stats" % field, lambda F, field=field: [AB.terms("t").field(F(field)).size(10).minDocCount(0)
                        .subAggregation(AB.stats("s").field(F("rt")))], (field, "rt"),
                        lambda n, layout, cols, T=T: grid_path(T, 1, 2, pi=_packed(layout), key_window=False)))
        for oname, order in ORDERS.items():
            out.append(Case("c_%s_%s" % (field, oname), lambda F, field=field, order=order: [
                AB.terms("t").field(F(field)).size(10).minDocCount(0).order(order)], (field,),
                lambda n, layout, cols, T=T: grid_path(T, 1, 0, key_window=False)))
    return out


def group_d():
    f = ("host_s", "ts_s", "rt_s", "host_none", "host_last", "ts_none", "ts_last", "rt_none", "rt_last", "kw12_none", "kw12_last")
    ns = lambda o, t, m: (lambda F: _ns(F, o, t, m))  # noqa: E731
    return [
        Case("d_sparse", ns("host_s", "ts_s", "rt_s"), f, path_sparse_grid("host_s", "ts_s")),
        Case("d_sparse_accept", ns("host_s", "ts_s", "rt_s"), f, path_sparse_grid("host_s", "ts_s"), accept=True),
        Case("d_all_missing", ns("host_none", "ts_none", "rt_none"), f, path_sparse_grid("host_none", "ts_none")),
        Case("d_only_last", ns("host_last", "ts_last", "rt_last"), f, path_sparse_grid("host_last", "ts_last")),
        Case("d_only_last_accept", ns("host_last", "ts_last", "rt_last"), f, path_sparse_grid("host_last", "ts_last"), accept=True),
        Case("d_hist_sparse", lambda F: [_dh(F, "ts_s").subAggregation(AB.extendedStats("e").field(F("rt_s")))], f,
             path_hist("ts_s", 3, vcnt=1)),
        Case("d_hist_all_missing", lambda F: [_dh(F, "ts_none").subAggregation(AB.stats("e").field(F("rt_none")))], f,
             path_hist("ts_none", 2, vcnt=1)),
        Case("d_hist_only_last", lambda F: [_dh(F, "ts_last").subAggregation(AB.stats("e").field(F("rt_last")))], f,
             path_hist("ts_last", 2, vcnt=1)),
        Case("d_terms_missing_mdc0", lambda F: [AB.terms("t").field(F("kw12_none")).size(20).minDocCount(0)
                                                .subAggregation(AB.avg("a").field(F("rt_last")))], f,
             lambda n, layout, cols: grid_path(12, 1, 1, vcnt=1, key_window=False)),
        Case("d_terms_only_last", lambda F: [AB.terms("t").field(F("kw12_last")).size(20)
                                             .subAggregation(AB.stats("a").field(F("rt_s")))], f,
             lambda n, layout, cols: grid_path(12, 1, 2, vcnt=1, key_window=False)),
    ]


def group_e():
    return [
        Case("e_terms_price", lambda F: [AB.terms("t").field(F("host")).size(10).subAggregation(AB.stats("p").field(F("price")))],
             ("host", "price"), lambda n, layout, cols: grid_path(HOST_TERMS, 1, 2, key_window=False), exact=False),
        Case("e_terms_price_extended", lambda F: [AB.terms("t").field(F("kw12")).size(12).subAggregation(
            AB.extendedStats("p").field(F("price")))], ("kw12", "price"),
            lambda n, layout, cols: grid_path(12, 1, 3, key_window=False), exact=False),
        Case("e_hist_price", lambda F: [_dh(F).subAggregation(AB.stats("p").field(F("price")))], ("@timestamp", "price"),
             path_hist(met=2), exact=False),
        Case("e_hist_price_avg_40d", lambda F: [_dh(F).subAggregation(AB.avg("p").field(F("price")))], ("@timestamp", "price"),
             path_hist(met=1), exact=False, wide=True),
    ]


def group_f():
    """multi-valued columns: every request takes the CSR kernel (:3055-3059, :3279-3286 -> collect_multi, 5)"""
    out = []
    five = path_const(5)
    for k in (0, 3):
        tags, nums = "tags%d" % k, "nums%d" % k
        f = (tags, nums, "rt", "host_s", "rt_s", "@timestamp")

        def singles(F, nums=nums):
            return [AB.sum("s").field(F(nums)), AB.min("mn").field(F(nums)), AB.max("mx").field(F(nums)), AB.count("vc").field(F(nums))]
        out += [
            Case("f%d_terms_tags" % k, lambda F, tags=tags: [AB.terms("t").field(F(tags)).size(10).subAggregation(
                AB.stats("s").field(F("rt")))], f, five),
            Case("f%d_terms_tags_mdc0" % k, lambda F, tags=tags: [AB.terms("t").field(F(tags)).size(60).minDocCount(0)
                                                                  .order(Order.term(True))], f, five),
            Case("f%d_stats_nums" % k, lambda F, nums=nums: [AB.stats("s").field(F(nums))], f, five),
            # (the lone root value_count is a pipeline of its own, collected last through its product -- a dense 16-bit
            # metric, value_count_metric :4019-4047 -- by the single-valued kernel: the path reported is that launch's)
            Case("f%d_singles_nums" % k, singles, f, path_const(1), sm=True),
            Case("f%d_sum_min_max_nums" % k, lambda F, nums=nums: [AB.sum("s").field(F(nums)), AB.min("mn").field(F(nums)),
                                                                  AB.max("mx").field(F(nums))], f, five, sm=True),
            Case("f%d_hist_nums" % k, lambda F, nums=nums: [_dh(F).subAggregation(AB.stats("s").field(F(nums)))], f, five),
            # the value-count product's three sources: CSR offsets, ordinals with missing, a present bitset -- each a lone
            # value_count under a bucket aggregation (a dense 16-bit metric: the single-valued kernels read the product)
            Case("f%d_vc_csr" % k, lambda F, nums=nums: [AB.terms("t").field(F("host_s")).size(10).subAggregation(
                AB.count("vc").field(F(nums)))], f, lambda n, layout, cols: grid_path(HOST_TERMS, 1, 1, key_window=False), sm=True),
        ]
    f = ("host_s", "rt_s", "@timestamp", "kw12")
    out += [
        Case("f_vc_ord", lambda F: [_dh(F).subAggregation(AB.count("vc").field(F("host_s")))], f, path_hist(met=1), sm=True,
             oracle_fields={"host_s": "host_s_num"}),
        Case("f_vc_present", lambda F: [AB.terms("t").field(F("kw12")).size(12).subAggregation(AB.count("vc").field(F("rt_s")))], f,
             lambda n, layout, cols: grid_path(12, 1, 1, key_window=False), sm=True),
        Case("f_vc_present_root", lambda F: [AB.count("vc").field(F("rt_s"))], f, lambda n, layout, cols: 1, sm=True),
    ]
    return out


def group_g():
    out = []
    for field in ("h", "rt", "host"):
        for thr in (100, 40000):
            out.append(Case("g_root_%s_%d" % (field, thr), lambda F, field=field, thr=thr: [
                AB.cardinality("c").field(F(field)).precisionThreshold(thr)], (field,), path_const(3)))  # collect_hll, :4361
            out.append(Case("g_terms_%s_%d" % (field, thr), lambda F, field=field, thr=thr: [
                AB.terms("t").field(F("kw12")).size(12).subAggregation(AB.cardinality("c").field(F(field)).precisionThreshold(thr))],
                ("kw12", field), lambda n, layout, cols: grid_path(12, 1, 0, key_window=False)))
    return out


def group_h():
    out = []
    for field in ("status", "ids", "@timestamp"):
        for oname, order in ORDERS.items():
            out.append(Case("h_%s_%s" % (field.strip("@"), oname), lambda F, field=field, order=order: [
                AB.terms("t").field(F(field)).size(7).order(order).subAggregation(AB.stats("s").field(F("rt")))],
                (field, "rt"), path_long_terms(field), long_fields=(field,), long_names=("t",)))
    return out


HC_TERMS = (70_000, 300_000)


def group_i(T):
    out = []
    f = ("kw", "kw_none", "kw_one", "rt")
    rf = lambda: [QB.rangeQuery("rt").gte(100).lt(800)]  # noqa: E731
    for field in ("kw", "kw_none", "kw_one"):
        for oname, order in (("count", Order.count(False)), ("term", Order.term(True))):
            mk = lambda F, field=field, order=order: [AB.terms("t").field(F(field)).size(2).shardSize(2).order(order)]  # noqa: E731
            cd = oname == "count"
            out += [Case("i%d_%s_%s" % (T, field, oname), mk, f, path_hotcold(field, 2, cd, False, False), hc=T),
                    Case("i%d_%s_%s_range" % (T, field, oname), mk, f, path_hotcold(field, 2, cd, True, False), hc=T, filters=rf()),
                    Case("i%d_%s_%s_accept" % (T, field, oname), mk, f, path_hotcold(field, 2, cd, False, True), hc=T, accept=True)]
    return out


def group_j():
    f = ("host", "kw12", "kw5", "@timestamp", "rt")
    two = lambda F: [AB.terms("o").field(F("host")).size(5).subAggregation(AB.terms("i").field(F("kw12")).size(3))]  # noqa: E731
    two_stats = lambda F: [AB.terms("o").field(F("kw12")).size(5).subAggregation(  # noqa: E731
        AB.terms("i").field(F("host")).size(3).subAggregation(AB.stats("s").field(F("rt"))))]
    three = lambda F: [AB.terms("A").field(F("kw12")).size(6).subAggregation(  # noqa: E731
        AB.terms("B").field(F("kw5")).size(4).subAggregation(
            AB.dateHistogram("d").field(F("@timestamp")).interval("1h").subAggregation(AB.stats("s").field(F("rt")))))]
    # [outer x inner] cells with the inner ordinals as the key dimension (no key window: :3430) and outer counts per doc
    # (:3106-3117); collected breadth-first (:3028-3047) only the outer counts are launched: [T] cells -- in LDS either way
    p2 = lambda n, layout, cols: grid_path(HOST_TERMS, 12, 0, ocnt="terms", key_window=False)  # noqa: E731
    p2d = lambda n, layout, cols: grid_path(HOST_TERMS, 1, 0, key_window=False)  # noqa: E731
    p2s = lambda n, layout, cols: grid_path(12, HOST_TERMS, 2, ocnt="terms", key_window=False)  # noqa: E731
    p2sd = lambda n, layout, cols: grid_path(12, 1, 0, key_window=False)  # noqa: E731
    p3 = lambda n, layout, cols: 1  # noqa: E731 -- 60 composite ordinals x 2 keys
    return [Case("j_two", two, f, p2), Case("j_two_deferred", two, f, p2d, defer_env=True),
            Case("j_two_stats", two_stats, f, p2s), Case("j_two_stats_deferred", two_stats, f, p2sd, defer_env=True),
            Case("j_three", three, f, p3), Case("j_three_deferred", three, f, p3, defer_env=True)]


GROUPS = {"a": group_a, "a40d_ranked": lambda: group_a(True)[0:1], "a40d_every_term": lambda: group_a(True)[1:2],
          "a40d_filtered": lambda: group_a(True)[2:3], "b": group_b, "c": group_c, "d": group_d, "e": group_e, "f": group_f, "g": group_g, "h": group_h,
          "i70000": lambda: group_i(70_000), "i300000": lambda: group_i(300_000), "j": group_j}

# ---- many small segments in one plan -----------------------------------------------------------------------------------
MULTI_SIZES = [1, 8193, 0, 5, 64, 2049, 3]


def sub_dictionary(col, k, n_terms):
    """segment k's own dictionary of a keyword column over the shard-wide terms "name-%04d": the terms its docs hold plus
    every term whose number is k modulo 3 -- the segments' dictionaries differ and overlap"""
    vals = col["values"]
    used = np.unique(vals[vals != MISSING])
    keep = np.union1d(used, np.arange(k % 3, n_terms, 3)).astype(np.int64)
    local = np.full(n_terms, MISSING, dtype=np.uint32)
    local[keep] = np.arange(len(keep), dtype=np.uint32)
    out = np.where(vals == MISSING, MISSING, local[np.minimum(vals, n_terms - 1)]).astype(np.uint32)
    return out, keep


def concat_columns(parts, sizes, fields, absent=()):
    """the segments' docs as one segment: values and CSR offsets concatenated, present bitsets joined; a field absent
    from a segment (absent: {(segment index, field)}) is missing in its docs"""
    one = {}
    for f in fields:
        first = parts[0][f]
        if first.get("offsets") is not None:
            counts = np.concatenate([np.diff(p[f]["offsets"].astype(np.int64)) for p in parts])
            offs = np.zeros(len(counts) + 1, dtype=np.uint64)
            np.cumsum(counts, out=offs[1:])
            c = dict(first, values=np.concatenate([p[f]["values"] for p in parts]), offsets=offs)
        else:
            c = dict(first, values=np.concatenate([p[f]["values"] for p in parts]))
            masks = [mask_of(p[f], n) & ((k, f) not in absent) for k, (p, n) in enumerate(zip(parts, sizes))]
            if first["type"] != N.COL_ORD_U32 and (any(p[f].get("present") is not None for p in parts) or
                                                    any(kf[1] == f for kf in absent)):
                c["present"] = bits_from_mask(np.concatenate(masks))
                c["values"] = np.where(np.concatenate(masks), c["values"], 0).astype(c["values"].dtype)
        one[f] = c
    return one


def multi_segments(case, order, seed=SEED, ts_fields=("@timestamp", "ts_s"), dict_fields=(), absent=()):
    """The columns of MULTI_SIZES segments in `order` (indices into MULTI_SIZES) and their concatenation for the oracle.
    Segment k's timestamps are shifted by whole hours, alternately back and forth, so the grid grows along the key axis
    both ways; the keyword columns in dict_fields get per-segment dictionaries (sub_dictionary), the concatenation the
    union of them.  Returns ([(upload columns, n)], (oracle columns, total))."""
    parts, sizes, uploads = [], [], []
    for pos, k in enumerate(order):
        n = MULTI_SIZES[k]
        src = columns(n, seed + 1 + k, case.wide)
        cols = {f: dict(src[f]) for f in set(case.fields) | {f + "_kw" for f in case.long_fields}}
        shift = ((pos + 1) // 2) * (2 * HOUR) * (1 if pos % 2 else -1)
        for f in ts_fields:
            if f in cols:
                cols[f]["values"] = np.where(mask_of(cols[f], n), cols[f]["values"] + shift, 0).astype(np.int64)
        parts.append(cols)
        sizes.append(n)
    unions = {}
    for f in dict_fields:
        n_terms = {"host": HOST_TERMS, "host_s": HOST_TERMS, "tags0": 60, "tags3": 60}[f]
        fmt = "t%02d" if f.startswith("tags") else "host-%04d"
        keeps = []
        for k, cols in zip(order, parts):
            local, keep = sub_dictionary(cols[f], k, n_terms)
            cols[f + "#global"] = cols[f]["values"]
            cols[f] = dict({a: b for a, b in cols[f].items() if a != "terms_blob"}, values=local, terms=[fmt % i for i in keep])
            keeps.append(keep)
        unions[f] = np.unique(np.concatenate(keeps)).astype(np.int64)
    for cols, n in zip(parts, sizes):
        uploads.append(({f: cols[f] for f in case.fields if (len(uploads), f) not in absent}, n))
    # the oracle's one segment
    glob = []
    for cols in parts:
        g = {}
        for f, c in cols.items():
            if f.endswith("#global"):
                continue
            if f in dict_fields:
                union = unions[f]
                to_union = np.full(int(union.max()) + 1 if len(union) else 1, MISSING, dtype=np.uint32)
                to_union[union] = np.arange(len(union), dtype=np.uint32)
                gv = cols[f + "#global"]
                fmt = "t%02d" if f.startswith("tags") else "host-%04d"
                c = dict({a: b for a, b in c.items() if a != "terms_blob"}, values=np.where(gv == MISSING, MISSING, to_union[np.minimum(gv, len(to_union) - 1)]).astype(np.uint32),
                         terms=[fmt % i for i in union])
            g[f] = c
        glob.append(g)
    fields = [f for f in glob[0]]
    one = concat_columns(glob, sizes, [f for f in fields if not f.endswith("_kw")], absent)
    for f in case.long_fields:  # the twin of the concatenated long column
        one[f + "_kw"] = twin_column(one[f]["values"], mask_of(one[f], sum(sizes)) if one[f].get("present") is not None else None)
    return uploads, (one, sum(sizes))
