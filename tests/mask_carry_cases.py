"""The crafted segment and the request tables for the mask collects -- range (collect path 11), filters (12) and a
date_histogram under either (13) -- when one workgroup walks several zone blocks (tests/test_gpu_mask_block_carry.py and
tests/test_gpu_mask_float_exact.py run them on the GPU with ESGPU_DEBUG_BPW over BPWS; tests/test_mask_carry_cases_host.py
proves from the tables below, without a GPU, that every block-to-block event those kernels know occurs).

One segment of 13 zone blocks, 12 * 8192 + 5001 docs.  The clause, range and metric columns are the synthetic shard's
(helpers.synthetic_columns) plus a few crafted ones; the timestamps are built block by block from BLOCKS, a table of the
grid rows (hours after T0) each block holds.  They are not globally sorted: a later block lies below an earlier one.

The references never run the code under test (run_plan, at the end, is the GPU files' shared runner).  They are the
bucket doc masks of range_ref / filters_ref / mask_hist_ref and, per bucket, the oracle's result for the bucket's
children at top level with accept = the bucket's mask.
"""
import copy
import math

import numpy as np

import filters_ref as FR
import mask_hist_ref as MH
import oracle as O
import range_ref as RR
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import _native as N
from helpers import assert_same, assert_same_exact, bits_from_mask, synthetic_columns

BLOCK = 8192
NB = 13
NDOCS = 12 * BLOCK + 5001
BPWS = (1, 2, 3, 4, 5, 13, 14)  # every small range length, a shorter last workgroup, one workgroup exactly, above n_blocks
SLOTS = 4                       # kMhSlots: the grid rows a workgroup's cells stand for at a time
T0 = 1441065600000              # 2015-09-01T00:00:00Z
HOUR = 3600000
ROWS = 600                      # H: the grid rows of the segment's keys
FIELDS = ("status", "response_time_ms", "bytes", "price")
RT, TS = "response_time_ms", "@timestamp"
INF = math.inf

# the grid rows of each zone block's timestamps: single -- one key, no timestamp is read; multi / shuffled -- every doc a
# row of the set, drawn at random (every wave meets every row of a small set); nokey -- no doc has a timestamp
BLOCKS = [
    ("single", (10,)),
    ("single", (10,)),                        # the same row again
    ("single", (13,)),                        # the window's last slot
    ("single", (14,)),                        # one past it
    ("multi", (15, 16, 17)),                  # inside the window the block before opened; a sparse present bitset
    ("nokey", ()),
    ("single", (16,)),                        # still that window; a sparse present bitset
    ("multi", (100, 101, 102, 103, 104)),     # five rows: the fifth goes straight to the grid
    ("single", (104,)),                       # inside the block's span, outside its window
    ("shuffled", tuple(range(200, 550))),
    ("single", (300,)),                       # inside the block's span, outside its window
    ("multi", (0, 1, 2, 3)),                  # below the window, four rows, row 0
    ("multi", (ROWS - 2, ROWS - 1)),          # the partial last block; two slots of its window stand for no row
]
SPARSE_TS = (4, 6)  # blocks whose timestamps carry a sparse present bitset (with whole clear 64-bit words)
assert len(BLOCKS) == NB


def block_slice(b, n=NDOCS):
    return slice(b * BLOCK, min((b + 1) * BLOCK, n))


def timestamps():
    """-> ([NDOCS] int64, [NDOCS] bool present) from BLOCKS"""
    rng = np.random.default_rng(20261021)
    ts = np.empty(NDOCS, dtype=np.int64)
    pres = np.ones(NDOCS, dtype=bool)
    for b, (kind, rows) in enumerate(BLOCKS):
        sl = block_slice(b)
        n = sl.stop - sl.start
        if kind == "nokey":
            pres[sl] = False
            continue
        r = np.asarray(rows)[rng.integers(0, len(rows), size=n)]
        if b in SPARSE_TS:
            p = rng.random(n) < 0.65
            p[64:128] = False
            p[n - 64:] = False
            if b == 6:
                p[:64] = False
            pres[sl] = p
        live = np.nonzero(pres[sl])[0]
        r[live[:len(rows)]] = rows  # every row of the set occurs among the docs that have a timestamp
        ts[sl] = T0 + r * HOUR + (np.arange(n) % 997) * 1000
    ts[~pres] = T0 + 5000 * HOUR  # stored values under absent docs are not values
    return ts, pres


# ---- the requests' bucket tables ---------------------------------------------------------------------------------------
CLASSES = [("c0", QB.rangeQuery(RT).lt(50)), ("c1", QB.rangeQuery(RT).gte(50).lt(100)), ("c2", QB.rangeQuery(RT).gte(100).lt(250)),
           ("c3", QB.rangeQuery(RT).gte(250).lt(500))]  # with the other bucket: a partition
MIXED = [("fast", QB.rangeQuery(RT).lt(100)), ("ok", QB.termQuery("status", 200)),
         ("big_ok", [QB.termQuery("status", 200), QB.rangeQuery("bytes").gte(100000)]), ("mid", QB.rangeQuery(RT).gte(50).lte(600)),
         ("tail", QB.rangeQuery(RT).gte(990))]  # overlapping
RANGES = [("lo", -INF, 100.0), ("mid", 50.0, 500.0), (None, 500.0, INF), ("empty", 300.0, 300.0), ("tail", 990.0, INF)]
TAIL_LO = 990  # the docs of the "tail" buckets: response_time_ms >= 990
ZONES = 65     # the crafted `zone` column: 5 values per block, zone = 5 * block + doc % 5
# 64 ranges: one per zone up to 61 (each in one block only; the last, bucket 63, in the partial block), every doc, a middle
RANGES64 = [(None, float(k), float(k + 1)) for k in range(62)] + [("all", -INF, INF), ("middle", 20.0, 45.0)]
# 63 filters and the other bucket (bit 63: zones 63 and 64, the partial block)
FILTERS63 = [("z%02d" % k, QB.termQuery("zone_kw", "z%02d" % k)) for k in range(62)] + [("wide", QB.rangeQuery("zone").lt(62))]
CODES = [(None, 0.0, 500.0), (None, 500.0, 1000.0), (None, 250.0, 750.0), (None, -INF, INF), (None, 990.0, INF)]
QUERY = [QB.termQuery("status", 200), QB.rangeQuery("bytes").gte(500)]
SPECIAL = ("inf", "inf_ninf", "nan", "subnormal", "mixed")


def ord_lookup(field, term):
    """the ordinal of a keyword term of the crafted columns (zone_kw: "z%02d" -> its number), -1 when absent"""
    assert field == "zone_kw"
    k = int(term[1:])
    return k if 0 <= k < ZONES else -1


def special_column(rng, n, kind):
    """the five kinds of tests/test_gpu_float_parity._special_column"""
    v = rng.random(n) * 1000.0
    if kind == "inf":
        v[rng.integers(0, n, 20)] = math.inf
    elif kind == "inf_ninf":
        v[rng.integers(0, n, 20)] = math.inf
        v[rng.integers(0, n, 20)] = -math.inf
    elif kind == "nan":
        v[rng.integers(0, n, 5)] = math.nan
    elif kind == "subnormal":
        v = (rng.random(n) - 0.3) * 2.0 ** -1040
    elif kind == "mixed":
        v[rng.integers(0, n, 50)] = -0.0
        v[rng.integers(0, n, 5000)] *= -1.0
        v[rng.integers(0, n, 100)] = 2.0 ** -1070
    return v


_cache = {}


def _i64(v, present=None):
    c = {"type": N.COL_I64, "values": np.ascontiguousarray(v, dtype=np.int64)}
    if present is not None:
        c["present"] = bits_from_mask(present)
    return c


def _f64(v):
    return {"type": N.COL_F64, "values": np.ascontiguousarray(v, dtype=np.float64)}


def main_columns():
    """every column of the 13-block segment (computed once, shared, never modified)"""
    if "main" in _cache:
        return _cache["main"]
    n = NDOCS
    base = synthetic_columns(FIELDS, n)
    c = {f: {"type": base[f]["type"], "values": base[f]["values"]} for f in FIELDS}
    ts, pres = timestamps()
    c[TS] = _i64(ts, pres)
    rng = np.random.default_rng(77)
    doc = np.arange(n)
    zone = 5 * (doc // BLOCK) + doc % 5
    c["zone"] = _i64(zone)
    c["zone_kw"] = {"type": N.COL_ORD_U32, "values": zone.astype(np.uint32), "terms": ["z%02d" % k for k in range(ZONES)]}
    # the metric of the 64-bucket requests: bytes with the segment's minimum in the first block and its maximum in the last
    m = base["bytes"]["values"].astype(np.int64).copy()
    m[3] = -5
    m[n - 4] = 10_000_000  # (zone 61: inside the widest filter too)
    c["m"] = _i64(m)
    # a sparse metric: half the docs, no value at all in block 7, a whole clear word in block 2
    sp = rng.random(n) < 0.5
    sp[block_slice(7)] = False
    sp[2 * BLOCK + 128:2 * BLOCK + 192] = False
    sp[-17:] = np.arange(17) % 2 == 0
    c["sz"] = _i64(np.where(sp, base["bytes"]["values"], 0), sp)
    # a multi-valued range field: 0-4 values per doc
    cnt = rng.integers(0, 5, size=n)
    cv = rng.integers(0, 1000, size=int(cnt.sum()))
    order = np.lexsort((cv, np.repeat(doc, cnt)))
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(cnt, out=offs[1:])
    c["codes"] = {"type": N.COL_I64, "values": cv[order].astype(np.int64), "offsets": offs}
    # exact sums and special values: sums past 2^53 from a 10^12 base, and the five special kinds
    c["big"] = _i64(10 ** 12 + rng.integers(0, 999, size=n))
    tail = base[RT]["values"] >= TAIL_LO
    for k, kind in enumerate(SPECIAL):
        v = special_column(np.random.default_rng(200 + k), n, kind)
        if kind == "mixed":  # -0.0 against 0.0 alone in the "tail" buckets
            v[tail] = np.where(np.arange(int(tail.sum())) % 3 == 1, -0.0, 0.0)
        c["sp_" + kind] = _f64(v)
    _cache["main"] = c
    return c


def _sorted_ts(n, rows):
    """[n] timestamps in runs of the given rows (odd run lengths: the key changes inside a lane's four docs)"""
    edges = [n * (i + 1) // len(rows) | 1 for i in range(len(rows) - 1)]
    key = np.searchsorted(np.asarray(edges), np.arange(n), side="right")
    return (T0 + np.asarray(rows)[key] * HOUR + (np.arange(n) % 997) * 1000).astype(np.int64)


def tail_columns():
    """a 2-block segment whose keys lie above the main segment's (the grid grows, whichever comes first)"""
    if "tail" not in _cache:
        n = BLOCK + 300
        base = synthetic_columns(FIELDS, n, shard=1)
        c = {f: {"type": base[f]["type"], "values": base[f]["values"]} for f in FIELDS}
        c[TS] = _i64(_sorted_ts(n, (650, 651, 652)))
        _cache["tail"] = (c, n)
    return _cache["tail"]


def v_columns(which):
    """the plan-level cases' segments: the metric field `v` small in one (2 blocks: the double-double rule stays off)
    and 10^12-based in the other (the 13 blocks: the rule turns on)"""
    if which == "big":
        main = main_columns()
        c = {f: main[f] for f in FIELDS + (TS,)}
        c["v"] = main["big"]
        return c, NDOCS
    if "small_v" not in _cache:
        c, n = tail_columns()
        c = dict(c)
        c[TS] = _i64(_sorted_ts(n, (9, 10, 11)))
        c["v"] = _i64(c[RT]["values"] * 3 + 1)
        _cache["small_v"] = (c, n)
    return _cache["small_v"]


# ---- builders --------------------------------------------------------------------------------------------------------------
def dh(subs=(), name="h"):
    h = AB.dateHistogram(name).field(TS).interval("1h")
    for s in subs:
        h.subAggregation(copy.deepcopy(s))
    return h


def flt_root(filters, kids, other=False, name="f"):
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


SINGLE = {"su": "sum", "mi": "min", "ma": "max"}  # single-value leaves and the value of the oracle's stats `st` they restate


class Case:
    """One request: a filters (spec = [(key, query)]) or a range (spec = [(key, from, to)] over `field`) aggregation
    with the children kids() -- metrics (paths 11 / 12) or a date_histogram over them (13).  twin(): what the oracle runs
    where kids() hold single-value leaves (SINGLE).  exact: integer-valued sums the oracle adds exactly are bit-exact.
    strict: every floating sum within the bar of the exact sum (helpers.assert_same_exact(strict=True))."""

    def __init__(self, name, kind, spec, kids, path, field=RT, other=False, query=None, accept=False, exact=True,
                 bpws=BPWS, twin=None, strict=False, metric=None):
        self.name, self.kind, self.spec, self.kids, self.path, self.field = name, kind, spec, kids, path, field
        self.other, self.query, self.accept, self.exact, self.bpws, self.twin = other, query, accept, exact, tuple(bpws), twin
        self.strict, self.metric = strict, metric

    def root(self):
        if self.kind == "filters":
            return flt_root(self.spec, self.kids(), self.other)
        return rng_root(self.spec, self.kids(), self.field)

    @property
    def agg_name(self):
        return "f" if self.kind == "filters" else "r"

    def accept_mask(self, n):
        return (np.random.default_rng(5).random(n) < 0.7) if self.accept else None

    def masks(self, cols, n):
        """-> (bucket keys, [R] x [n] bool) in result order, the accept bits included, the query not"""
        acc = self.accept_mask(n)
        if self.kind == "filters":
            return [k for k, _q in self.spec] + (["_other_"] if self.other else []), MH.filters_masks(cols, self.spec, n, self.other, acc)
        c = cols[self.field]
        if c.get("offsets") is not None:
            bks = RR.buckets(self.spec)
            return [k for _i, k, _lo, _hi in bks], list(RR.doc_masks(c["values"], bks, n, offsets=c["offsets"], accept=acc))
        return MH.range_masks(cols, self.field, self.spec, n, acc)


def reference(case, segs):
    """segs: [(name, columns, n)].  -> {"keys", "counts": doc count per bucket, "want": per bucket the oracle's result for
    the children at top level under the bucket's doc masks}; computed once per (case, segments) and never modified"""
    key = (case.name,) + tuple(s[0] for s in segs)
    if key in _cache:
        return _cache[key]
    per = [case.masks(c, n) for _nm, c, n in segs]
    keys = per[0][0]
    counts, want = [], []
    for b in range(len(keys)):
        ms = [per[s][1][b] for s in range(len(segs))]
        dc = 0
        for (_nm, c, n), m in zip(segs, ms):
            q = m.copy()
            for cl in case.query or ():
                q &= FR.clause_mask(c, cl, n)
            dc += int(q.sum())
        counts.append(dc)
        kids = (case.twin or case.kids)()
        want.append(O.run([(c, n) for _nm, c, n in segs], kids, filters=case.query, accept=[bits_from_mask(m) for m in ms],
                          exact=True) if kids else None)
    _cache[key] = {"keys": keys, "counts": counts, "want": want}
    return _cache[key]


def main_segs():
    return [("main", main_columns(), NDOCS)]


def stats_of(field, name="s"):
    return lambda: [AB.stats(name).field(field)]


def hist_of(make):
    return lambda: [dh(make())]


def carry_cases():
    """the block-carry requests of tests/test_gpu_mask_block_carry.py"""
    st, none = stats_of("bytes"), (lambda: [])
    ext = lambda: [AB.extendedStats("x").field("bytes")]  # noqa: E731
    return [
        Case("filters_hist_stats", "filters", MIXED, hist_of(st), 13, other=True),
        Case("range_hist_stats", "range", RANGES, hist_of(st), 13),
        Case("filters_hist_counts", "filters", MIXED, hist_of(none), 13, other=True),
        Case("range_hist_counts", "range", RANGES, hist_of(none), 13),
        Case("filters_hist_extended", "filters", CLASSES, hist_of(ext), 13, other=True, bpws=(3, 13)),
        Case("range_hist_extended", "range", RANGES, hist_of(ext), 13, bpws=(3, 13)),
        Case("range_64_stats", "range", RANGES64, stats_of("m"), 11, field="zone"),
        Case("filters_63_other_stats", "filters", FILTERS63, stats_of("m"), 12, other=True),
        Case("range_multi_valued_stats", "range", CODES, st, 11, field="codes", bpws=(3, 13)),
        Case("range_sparse_metric", "range", RANGES, stats_of("sz"), 11),
        Case("filters_sparse_metric", "filters", MIXED, stats_of("sz"), 12, other=True),
        Case("filters_hist_sparse_metric", "filters", CLASSES, hist_of(stats_of("sz")), 13, other=True),
        Case("range_hist_sparse_metric", "range", RANGES, hist_of(stats_of("sz")), 13, bpws=(2, 5)),
        Case("filters_hist_query_accept", "filters", CLASSES, hist_of(st), 13, other=True, query=QUERY, accept=True),
        Case("range_query_accept", "range", RANGES, st, 11, query=QUERY, accept=True, bpws=(2, 13)),
    ]


EXACT_BPWS = (1, 5)
EXACT_COLUMNS = [("big", True), ("bytes", True), ("price", False)] + [("sp_" + k, False) for k in SPECIAL]


def exact_cases(field, exact):
    """the four requests a metric column of tests/test_gpu_mask_float_exact.py goes through"""
    ext = lambda: [AB.extendedStats("x").field(field)]  # noqa: E731
    st_avg = lambda: [AB.stats("s").field(field), AB.avg("a").field(field)]  # noqa: E731
    three = lambda: [dh([AB.sum("su").field(field), AB.min("mi").field(field), AB.max("ma").field(field)])]  # noqa: E731
    twin = lambda: [dh([AB.stats("st").field(field)])]  # noqa: E731
    kw = dict(exact=exact, bpws=EXACT_BPWS, strict=True, metric=field)
    return [
        Case("exact_%s_range_extended" % field, "range", RANGES, ext, 11, **kw),
        Case("exact_%s_filters_stats_avg" % field, "filters", MIXED, st_avg, 12, other=True, **kw),
        Case("exact_%s_filters_hist_extended" % field, "filters", MIXED, hist_of(ext), 13, other=True, **kw),
        Case("exact_%s_range_hist_sum_min_max" % field, "range", RANGES, three, 13, twin=twin, **kw),
    ]


def plan_cases():
    """the plan-level requests over the metric field `v` (v_columns)"""
    kw = dict(exact=True, bpws=EXACT_BPWS, strict=True, metric="v")
    return [Case("plan_v_filters_hist_stats", "filters", MIXED, hist_of(stats_of("v")), 13, other=True, **kw),
            Case("plan_v_range_extended", "range", RANGES, lambda: [AB.extendedStats("x").field("v")], 11, **kw)]


# ---- the key window, restated (esgpu_mask_hist.hip) ------------------------------------------------------------------------
def ranges_of(bpw, nb=NB):
    """the zone blocks of each workgroup: blocks_per_wg = bpw, grid = ceil(nb / bpw)"""
    return [list(range(b, min(b + bpw, nb))) for b in range(0, nb, bpw)]


def walk(blocks):
    """One workgroup over `blocks` (indices into BLOCKS) -> per block a dict: w0 before and after, whether the window
    moved and whether that flushed live cells.  The window moves to a block's first row when it is unset, kmn < w0 or
    kmx >= w0 + SLOTS; a block without a key is skipped."""
    w0, out = None, []
    for b in blocks:
        kind, rows = BLOCKS[b]
        step = {"block": b, "kind": kind, "rows": rows, "w0_before": w0, "moved": False, "flushed": False}
        if kind != "nokey":
            kmn, kmx = min(rows), max(rows)
            if w0 is None or kmn < w0 or kmx >= w0 + SLOTS:
                step["moved"], step["flushed"] = True, w0 is not None
                w0 = kmn
            step["to_grid"] = [r for r in rows if not (0 <= r - w0 < SLOTS)]  # rows added straight to the grid
        step["w0_after"] = w0
        out.append(step)
    return out


# ---- a rendered result against the reference ---------------------------------------------------------------------------
SQUARES = {"sum_of_squares"}
DERIVED = {"variance", "std_deviation", "std_deviation_bounds"}  # what extended_stats derives from its two sums
PARTS = {"plain": lambda k: k not in SQUARES | DERIVED,  # count, min, max, avg, sum
         "squares": lambda k: k in SQUARES,
         "derived": lambda k: k in DERIVED}


def part_of(tree, part):
    """a result tree with every extended_stats leaf (rendered values, _internal, _exact) cut down to one of PARTS; keys,
    doc counts and every other leaf stay as they are"""
    if part is None:
        return tree
    if isinstance(tree, list):
        return [part_of(v, part) for v in tree]
    if not isinstance(tree, dict):
        return tree
    if "variance" in tree:
        def cut(d):
            return {k: (cut(v) if k in ("_internal", "_exact") else v) for k, v in d.items()
                    if k in ("_internal", "_exact") or PARTS[part](k)}
        return cut(tree)
    return {k: part_of(v, part) for k, v in tree.items()}


def _same(case, got, want, path, report=None, part=None, exact=None):
    got, want = part_of(got, part), part_of(want, part)
    exact = case.exact if exact is None else exact
    if case.strict:
        assert_same_exact(got, want, path, exact_floats=exact, report=report, strict=True)
    else:
        assert_same(got, want, path, exact)


def _single_leaves(case, got, want, path, report):
    """a histogram whose buckets hold the single-value leaves of SINGLE against the oracle's with the stats leaf `st`:
    keys and doc counts as they stand, every leaf against the stats value it restates (_internal: +-Infinity / 0.0 where
    no doc has a value; the sum with its exact counterpart)"""
    assert len(got["buckets"]) == len(want["buckets"]), path
    for g, w in zip(got["buckets"], want["buckets"]):
        p = "%s[%s]" % (path, w["key"])
        assert {k: v for k, v in g.items() if k not in SINGLE} == {k: v for k, v in w.items() if k != "st"}, p
        assert set(g) >= set(SINGLE), p
        st = w["st"]
        for leaf, stat in SINGLE.items():
            one = {stat: st["_internal"][stat]}
            if stat == "sum" and "_exact" in st:
                one["_exact"] = {"sum": st["_exact"]["_internal"]["sum"]}
            _same(case, {stat: g[leaf]["value"]}, one, "%s.%s" % (p, leaf), report)


def compare(case, ref, shard, red, nsegs, tag="", report=None, part=None, exact=None):
    """shard / red: the request's aggregation as rendered from the shard result and from reduce([result]).  Keys and doc
    counts exact; bucket i's children against the oracle's result under bucket i's mask -- the reduced one, and the
    shard's own where the plan collected one segment.  part: one of PARTS -- that part of every extended_stats leaf
    alone; exact: in place of case.exact."""
    for d in (shard, red):
        assert [b["key"] for b in d["buckets"]] == list(ref["keys"]), tag
        assert [b["doc_count"] for b in d["buckets"]] == ref["counts"], tag
    names = [k.name for k in case.kids()]
    for i, want in enumerate(ref["want"]):
        for d in (shard, red):
            assert set(d["buckets"][i]) - {"key", "from", "to", "doc_count", "from_as_string", "to_as_string"} == set(names), tag
        for nm in names:
            pairs = [(red["buckets"][i][nm], want["reduced"][nm], "%s reduced bucket[%d].%s" % (tag, i, nm))]
            if nsegs == 1:
                pairs.append((shard["buckets"][i][nm], want["shards"][0][nm], "%s shard bucket[%d].%s" % (tag, i, nm)))
            for got, w, path in pairs:
                if case.twin:
                    _single_leaves(case, got, w, path, report)
                else:
                    _same(case, got, w, path, report, part, exact)



# ---- the GPU files' runner (the one function here that runs the code under test) -----------------------------------------
def run_plan(engine, monkeypatch, case, segs, bpw):
    """segs: [(segment, n)], collected with bpw zone blocks per workgroup -> the request's aggregation of the shard
    result and of reduce([result]), the collect statistics"""
    from elasticsearch_amd import reduce
    monkeypatch.setenv("ESGPU_DEBUG_BPW", str(bpw))
    plan = engine.plan([case.root()], filters=case.query, ord_lookup=ord_lookup)
    for s, n in segs:
        plan.collect(s, accept_bits=bits_from_mask(case.accept_mask(n)) if case.accept else None)
    res = plan.build()
    stats = plan.last_collect_stats()
    mergeable = plan.shard_mergeable()
    plan.close()
    assert mergeable
    return res.to_dict()[case.agg_name], reduce([res]).to_dict()[case.agg_name], stats
