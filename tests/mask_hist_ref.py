"""Test-side helpers for a date_histogram under a range or a filters aggregation (collect path 13).  Nothing here calls
the code under test.

hist_instance(agg, buckets)          a shard-level histogram instance of the builder `agg` for record(): buckets =
                                     [(key, doc_count, (count, sum, min, max) or None per metric child)]
record(aggs)                         the library-private shard record (version 8) of hand-built filters / range blocks
                                     whose buckets carry histogram (and metric) instances: filters_ref.record /
                                     range_ref.record with the sub-blocks written by result_stream
bucket_masks(...)                    the doc masks of a range's or a filters aggregation's buckets, in result order
decode_stream(bytes)                 filters_ref.decode_stream extended by a histogram reader that recurses into it, so
                                     the single-value metrics decode below a nested histogram too
"""
import struct

import numpy as np

import filters_ref as FR
import range_ref as RR
import result_stream as RS
from elasticsearch_amd import _native as N

VERSION = FR.VERSION


def hist_instance(agg, buckets):
    """agg: a top-level AB.dateHistogram(...) builder with stats-like children; buckets: [(key, doc_count, [st, ...])], one
    st = (count, sum, min, max) or None (no value) per child -> the instance dict result_stream._block writes.  The
    parameters (rounding, min_doc_count, bounds, order, format, the empty sub-aggregations) come from the builder's own
    lowering (result_stream.from_shard_json)."""
    names = [s.name for s in agg.subs]
    js = {"buckets": []}
    for key, dc, sts in buckets:
        b = {"key": key, "doc_count": dc}
        for nm, st in zip(names, sts):
            cnt, sm, mn, mx = st if st is not None else (0, 0.0, float("inf"), float("-inf"))
            b[nm] = {"_internal": {"count": cnt, "sum": sm, "min": mn, "max": mx}}
        js["buckets"].append(b)
    return RS.from_shard_json([agg], {agg.name: js})[0]


METRIC_TYPES = (N.AGG_STATS, N.AGG_EXTENDED_STATS, N.AGG_AVG, N.AGG_SUM, N.AGG_MIN, N.AGG_MAX, N.AGG_VALUE_COUNT)
KEYED_TYPES = (N.AGG_FILTERS, N.AGG_RANGE)          # buckets by position, their keys in the term pool


def _block(b, insts, spec=None):
    """One block of the version-8 layout from same-spec instance dicts (`spec` alone: a block with no instance):
    result_stream._block's fields plus the terms kind and long keys of version 6 and the range bounds of version 7 -- a
    filters or a range block as filters_ref._block / range_ref._block write it, with histogram and metric sub-blocks, one
    instance per bucket."""
    a = insts[0] if insts else spec
    t = a["type"]
    bucket = t in RS.BUCKET_TYPES or t in KEYED_TYPES
    b += struct.pack("<ii", t, a.get("order", 0))
    RS._str(b, a["name"])
    b += struct.pack("<iiqii", a.get("required_size", 10), a.get("shard_size", 10), a.get("min_doc_count", 1),
                     a.get("show_err", 0), a.get("keyed", 0))
    b += struct.pack("<Biqq", a.get("has_empty_info", 0), a.get("date_unit", 0), a.get("interval", 1), a.get("offset", 0))
    RS._vec(b, "q", a.get("tz_starts", []))
    RS._vec(b, "q", a.get("tz_offs", []))
    b += struct.pack("<BBqq", a.get("has_bmin", 0), a.get("has_bmax", 0), a.get("bmin", 0), a.get("bmax", 0))
    b += struct.pack("<di", a.get("sigma", 2.0), a.get("precision", 14))
    RS._str(b, a.get("order_path", ""))
    RS._fmt(b, a)
    b += struct.pack("<Q", len(insts))
    bks = [bk for x in insts for bk in x.get("buckets", [])] if bucket else []
    RS._vec(b, "q", [0 for _ in insts] if bucket else [])
    RS._vec(b, "q", [0 for _ in insts] if bucket else [])
    offs = [0]
    for x in insts:
        offs.append(offs[-1] + len(x.get("buckets", [])))
    RS._vec(b, "Q", offs if bucket else [])
    if t in KEYED_TYPES:
        RS._vec(b, "q", [k - offs[i] for i, x in enumerate(insts) for k in range(offs[i], offs[i + 1])])
        keys = [bk["key"].encode() for bk in bks]
    else:
        RS._vec(b, "q", [bk["key"] for bk in bks])
        keys = [b"" for _ in bks]
    toff = [0]
    for s in keys:
        toff.append(toff[-1] + len(s))
    RS._vec(b, "Q", toff if bucket else [])
    RS._str(b, b"".join(keys))
    RS._vec(b, "q", [bk["doc_count"] for bk in bks])
    RS._vec(b, "q", [0 for _ in bks])
    b += struct.pack("<i", 0)  # terms kind (version 6)
    RS._vec(b, "q", [])        # long keys
    rng = t == N.AGG_RANGE     # range bounds (version 7)
    RS._vec(b, "d", [float(bk["from"]) for bk in bks] if rng else [])
    RS._vec(b, "d", [float(bk["to"]) for bk in bks] if rng else [])
    subs = a.get("sub_specs", bks[0]["subs"] if bks else [])
    b += struct.pack("<I", len(subs))
    for j in range(len(subs)):
        rows = [bk["subs"][j] for bk in bks]
        if a.get("sub_rows") is not None:      # a corrupt record: sub-block j with this many instances instead
            rows = rows[: a["sub_rows"]]
        _block(b, rows, subs[j])
    empty = a.get("empty_subs", [])
    b += struct.pack("<I", len(empty))
    for e in empty:
        _block(b, [e])
    met = t in METRIC_TYPES
    RS._vec(b, "q", [x.get("count", 0) for x in insts] if met else [])
    RS._vec(b, "d", [x.get("sum", 0.0) for x in insts] if met else [])
    RS._vec(b, "d", [x.get("min", float("inf")) for x in insts] if met else [])
    RS._vec(b, "d", [x.get("max", float("-inf")) for x in insts] if met else [])
    RS._vec(b, "d", [x.get("sumsq", 0.0) for x in insts] if met else [])
    RS._vec(b, "B", [])
    RS._vec(b, "i", [])
    b += struct.pack("<QQ", 0, 0)


def record(aggs, version=VERSION):
    b = bytearray(struct.pack("<II", RS.MAGIC, version))
    b += struct.pack("<I", len(aggs))
    for a in aggs:
        _block(b, [a])
    return bytes(b)


# ---- doc masks of the buckets ----------------------------------------------------------------------------------------
def filters_masks(cols, filters, n, other=False, accept=None):
    """filters: [(key, query)] -> the buckets' [n] bool masks in result order (the filters, then the other bucket)"""
    fm, om = FR.doc_masks(cols, [q for _k, q in filters], n, accept)
    return list(fm) + ([om] if other else [])


def range_masks(cols, field, ranges, n, accept=None):
    """ranges: [(key, from, to)] -> (bucket keys, [n] bool masks) in bucket order"""
    c = cols[field]
    bks = RR.buckets(ranges)
    pres = None if c.get("present") is None else FR.mask_from_bits(c["present"], n)
    dm = RR.doc_masks(np.asarray(c["values"])[:n], bks, n, present=pres, accept=accept)
    return [k for _i, k, _lo, _hi in bks], list(dm)


# ---- InternalAggregations.readFrom: filters / range over histograms over any metric ---------------------------------
def decode_stream(data):
    """filters_ref.decode_stream (InternalFilters / InternalRange / the single-value metrics) with
    InternalHistogram.doReadFrom (es_stream._agg's reader, InternalHistogram.java:479-495) recursing into this decoder"""
    import es_stream as ES

    def aggs(s):
        out = []
        for _ in range(s.vint()):
            typ = s.bytes_ref().decode()
            if typ not in ("filters", "range", "sum", "min", "max", "value_count", "histo", "dhisto"):
                out.append(ES._agg(s, typ))
                continue
            a = {"stream_type": typ, "name": s.string()}
            assert s.sbyte() == -1 and s.vint() == 0  # null metadata, no pipeline aggregators
            if typ == "filters":
                a["keyed"] = s.boolean()
                a["buckets"] = []
                for _b in range(s.vint()):
                    key = s.string() if s.boolean() else None
                    a["buckets"].append({"key": key, "doc_count": s.vlong(), "aggs": aggs(s)})
            elif typ in ("histo", "dhisto"):
                a["factory"] = s.string()
                a["order"] = s.byte()
                a["min_doc_count"] = s.vlong()
                if a["min_doc_count"] == 0:
                    a["rounding"] = ES._rounding(s)
                    a["empty_aggs"] = aggs(s)
                    if s.boolean():
                        lo = s.i64() if s.boolean() else None
                        hi = s.i64() if s.boolean() else None
                        a["bounds"] = (lo, hi)
                a["formatter"] = ES._formatter(s)
                a["keyed"] = s.boolean()
                a["buckets"] = [{"key": s.i64(), "doc_count": s.vlong(), "aggs": aggs(s)} for _ in range(s.vint())]
            else:
                a["formatter"] = ES._formatter(s)
                if typ == "range":
                    a["keyed"] = s.boolean()
                    a["buckets"] = []
                    for _b in range(s.vint()):
                        key = s.string() if s.boolean() else None
                        a["buckets"].append({"key": key, "from": s.f64(), "to": s.f64(), "doc_count": s.vlong(), "aggs": aggs(s)})
                elif typ == "value_count":
                    a["value"] = s.vlong()
                else:
                    a["value"] = s.f64()
            out.append(a)
        return out

    s = ES.StreamInput(data)
    out = aggs(s)
    assert s.i == len(s.b), "%d trailing bytes" % (len(s.b) - s.i)
    return out
