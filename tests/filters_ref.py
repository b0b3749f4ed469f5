"""Test-side reference of the filters aggregation (A/bucket/filters/FiltersAggregator.java, InternalFilters.java,
FiltersParser.java; A = core/src/main/java/org/elasticsearch/search/aggregations).  Nothing here calls the code under
test.

clause_mask(cols, q, n)              [n] bool: the docs a TermQuery / RangeQuery accepts, restated over numpy columns
doc_masks(cols, filters, n, ...)     ([F][n] bool per filter, [n] bool of the other bucket)
metric(mask, vals, present)          range_ref.metric: count / exact sum / min / max over the docs of a mask
filter_twin(filters, subs)           one top-level filter aggregation "f<i>" per filter, for the oracle
record(aggs)                         the library-private shard record (version 8) of hand-built filters blocks
decode_stream(bytes)                 tests/es_stream.decode extended by the filters, range and single-value metric types
"""
import copy
import math
import struct

import numpy as np

import range_ref as RR
import result_stream as RS
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import _native as N
from elasticsearch_amd.aggs import RangeQuery, TermQuery

VERSION = 8  # the layout of version 7; the version of a result holding a filters block
MISSING_ORD = 0xFFFFFFFF
metric = RR.metric


def mask_from_bits(bits, n):
    """the inverse of helpers.bits_from_mask"""
    w = np.ascontiguousarray(bits, dtype=np.uint64)
    return ((w[np.arange(n) >> 6] >> (np.arange(n, dtype=np.uint64) & np.uint64(63))) & np.uint64(1)).astype(bool)


def _terms(c):
    if c.get("terms") is not None:
        return [t.encode() if isinstance(t, str) else bytes(t) for t in c["terms"]]
    blob, offs = c["terms_blob"]
    blob = bytes(np.asarray(blob, dtype=np.uint8))
    return [blob[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def clause_mask(cols, q, n):
    """the docs of the first n a clause accepts.  A doc without a value -- a clear present bit, the missing ordinal --
    matches no clause; on a double column the comparisons are IEEE (NaN matches nothing, both zeros are equal); on a
    keyword column terms compare as unsigned bytes and a term absent from the dictionary matches nothing."""
    c = cols[q.field]
    vals = np.asarray(c["values"])[:n]
    has = np.ones(n, dtype=bool) if c.get("present") is None else mask_from_bits(c["present"], n)
    if c["type"] == N.COL_ORD_U32:
        terms = _terms(c)
        has = has & (vals != MISSING_ORD)
        ok = np.zeros(len(terms), dtype=bool)
        as_bytes = lambda t: t.encode() if isinstance(t, str) else bytes(t)  # noqa: E731
        for o, t in enumerate(terms):
            if isinstance(q, TermQuery):
                ok[o] = t == as_bytes(q.value)
            else:
                lo_ok = q.lo is None or (t >= as_bytes(q.lo) if q.include_lower else t > as_bytes(q.lo))
                hi_ok = q.hi is None or (t <= as_bytes(q.hi) if q.include_upper else t < as_bytes(q.hi))
                ok[o] = lo_ok and hi_ok
        m = np.zeros(n, dtype=bool)
        m[has] = ok[vals[has].astype(np.int64)]
        return m
    if c["type"] == N.COL_F64:
        v = vals.astype(np.float64)
        with np.errstate(invalid="ignore"):
            if isinstance(q, TermQuery):
                m = v == float(q.value)
            else:
                m = np.ones(n, dtype=bool)
                if q.lo is not None:
                    m &= (v >= float(q.lo)) if q.include_lower else (v > float(q.lo))
                if q.hi is not None:
                    m &= (v <= float(q.hi)) if q.include_upper else (v < float(q.hi))
        return m & has
    v = [int(x) for x in vals.astype(np.int64)]  # python ints: no overflow at the ends of the long range
    if isinstance(q, TermQuery):
        m = np.array([x == int(q.value) for x in v], dtype=bool)
    else:
        # (an infinite bound stays the float it is: python compares ints with it exactly)
        lo, hi = (b if b is None or (isinstance(b, float) and math.isinf(b)) else int(b) for b in (q.lo, q.hi))
        m = np.array([(lo is None or (x >= lo if q.include_lower else x > lo)) and
                      (hi is None or (x <= hi if q.include_upper else x < hi)) for x in v], dtype=bool)
    return m.reshape(n) & has


def _clauses(q):
    return list(q) if isinstance(q, (list, tuple)) else [q]


def doc_masks(cols, filters, n, accept=None):
    """filters: one query (a clause or a list of clauses; [] = match_all) per filter, in bucket order.
    -> ([F][n] bool, [n] bool): the docs of each filter and of the other bucket, both within `accept` (bool per doc)"""
    acc = np.ones(n, dtype=bool) if accept is None else np.asarray(accept, dtype=bool)[:n]
    out = []
    for q in filters:
        m = acc.copy()
        for cl in _clauses(q):
            m &= clause_mask(cols, cl, n)
        out.append(m)
    fm = np.array(out).reshape(len(filters), n)
    return fm, acc & ~fm.any(axis=0)


def filter_twin(filters, subs):
    """One top-level filter aggregation "f<i>" per filter with deep copies of `subs`; match_all ([]) becomes a range
    clause every doc of `response_time_ms` passes (a filter aggregation needs a clause)."""
    out = []
    for i, q in enumerate(filters):
        cl = _clauses(q) or [QB.rangeQuery("response_time_ms").gte(-(1 << 62))]
        f = AB.filter("f%d" % i, cl)
        for s in subs:
            f.subAggregation(copy.deepcopy(s))
        out.append(f)
    return out


# ---- the library-private shard record of hand-built blocks ---------------------------------------------------------
stats = RR.stats


def filters_agg(name, bks, keyed=True, **params):
    """a filters instance: bks = [{"key", "doc_count", "subs": [stats(...), ...]}] in bucket order"""
    a = {"type": N.AGG_FILTERS, "name": name, "keyed": int(keyed), "buckets": bks}
    a.update(params)
    return a


def _block(b, insts):
    a = insts[0]
    t = a["type"]
    b += struct.pack("<ii", t, 0)
    RS._str(b, a["name"])
    b += struct.pack("<iiqii", 10, 10, 1, 0, a.get("keyed", 0))
    b += struct.pack("<Biqq", 0, 0, 1, 0)
    RS._vec(b, "q", [])
    RS._vec(b, "q", [])
    b += struct.pack("<BBqq", 0, 0, 0, 0)
    b += struct.pack("<di", a.get("sigma", 2.0), 14)
    RS._str(b, "")
    RS._fmt(b, a)
    b += struct.pack("<Q", len(insts))
    flt = t == N.AGG_FILTERS
    bks = [bk for x in insts for bk in x.get("buckets", [])]
    RS._vec(b, "q", [0 for _ in insts] if flt else [])
    RS._vec(b, "q", [0 for _ in insts] if flt else [])
    offs = [0]
    for x in insts:
        offs.append(offs[-1] + len(x.get("buckets", [])))
    RS._vec(b, "Q", offs if flt else [])
    RS._vec(b, "q", [k - offs[i] for i, x in enumerate(insts) for k in range(offs[i], offs[i + 1])])
    keys = [bk["key"].encode() for bk in bks]
    toff = [0]
    for s in keys:
        toff.append(toff[-1] + len(s))
    RS._vec(b, "Q", toff if flt else [])
    RS._str(b, b"".join(keys))
    RS._vec(b, "q", [bk["doc_count"] for bk in bks])
    RS._vec(b, "q", [0 for _ in bks])
    b += struct.pack("<i", 0)  # terms kind (version 6)
    RS._vec(b, "q", [])        # long keys
    RS._vec(b, "d", [])        # range bounds (version 7): none on a filters block
    RS._vec(b, "d", [])
    nsubs = len(bks[0]["subs"] if bks else [])
    b += struct.pack("<I", nsubs)
    for j in range(nsubs):
        _block(b, [bk["subs"][j] for bk in bks])
    b += struct.pack("<I", 0)
    met = not flt
    RS._vec(b, "q", [x["count"] for x in insts] if met else [])
    RS._vec(b, "d", [x["sum"] for x in insts] if met else [])
    RS._vec(b, "d", [x["min"] for x in insts] if met else [])
    RS._vec(b, "d", [x["max"] for x in insts] if met else [])
    RS._vec(b, "d", [x["sumsq"] for x in insts] if met else [])
    RS._vec(b, "B", [])
    RS._vec(b, "i", [])
    b += struct.pack("<QQ", 0, 0)


def record(aggs, version=VERSION):
    """esgpu_result_serialize's format of top-level filters_agg(...) / stats(...) instances"""
    b = bytearray(struct.pack("<II", RS.MAGIC, version))
    b += struct.pack("<I", len(aggs))
    for a in aggs:
        _block(b, [a])
    return bytes(b)


# ---- InternalAggregations.readFrom with the filters type -----------------------------------------------------------
def decode_stream(data):
    """tests/es_stream.decode extended by InternalFilters.doReadFrom (InternalFilters.java:231-243: keyed, a vInt size,
    per bucket Bucket.readFrom :145-151 -- readOptionalString, a vLong doc count, the aggregations; no formatter), by
    InternalRange.doReadFrom and by the single-value metrics' doReadFrom"""
    import es_stream as ES

    def aggs(s):
        out = []
        for _ in range(s.vint()):
            typ = s.bytes_ref().decode()
            if typ not in ("filters", "range", "sum", "min", "max", "value_count"):
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
                out.append(a)
                continue
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
