"""Test-side reference of the range aggregation (A/bucket/range/RangeAggregator.java, InternalRange.java;
A = core/src/main/java/org/elasticsearch/search/aggregations).  Nothing here calls the code under test.

buckets(ranges)                      the ranges sorted as RangeAggregator.sortRanges sorts them, with their keys
doc_masks(vals, ranges, ...)         [R][n_docs] bool: doc d is in bucket r (a value v with (double) v >= from and < to)
metric(mask, vals, present)          count / exact sum / min / max of a metric column over the docs of a mask
filter_twin(field, ranges, subs)     one top-level filter aggregation per range (integral bounds), for the oracle
record(aggs)                         the library-private shard record (version 7) of hand-built range blocks
decode_stream(bytes)                 tests/es_stream.decode extended by the range and single-value metric types
"""
import copy
import math
import struct

import numpy as np

import result_stream as RS
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import _native as N
from single_metric_stream import java_double

INF = math.inf
VERSION = 7  # version 6 (terms kind + long keys per block) plus the range bounds per block


def _double_compare_key(v):
    """Double.compare order on non-NaN doubles: numeric, -0.0 before 0.0"""
    return (v, 0 if (v != 0.0 or math.copysign(1.0, v) < 0) else 1)


def buckets(ranges, fmt=java_double):
    """ranges: (key or None, from, to) in request order -> [(request index, key, from, to)] in bucket order: a stable
    sort by (from, to) (RangeAggregator.java:225-244); a missing key is generated (InternalRange.Bucket.generateKey)."""
    out = []
    for i, (key, lo, hi) in enumerate(ranges):
        lo, hi = float(lo), float(hi)
        if key is None:
            key = ("*" if math.isinf(lo) else fmt(lo)) + "-" + ("*" if math.isinf(hi) else fmt(hi))
        out.append((i, key, lo, hi))
    return sorted(out, key=lambda b: (_double_compare_key(b[2]), _double_compare_key(b[3])))


def value_masks(vals, bks):
    """[R][n_values] bool over the values as doubles (Range.matches: value >= from && value < to)"""
    d = np.asarray(vals).astype(np.float64)
    return np.array([(d >= lo) & (d < hi) for _i, _k, lo, hi in bks]).reshape(len(bks), len(d))


def doc_masks(vals, bks, n_docs, present=None, offsets=None, accept=None):
    """[R][n_docs] bool.  present: bool per doc (single-valued sparse field); offsets: CSR offsets of a multi-valued
    field (a doc is in a bucket once, whatever number of its values match); accept: bool per doc (filters)."""
    vm = value_masks(vals, bks)
    if offsets is not None:
        offsets = np.asarray(offsets, dtype=np.int64)
        cs = np.concatenate([np.zeros((len(bks), 1), np.int64), np.cumsum(vm, axis=1, dtype=np.int64)], axis=1)
        dm = (cs[:, offsets[1:]] - cs[:, offsets[:-1]]) > 0
    else:
        dm = vm[:, :n_docs].copy()
        if present is not None:
            dm &= np.asarray(present, dtype=bool)[None, :]
    if accept is not None:
        dm &= np.asarray(accept, dtype=bool)[None, :]
    return dm


def metric(mask, vals, present=None):
    """-> (count, sum, min, max) of `vals` over the docs of `mask` that have a value: the sum exact (int64 arithmetic
    for a long column, math.fsum for doubles), min / max +-inf when there is none"""
    m = np.asarray(mask, dtype=bool)
    if present is not None:
        m = m & np.asarray(present, dtype=bool)
    v = np.asarray(vals)[: len(m)][m]
    if len(v) == 0:
        return 0, 0.0, INF, -INF
    s = float(int(v.astype(np.int64).sum())) if v.dtype.kind in "iu" else math.fsum(v.tolist())
    return int(len(v)), s, float(v.min()), float(v.max())


def filter_twin(field, ranges, subs):
    """One top-level filter aggregation "f<i>" per range, i in bucket order: rangeQuery(field).gte(from).lt(to) with
    deep copies of `subs`.  Bounds must be integral or infinite (the oracle's range clause on a long field takes longs)."""
    out = []
    for b, (_i, _key, lo, hi) in enumerate(buckets(ranges)):
        q = QB.rangeQuery(field)
        if not math.isinf(lo):
            assert lo == int(lo)
            q = q.gte(int(lo))
        if not math.isinf(hi):
            assert hi == int(hi)
            q = q.lt(int(hi))
        if math.isinf(lo) and math.isinf(hi):
            q = q.gte(-(1 << 62))  # (a range clause needs a bound)
        f = AB.filter("f%d" % b, q)
        for s in subs:
            f.subAggregation(copy.deepcopy(s))
        out.append(f)
    return out


# ---- the library-private shard record of hand-built blocks ---------------------------------------------------------
def stats(kind, name, count=0, sum=0.0, min=INF, max=-INF, sumsq=0.0, **params):  # noqa: A002
    """a metric instance (stats / extended_stats / avg / sum / min / max / value_count) for record()"""
    a = {"type": kind, "name": name, "count": count, "sum": sum, "min": min, "max": max, "sumsq": sumsq}
    a.update(params)
    return a


def range_agg(name, bks, keyed=False, **params):
    """a range instance: bks = [{"key", "from", "to", "doc_count", "subs": [stats(...), ...]}] in bucket order"""
    a = {"type": N.AGG_RANGE, "name": name, "keyed": int(keyed), "buckets": bks}
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
    rng = t == N.AGG_RANGE
    bks = [bk for x in insts for bk in x.get("buckets", [])]
    RS._vec(b, "q", [0 for _ in insts] if rng else [])
    RS._vec(b, "q", [0 for _ in insts] if rng else [])
    offs = [0]
    for x in insts:
        offs.append(offs[-1] + len(x.get("buckets", [])))
    RS._vec(b, "Q", offs if rng else [])
    RS._vec(b, "q", [k - offs[i] for i, x in enumerate(insts) for k in range(offs[i], offs[i + 1])])
    keys = [bk["key"].encode() for bk in bks]
    toff = [0]
    for s in keys:
        toff.append(toff[-1] + len(s))
    RS._vec(b, "Q", toff if rng else [])
    RS._str(b, b"".join(keys))
    RS._vec(b, "q", [bk["doc_count"] for bk in bks])
    RS._vec(b, "q", [0 for _ in bks])
    b += struct.pack("<i", 0)  # terms kind (version 6)
    RS._vec(b, "q", [])        # long keys
    RS._vec(b, "d", [float(bk["from"]) for bk in bks])  # range bounds (version 7)
    RS._vec(b, "d", [float(bk["to"]) for bk in bks])
    nsubs = len(a.get("sub_specs", bks[0]["subs"] if bks else []))
    b += struct.pack("<I", nsubs)
    for j in range(nsubs):
        _block(b, [bk["subs"][j] for bk in bks])
    b += struct.pack("<I", 0)
    met = not rng
    RS._vec(b, "q", [x["count"] for x in insts] if met else [])
    RS._vec(b, "d", [x["sum"] for x in insts] if met else [])
    RS._vec(b, "d", [x["min"] for x in insts] if met else [])
    RS._vec(b, "d", [x["max"] for x in insts] if met else [])
    RS._vec(b, "d", [x["sumsq"] for x in insts] if met else [])
    RS._vec(b, "B", [])
    RS._vec(b, "i", [])
    b += struct.pack("<QQ", 0, 0)


def record(aggs):
    """esgpu_result_serialize's format, version 7, of top-level range_agg(...) / stats(...) instances"""
    b = bytearray(struct.pack("<II", RS.MAGIC, VERSION))
    b += struct.pack("<I", len(aggs))
    for a in aggs:
        _block(b, [a])
    return bytes(b)


# ---- InternalAggregations.readFrom with the range type -------------------------------------------------------------
def decode_stream(data):
    """tests/es_stream.decode extended by InternalRange.doReadFrom (InternalRange.java:308-321) and the single-value
    metrics' doReadFrom (formatter, then a double; value_count: a vLong)"""
    import es_stream as ES

    def aggs(s):
        out = []
        for _ in range(s.vint()):
            typ = s.bytes_ref().decode()
            if typ not in ("range", "sum", "min", "max", "value_count"):
                out.append(ES._agg(s, typ))
                continue
            a = {"stream_type": typ, "name": s.string()}
            assert s.sbyte() == -1 and s.vint() == 0  # null metadata, no pipeline aggregators
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
