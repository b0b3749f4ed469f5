"""Test-side helpers for the single-value metrics sum / min / max / value_count (A/metrics/sum/InternalSum.java,
A/metrics/min/InternalMin.java, A/metrics/max/InternalMax.java, A/metrics/valuecount/InternalValueCount.java;
A = core/src/main/java/org/elasticsearch/search/aggregations).

The oracle has no aggregator for them.  Their reference results come from the **stats twin** of a request: every sum /
min / max / value_count leaf replaced by a stats leaf of the same name and field (StatsAggegator collects the same
values in the same order), an order path `s` by `s.sum` / `s.min` / `s.max` / `s.count`, the twin run through the
oracle and each stats object mapped back to {"value": ...}.

twin(aggs) / untwin(tree, aggs)   the two directions of that mapping
write_stream(decoded, aggs)       InternalAggregations.writeTo of the request, restated: fed from the twin's decoded
                                  transport bytes (tests/es_stream.py), the four doWriteTo methods written here
xcontent(tree, aggs)              the REST body of a result tree (doXContentBody of the four, terms, date_histogram)
record(aggs)                      the library-private shard record (version 5) of hand-built blocks of the four
"""
import copy
import math
import struct

import result_stream as RS
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import _native as N
from elasticsearch_amd.aggs import AggOrder

SINGLE = {N.AGG_SUM: "sum", N.AGG_MIN: "min", N.AGG_MAX: "max", N.AGG_VALUE_COUNT: "count"}
STREAM_TYPE = {N.AGG_SUM: "sum", N.AGG_MIN: "min", N.AGG_MAX: "max", N.AGG_VALUE_COUNT: "value_count"}


# ---- the stats twin ------------------------------------------------------------------------------------------------
def twin(aggs):
    """The request with every single-value leaf as a stats leaf, and order paths naming the stats metric."""
    def visit(b):
        if b.type in SINGLE:
            t = AB.stats(b.name).field(b._field)
            t._format = b._format
            return t
        c = copy.copy(b)
        c.subs = [visit(s) for s in b.subs]
        o = getattr(b, "_order", None)
        if isinstance(o, AggOrder):
            name = o.path[:-len(".value")] if o.path.endswith(".value") else o.path
            for s in b.subs:
                if s.name == name and s.type in SINGLE:
                    c._order = AggOrder(name + "." + SINGLE[s.type], o.asc)
        return c
    return [visit(a) for a in aggs]


def _value(js, kind):
    st = js["_internal"]
    v = st[kind]
    out = {"value": int(v) if kind == "count" else float(v)}
    if "_exact" in js and kind == "sum":  # the exact sum the reference's doc-order additions approximate
        out["_exact"] = {"value": float(js["_exact"]["_internal"]["sum"])}
    return out


def untwin(tree, aggs):
    """An oracle result tree of twin(aggs) with every twinned stats object mapped back to {"value": v}: the sum (0.0
    when empty), the min / max (+-Infinity when empty) or the count."""
    def conv(js, b):
        if b.type in SINGLE:
            return _value(js, SINGLE[b.type])
        if b.type in RS.BUCKET_TYPES:
            js = dict(js)
            js["buckets"] = [dict(bk, **{s.name: conv(bk[s.name], s) for s in b.subs}) for bk in js["buckets"]]
            return js
        if b.type == N.AGG_FILTER:
            return dict(js, **{s.name: conv(js[s.name], s) for s in b.subs})
        return js
    return dict(tree, **{a.name: conv(tree[a.name], a) for a in aggs})


# ---- InternalAggregations.writeTo, restated ------------------------------------------------------------------------
class Out:
    """StreamOutput (C/common/io/stream/StreamOutput.java): big-endian fixed widths, 7-bit variable ints."""

    def __init__(self):
        self.b = bytearray()

    def byte(self, v):
        self.b.append(v & 0xFF)

    def boolean(self, v):
        self.byte(1 if v else 0)

    def vint(self, v):
        v &= 0xFFFFFFFF
        while v & ~0x7F:
            self.byte((v & 0x7F) | 0x80)
            v >>= 7
        self.byte(v)

    def vlong(self, v):
        assert v >= 0
        while v & ~0x7F:
            self.byte((v & 0x7F) | 0x80)
            v >>= 7
        self.byte(v)

    def i64(self, v):
        self.b += struct.pack(">q", v)

    def f64(self, v):
        self.b += struct.pack(">d", v)

    def string(self, s):  # writeString: the char count, then each UTF-16 unit in 1-3 bytes
        units = struct.unpack("<%dH" % (len(s.encode("utf-16-le")) // 2), s.encode("utf-16-le"))
        self.vint(len(units))
        for c in units:
            if c <= 0x7F:
                self.byte(c)
            elif c > 0x7FF:
                self.byte(0xE0 | (c >> 12 & 0x0F)); self.byte(0x80 | (c >> 6 & 0x3F)); self.byte(0x80 | (c & 0x3F))
            else:
                self.byte(0xC0 | (c >> 6 & 0x1F)); self.byte(0x80 | (c & 0x3F))

    def bytes_ref(self, data):
        self.vint(len(data))
        self.b += bytes(data)


def _formatter(o, f):  # ValueFormatterStreams.writeOptional (A/support/format/ValueFormatterStreams.java:54-64)
    o.boolean(f is not None)
    if f is None:
        return
    if f[0] == "raw":
        o.byte(1)
    elif f[0] == "date_time":
        o.byte(2); o.string(f[1]); o.string(f[2])
    else:
        o.byte(4); o.string(f[1])


def _rounding(o, r):  # Rounding.Streams.write
    if r[0] == "interval":
        o.byte(0); o.vlong(r[1])
    elif r[0] == "time_unit":
        o.byte(1); o.byte(r[1]); o.string(r[2])
    elif r[0] == "time_interval":
        o.byte(2); o.vlong(r[1]); o.string(r[2])
    else:
        o.byte(8); _rounding(o, r[1]); o.i64(r[2])


def _order(o, order, rename):  # InternalOrder.Streams.writeOrder
    if isinstance(order, str):
        o.byte({"_count desc": 1, "_count asc": 2, "_term desc": 3, "_term asc": 4}[order])
    elif order[0] == "agg":
        o.byte(0); o.boolean(order[2]); o.string(rename.get(order[1], order[1]))
    else:
        o.byte(0xFF); o.vint(len(order[1]))
        for x in order[1]:
            _order(o, x, rename)


def _size(o, s):
    o.vint(s)  # (the decoder returns what writeSize wrote)


def write_single(o, kind, value, formatter=("raw",)):
    """doWriteTo of InternalSum (:97-100), InternalMin (:97-100), InternalMax (:96-99): the optional formatter, then
    writeDouble(value); InternalValueCount (:97-100): the optional formatter, then writeVLong(value)."""
    _formatter(o, formatter)
    if kind == N.AGG_VALUE_COUNT:
        o.vlong(int(value))
    else:
        o.f64(float(value))


def _head(o, name):  # InternalAggregation.writeTo (A/InternalAggregation.java:212-221): name, null metadata, no pipelines
    o.string(name)
    o.byte(0xFF)
    o.vint(0)


def _list(o, decoded, builders):
    o.vint(len(decoded))
    for a, b in zip(decoded, builders):
        assert a["name"] == b.name
        if b.type in SINGLE:  # the twin's InternalStats (count, min, max, sum) supplies the value
            assert a["stream_type"] == "stats"
            o.bytes_ref(STREAM_TYPE[b.type].encode())
            _head(o, b.name)
            write_single(o, b.type, a[SINGLE[b.type]], a["formatter"])
            continue
        o.bytes_ref(a["stream_type"].encode())
        _head(o, b.name)
        t = a["stream_type"]
        if t == "sterms":  # StringTerms.doWriteTo (:205-217)
            rename = {s.name + "." + SINGLE[s.type]: s.name for s in b.subs if s.type in SINGLE}
            o.i64(a["doc_count_error"])
            _order(o, a["order"], rename)
            _size(o, a["required_size"]); _size(o, a["shard_size"])
            o.boolean(a["show_term_doc_count_error"])
            o.vlong(a["min_doc_count"]); o.vlong(a["other_doc_count"])
            o.vint(len(a["buckets"]))
            for bk in a["buckets"]:
                o.bytes_ref(bk["key"]); o.vlong(bk["doc_count"])
                if a["show_term_doc_count_error"]:
                    o.i64(bk["doc_count_error"])
                _list(o, bk["aggs"], b.subs)
        elif t in ("histo", "dhisto"):  # InternalHistogram.doWriteTo (:510-523)
            o.string(a["factory"]); o.byte(a["order"]); o.vlong(a["min_doc_count"])
            if a["min_doc_count"] == 0:
                _rounding(o, a["rounding"])
                _list(o, a["empty_aggs"], b.subs)
                o.boolean("bounds" in a)
                if "bounds" in a:
                    for v in a["bounds"]:
                        o.boolean(v is not None)
                        if v is not None:
                            o.i64(v)
            _formatter(o, a["formatter"])
            o.boolean(a["keyed"])
            o.vint(len(a["buckets"]))
            for bk in a["buckets"]:
                o.i64(bk["key"]); o.vlong(bk["doc_count"])
                _list(o, bk["aggs"], b.subs)
        else:
            raise ValueError("no writer for %r" % t)


def write_stream(decoded, aggs):
    """The transport bytes of `aggs` from the decoded transport bytes of its stats twin."""
    o = Out()
    _list(o, decoded, aggs)
    return bytes(o.b)


# ---- XContent ------------------------------------------------------------------------------------------------------
def java_double(v):
    """Double.toString: the shortest digits that round-trip (as Python's repr), positional for 1e-3 <= |v| < 1e7, else
    d.dddE<n>."""
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "Infinity" if v > 0 else "-Infinity"
    if v == 0:
        return "-0.0" if math.copysign(1.0, v) < 0 else "0.0"
    from decimal import Decimal
    sign, digits, exp = Decimal(repr(float(v))).as_tuple()
    digits = list(digits)
    while len(digits) > 1 and digits[-1] == 0:
        digits.pop()
        exp += 1
    e10 = len(digits) - 1 + exp
    ds = "".join(map(str, digits))
    neg = "-" if sign else ""
    if 1e-3 <= abs(v) < 1e7:
        if e10 >= 0:
            ip, fp = ds[:e10 + 1].ljust(e10 + 1, "0"), ds[e10 + 1:]
        else:
            ip, fp = "0", "0" * (-e10 - 1) + ds
        return neg + ip + "." + (fp or "0")
    return "%s%s.%sE%d" % (neg, ds[0], ds[1:] or "0", e10)


def xcontent_single(kind, value, value_as_string=None):
    """doXContentBody of InternalSum (:103-109) / InternalValueCount (:103-109): "value", then "value_as_string" unless
    the formatter is RAW; InternalMin (:103-110) / InternalMax (:102-109): null, and no string, unless a value was
    collected."""
    if kind == N.AGG_VALUE_COUNT:
        body = '"value":%d' % value
    elif kind in (N.AGG_MIN, N.AGG_MAX) and math.isinf(value):
        return '{"value":null}'
    else:
        body = '"value":' + java_double(value)
    if value_as_string is not None:
        body += ',"value_as_string":"%s"' % value_as_string
    return "{" + body + "}"


def xcontent(tree, aggs):
    """The aggregations object of a (stats-twin derived) result tree without formatters: StringTerms
    (InternalTerms.java:220-229, StringTerms.java:138-148), InternalHistogram (:152-173, :526-541), the four."""
    def one(js, b):
        if b.type in SINGLE:
            return xcontent_single(b.type, js["value"])
        if b.type == N.AGG_TERMS:
            bks = ",".join('{"key":"%s","doc_count":%d%s}' % (bk["key"], bk["doc_count"], subs(bk, b)) for bk in js["buckets"])
            return '{"doc_count_error_upper_bound":%d,"sum_other_doc_count":%d,"buckets":[%s]}' % (
                js["doc_count_error_upper_bound"], js["sum_other_doc_count"], bks)
        if b.type == N.AGG_DATE_HISTOGRAM:
            bks = ",".join('{"key_as_string":"%s","key":%d,"doc_count":%d%s}' % (bk["key_as_string"], bk["key"], bk["doc_count"],
                                                                              subs(bk, b)) for bk in js["buckets"])
            return '{"buckets":[%s]}' % bks
        raise ValueError("no XContent writer for type %d" % b.type)

    def subs(bk, b):
        return "".join(',"%s":%s' % (s.name, one(bk[s.name], s)) for s in b.subs)

    return "{" + ",".join('"%s":%s' % (a.name, one(tree[a.name], a)) for a in aggs) + "}"


# ---- the library-private shard record of hand-built blocks ---------------------------------------------------------
def single(kind, name, value=None, **params):
    """A shard-level InternalSum / InternalMin / InternalMax / InternalValueCount instance for record(): the block fills
    the one array of its kind; the others hold the empty aggregation's values."""
    a = {"type": kind, "name": name, "count": 0, "sum": 0.0, "min": math.inf, "max": -math.inf}
    if value is not None:
        a[SINGLE[kind]] = value
    a.update(params)
    return a


def _block(b, insts):
    a = insts[0]
    t = a["type"]
    b += struct.pack("<ii", t, a.get("order", 0))
    RS._str(b, a["name"])
    b += struct.pack("<iiqii", a.get("required_size", 10), a.get("shard_size", 10), a.get("min_doc_count", 1),
                     a.get("show_err", 0), 0)
    b += struct.pack("<Biqq", 0, 0, 1, 0)
    RS._vec(b, "q", [])
    RS._vec(b, "q", [])
    b += struct.pack("<BBqq", 0, 0, 0, 0)
    b += struct.pack("<di", 2.0, 14)
    RS._str(b, a.get("order_path", ""))
    RS._fmt(b, a)
    b += struct.pack("<Q", len(insts))
    bucket = t == N.AGG_TERMS or "buckets" in a  # (buckets on a metric instance: a malformed record, for the reader's checks)
    buckets = [bk for x in insts for bk in x.get("buckets", [])]
    RS._vec(b, "q", [x.get("doc_count_error", 0) for x in insts] if bucket else [])
    RS._vec(b, "q", [x.get("other_doc_count", 0) for x in insts] if bucket else [])
    offs = [0]
    for x in insts:
        offs.append(offs[-1] + len(x.get("buckets", [])))
    RS._vec(b, "Q", offs if bucket else [])
    RS._vec(b, "q", list(range(len(buckets))))
    terms = [bk["term"].encode() for bk in buckets]
    toff = [0]
    for s in terms:
        toff.append(toff[-1] + len(s))
    RS._vec(b, "Q", toff if bucket else [])
    RS._str(b, b"".join(terms))
    RS._vec(b, "q", [bk["doc_count"] for bk in buckets])
    RS._vec(b, "q", [0 for _ in buckets])
    nsubs = len(buckets[0]["subs"]) if buckets else 0
    b += struct.pack("<I", nsubs)
    for j in range(nsubs):
        _block(b, [bk["subs"][j] for bk in buckets])
    b += struct.pack("<I", 0)
    metric = t != N.AGG_TERMS
    RS._vec(b, "q", [x["count"] for x in insts] if metric else [])
    RS._vec(b, "d", [x["sum"] for x in insts] if metric else [])
    RS._vec(b, "d", [x["min"] for x in insts] if metric else [])
    RS._vec(b, "d", [x["max"] for x in insts] if metric else [])
    RS._vec(b, "d", [0.0 for _ in insts] if metric else [])
    RS._vec(b, "B", [])
    RS._vec(b, "i", [])
    b += struct.pack("<QQ", 0, 0)


def record(aggs):
    """esgpu_result_serialize's format (version 5) of top-level instances: single(...) dicts, or a terms dict
    {"type": AGG_TERMS, "name", "buckets": [{"term", "doc_count", "subs": [single(...), ...]}], ...}."""
    b = bytearray(struct.pack("<II", RS.MAGIC, RS.VERSION))
    b += struct.pack("<I", len(aggs))
    for a in aggs:
        _block(b, [a])
    return bytes(b)
