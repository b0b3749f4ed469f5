"""Request builders mirroring the reference's Java API for this path.

    AggregationBuilders.terms("keys").field("key").size(3).shardSize(3).order(Terms.Order.count(False))
    AggregationBuilders.dateHistogram("histo").field("date").interval("1h").minDocCount(0)
    QueryBuilders.termQuery("status", 200), QueryBuilders.rangeQuery("bytes").gte(1024).lte(65536)

(core/src/main/java/org/elasticsearch/search/aggregations/AggregationBuilders.java and
core/src/main/java/org/elasticsearch/index/query/QueryBuilders.java).  `flatten()` applies the parser defaults
the reference applies before an AggregatorFactory exists (TermsParser.java:46-77 + BucketCountThresholds,
DateHistogramParser.java:85-193, CardinalityParser.java:48-71, ExtendedStatsParser.java:57) and produces the
flattened esgpu_agg_spec array of include/esgpu.h.
"""
import ctypes
import functools
import math
import re
import struct

from . import _native as N

# ---- DateHistogramParser.DATE_FIELD_UNITS (DateHistogramParser.java:50-69) ----
DATE_FIELD_UNITS = {
    "year": N.UNIT_YEAR, "1y": N.UNIT_YEAR, "quarter": N.UNIT_QUARTER, "1q": N.UNIT_QUARTER,
    "month": N.UNIT_MONTH, "1M": N.UNIT_MONTH, "week": N.UNIT_WEEK, "1w": N.UNIT_WEEK,
    "day": N.UNIT_DAY, "1d": N.UNIT_DAY, "hour": N.UNIT_HOUR, "1h": N.UNIT_HOUR,
    "minute": N.UNIT_MINUTE, "1m": N.UNIT_MINUTE, "second": N.UNIT_SECOND, "1s": N.UNIT_SECOND,
}

_TIME_UNITS_MS = {"ms": 1, "s": 1000, "m": 60000, "h": 3600000, "d": 86400000, "w": 7 * 86400000}


def parse_time_value(text):
    """TimeValue.parseTimeValue (common/unit/TimeValue.java:232-272): the lower-cased text's suffix picks the unit
    (ms, s, m, h, d, w in that order of tests), a bare number is milliseconds.  As in Java, seconds truncate the
    number before scaling ((long) 1.5 * 1000 = 1000); the other units scale, then truncate."""
    t = str(text).lower().strip()
    m = re.fullmatch(r"(-?\d+(?:\.\d*)?|-?\.\d+)(ms|s|m|h|d|w)?", t)
    if not m:
        raise ValueError(f"Failed to parse [{text}]")
    num, unit = m.group(1), m.group(2)
    if unit is None:
        if "." in num:
            raise ValueError(f"Failed to parse [{text}]")
        return int(num)
    if unit == "s":
        return int(float(num)) * 1000
    return int(float(num) * _TIME_UNITS_MS[unit])


def parse_offset(text):
    """DateHistogramParser.parseOffset: "-" negates, "+" is dropped, the rest is a TimeValue."""
    t = str(text)
    if t.startswith("-"):
        return -parse_time_value(t[1:])
    return parse_time_value(t[1:] if t.startswith("+") else t)


def parse_time_zone(tz):
    """DateTimeZone.forID: fixed offsets ("UTC", "+01:00", "-08:00", "-2") -> offset in ms; a region id
    ("Europe/Berlin", "America/Chicago", "CET") -> its offset history (tz_history)."""
    if tz is None or tz in ("UTC", "Z", "utc"):
        return 0
    m = re.fullmatch(r"([+-])?(\d{1,2})(?::?(\d{2}))?", tz)
    if not m:
        return tz_history(tz)
    sign = -1 if m.group(1) == "-" else 1
    return sign * (int(m.group(2)) * 3600000 + int(m.group(3) or 0) * 60000)


@functools.lru_cache(maxsize=64)
def tz_history(name, first_year=1900, last_year=2100):
    """Offset history of an IANA zone as the C-ABI takes it (esgpu_agg_spec.tz_starts / tz_offsets_ms): offset
    offs[i] applies from UTC instant starts[i] on (starts[0] = -infinity).  What a JNI caller reads from joda's
    DateTimeZone (getOffset / nextTransition), read here from the IANA database behind Python's zoneinfo: the offset
    is sampled every 6 hours over [first_year, last_year) and each change is bisected to the second."""
    import datetime as _dt
    import zoneinfo
    try:
        z = zoneinfo.ZoneInfo(name)
    except (zoneinfo.ZoneInfoNotFoundError, ValueError) as e:
        raise ValueError(f"The datetime zone id '{name}' is not recognised") from e
    epoch = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)

    def off(sec):
        return int((epoch + _dt.timedelta(seconds=sec)).astimezone(z).utcoffset().total_seconds() * 1000)

    lo = int((_dt.datetime(first_year, 1, 1, tzinfo=_dt.timezone.utc) - epoch).total_seconds())
    hi = int((_dt.datetime(last_year, 1, 1, tzinfo=_dt.timezone.utc) - epoch).total_seconds())
    step = 6 * 3600
    starts, offs = [-(1 << 63)], [off(lo)]
    prev = offs[0]
    t = lo
    while t < hi:
        nxt = t + step
        o = off(nxt)
        if o != prev:
            a, b = t, nxt  # off(a) == prev != off(b): the transition instant is in (a, b]
            while b - a > 1:
                mid = (a + b) // 2
                if off(mid) == prev:
                    a = mid
                else:
                    b = mid
            starts.append(b * 1000)
            offs.append(off(b))
            prev = offs[-1]
            if o != prev:  # two changes inside one step: rescan from the transition
                t = b
                continue
        t = nxt
    return tuple(starts), tuple(offs)


class AggOrder:
    def __init__(self, path, asc):
        self.path, self.asc = path, bool(asc)


def order_code(o):
    """-> (ESGPU_ORDER_*, order path or None)"""
    if isinstance(o, AggOrder):
        return (N.ORDER_AGG_ASC if o.asc else N.ORDER_AGG_DESC), o.path
    return o, None


class Order:
    """Terms.Order (InternalOrder.java) and Histogram.Order."""

    @staticmethod
    def count(asc):
        return N.ORDER_COUNT_ASC if asc else N.ORDER_COUNT_DESC

    @staticmethod
    def term(asc):
        return N.ORDER_TERM_ASC if asc else N.ORDER_TERM_DESC

    @staticmethod
    def aggregation(path, asc):
        """Terms.Order.aggregation: order by a metric sub-aggregation, "avg_rt" or "rt.max" (InternalOrder.Aggregation)."""
        return AggOrder(path, asc)

    KEY_ASC = N.ORDER_KEY_ASC
    KEY_DESC = N.ORDER_KEY_DESC
    COUNT_ASC = N.ORDER_HCOUNT_ASC
    COUNT_DESC = N.ORDER_HCOUNT_DESC


class _Builder:
    type = 0

    def __init__(self, name):
        self.name = name
        self._field = None
        self._format = None
        self.subs = []

    def field(self, f):
        self._field = f
        return self

    def format(self, pattern):
        """the request's "format" (ValuesSourceParser formattable aggregations): a date pattern on a date field, a
        DecimalFormat pattern on a numeric one"""
        self._format = pattern
        return self

    def subAggregation(self, sub):  # noqa: N802 - mirrors the Java API
        self.subs.append(sub)
        return self

    sub_aggregation = subAggregation


class TermsBuilder(_Builder):
    type = N.AGG_TERMS

    def __init__(self, name):
        super().__init__(name)
        self._size, self._shard_size, self._min, self._shard_min = 10, -1, -1, -1
        self._order = N.ORDER_COUNT_DESC
        self._show_err = False

    def size(self, n):
        self._size = n
        return self

    def shardSize(self, n):  # noqa: N802
        self._shard_size = n
        return self

    def minDocCount(self, n):  # noqa: N802
        self._min = n
        return self

    def shardMinDocCount(self, n):  # noqa: N802
        self._shard_min = n
        return self

    def order(self, o):
        self._order = o
        return self

    def showTermDocCountError(self, b):  # noqa: N802
        self._show_err = bool(b)
        return self

    shard_size = shardSize
    min_doc_count = minDocCount


class HistogramBuilder(_Builder):
    type = N.AGG_HISTOGRAM

    def __init__(self, name):
        super().__init__(name)
        self._interval = None
        self._offset = 0
        self._min = 0  # HistogramParser / DateHistogramParser: min_doc_count default 0
        self._order = N.ORDER_KEY_ASC
        self._keyed = False
        self._bounds = (None, None)

    def interval(self, i):
        self._interval = i
        return self

    def offset(self, o):
        self._offset = o
        return self

    def minDocCount(self, n):  # noqa: N802
        self._min = n
        return self

    def order(self, o):
        self._order = o
        return self

    def keyed(self, k):
        self._keyed = bool(k)
        return self

    def extendedBounds(self, lo, hi):  # noqa: N802
        self._bounds = (lo, hi)
        return self

    min_doc_count = minDocCount


class DateHistogramBuilder(HistogramBuilder):
    type = N.AGG_DATE_HISTOGRAM

    def __init__(self, name):
        super().__init__(name)
        self._tz = None

    def timeZone(self, tz):  # noqa: N802
        self._tz = tz
        return self

    time_zone = timeZone


class _MetricBuilder(_Builder):
    def subAggregation(self, sub):  # noqa: N802
        raise ValueError("Aggregator [%s] of type [%d] cannot accept sub-aggregations" % (self.name, self.type))


class StatsBuilder(_MetricBuilder):
    type = N.AGG_STATS


class ExtendedStatsBuilder(_MetricBuilder):
    type = N.AGG_EXTENDED_STATS

    def __init__(self, name):
        super().__init__(name)
        self._sigma = 2.0

    def sigma(self, s):
        if s < 0:
            raise ValueError("[sigma] must not be negative")
        self._sigma = float(s)
        return self


class AvgBuilder(_MetricBuilder):
    type = N.AGG_AVG


class SumBuilder(_MetricBuilder):
    """sum (SumAggregator / InternalSum): {"value": the sum of the field's values, 0.0 when there are none}"""
    type = N.AGG_SUM


class MinBuilder(_MetricBuilder):
    """min (MinAggregator / InternalMin): +Infinity when no doc has a value (XContent: null)"""
    type = N.AGG_MIN


class MaxBuilder(_MetricBuilder):
    """max (MaxAggregator / InternalMax): -Infinity when no doc has a value (XContent: null)"""
    type = N.AGG_MAX


class ValueCountBuilder(_MetricBuilder):
    """value_count (ValueCountAggregator / InternalValueCount): the number of values, over numeric and keyword fields"""
    type = N.AGG_VALUE_COUNT


class CardinalityBuilder(_MetricBuilder):
    type = N.AGG_CARDINALITY

    def __init__(self, name):
        super().__init__(name)
        self._threshold = -1

    def precisionThreshold(self, t):  # noqa: N802
        self._threshold = int(t)
        return self

    precision_threshold = precisionThreshold


class FilterBuilder(_Builder):
    """filter aggregation (FilterAggregator / InternalFilter): one bucket of the docs matching `query` -- a TermQuery,
    a RangeQuery or a list of them (bool.filter conjunction), or, at the top level, any leaf or BoolQuery -- with
    sub-aggregations.  On the GPU path at the top level
    (any sub-aggregations) or directly under a top-level bucket aggregation (metric sub-aggregations)."""
    type = N.AGG_FILTER

    def __init__(self, name, query=None):
        super().__init__(name)
        self._query = query

    def filter(self, query):
        self._query = query
        return self

    def clauses(self):
        q = self._query
        if q is None:
            raise ValueError("[filter] aggregation [%s] requires a filter" % self.name)
        return list(q) if isinstance(q, (list, tuple)) else [q]


class RangeBuilder(_Builder):
    """range aggregation (RangeAggregator / InternalRange): one bucket per [from, to) over a long, date or double field,
    every range emitted, sorted by (from, to).  On the GPU path at the top level with numeric metric sub-aggregations
    and with date_histogram sub-aggregations of numeric metrics (one histogram per range; over a single-valued range
    field).  A numeric histogram, terms, filter, range, filters or cardinality child stays on the CPU path."""
    type = N.AGG_RANGE

    def __init__(self, name):
        super().__init__(name)
        self._ranges = []  # (key or None, from, to) in request order
        self._keyed = False

    @staticmethod
    def _key_and(args, n):
        if len(args) == n + 1:
            return (args[0],) + tuple(float(a) for a in args[1:])
        if len(args) != n:
            raise TypeError("expected [key,] and %d bound(s)" % n)
        return (None,) + tuple(float(a) for a in args)

    def addRange(self, *args):  # noqa: N802 -- addRange([key,] from, to)
        key, lo, hi = self._key_and(args, 2)
        self._ranges.append((key, lo, hi))
        return self

    def addUnboundedTo(self, *args):  # noqa: N802 -- addUnboundedTo([key,] to): (-inf, to)
        key, hi = self._key_and(args, 1)
        self._ranges.append((key, float("-inf"), hi))
        return self

    def addUnboundedFrom(self, *args):  # noqa: N802 -- addUnboundedFrom([key,] from): [from, +inf)
        key, lo = self._key_and(args, 1)
        self._ranges.append((key, lo, float("inf")))
        return self

    def keyed(self, k):
        self._keyed = bool(k)
        return self

    add_range = addRange
    add_unbounded_to = addUnboundedTo
    add_unbounded_from = addUnboundedFrom


class FiltersBuilder(_Builder):
    """filters aggregation (FiltersAggregator / InternalFilters, FiltersAggregationBuilder): one bucket per filter, in
    request order, a doc in every bucket whose filter it matches, and optionally the "other" bucket of the docs matching
    none.  filter(key, query) adds a named filter (a repeated key replaces the query and keeps its position),
    filter(query) an anonymous one (keys "0", "1", ...); a query is a TermQuery, a RangeQuery or a list of them (their
    conjunction; the empty list is match_all).  On the GPU path at the top level with numeric metric sub-aggregations
    and with date_histogram sub-aggregations of numeric metrics (one histogram per bucket, the other bucket included).
    A numeric histogram, terms, filter, range, filters or cardinality child stays on the CPU path."""
    type = N.AGG_FILTERS

    def __init__(self, name):
        super().__init__(name)
        self._keyed_filters = {}  # key -> query, in insertion order (FiltersAggregationBuilder's LinkedHashMap)
        self._anon_filters = []
        self._other = False
        self._other_key = None

    def filter(self, *args):
        if len(args) == 2:
            self._keyed_filters[str(args[0])] = args[1]
        elif len(args) == 1:
            self._anon_filters.append(args[0])
        else:
            raise TypeError("expected filter([key,] query)")
        return self

    def otherBucket(self, other):  # noqa: N802
        self._other = bool(other)
        return self

    def otherBucketKey(self, key):  # noqa: N802 -- FiltersParser.java:104-107: a key implies the other bucket
        self._other_key = str(key)
        self._other = True
        return self

    other_bucket = otherBucket
    other_bucket_key = otherBucketKey

    def filters(self):
        """-> (keyed, [(key, [clauses])]) in bucket order; ValueError as FiltersAggregationBuilder.internalXContent
        throws (:97-101): no filter at all, or keyed and anonymous filters mixed"""
        if not self._keyed_filters and not self._anon_filters:
            raise ValueError("At least one filter must be set on filter aggregation [%s]" % self.name)
        if self._keyed_filters and self._anon_filters:
            raise ValueError("Cannot add both keyed and non-keyed filters to filters aggregation [%s]" % self.name)
        as_list = lambda q: list(q) if isinstance(q, (list, tuple)) else [q]  # noqa: E731
        if self._keyed_filters:
            return True, [(k, as_list(q)) for k, q in self._keyed_filters.items()]
        return False, [(str(i), as_list(q)) for i, q in enumerate(self._anon_filters)]


class AggregationBuilders:
    terms = TermsBuilder
    filter = FilterBuilder
    filters = FiltersBuilder
    range = RangeBuilder
    histogram = HistogramBuilder
    dateHistogram = DateHistogramBuilder
    date_histogram = DateHistogramBuilder
    stats = StatsBuilder
    extendedStats = ExtendedStatsBuilder
    extended_stats = ExtendedStatsBuilder
    avg = AvgBuilder
    sum = SumBuilder
    min = MinBuilder
    max = MaxBuilder
    count = ValueCountBuilder  # AggregationBuilders.count(name) builds the value_count aggregation
    cardinality = CardinalityBuilder


# ---- queries: term / range / terms / exists leaves and bool (a list is a conjunction: bool.filter) ----
class TermQuery:
    def __init__(self, field, value):
        self.field, self.value = field, value


class RangeQuery:
    def __init__(self, field):
        self.field = field
        self.lo = self.hi = None
        self.include_lower = self.include_upper = True

    def gte(self, v):
        self.lo, self.include_lower = v, True
        return self

    def gt(self, v):
        self.lo, self.include_lower = v, False
        return self

    def lte(self, v):
        self.hi, self.include_upper = v, True
        return self

    def lt(self, v):
        self.hi, self.include_upper = v, False
        return self

    def from_(self, v, include=True):
        self.lo, self.include_lower = v, include
        return self

    def to(self, v, include=True):
        self.hi, self.include_upper = v, include
        return self


class TermsQuery:
    """terms (TermsQueryBuilder): the doc's value is one of `values`; an empty list matches no doc"""

    def __init__(self, field, values):
        self.field, self.values = field, list(values)


class ExistsQuery:
    """exists (ExistsQueryBuilder): the doc has a value in the field"""

    def __init__(self, field):
        self.field = field


class BoolQuery:
    """bool (BoolQueryBuilder): must and filter clauses are required alike (nothing is scored), must_not clauses
    prohibited, should clauses optional; minimum_should_match as Queries.calculateMinShouldMatch reads it (an int or a
    string: "2", "-1", "75%", "-25%", "3<90%", "2<-25% 9<-3")."""

    def __init__(self):
        self.must_clauses, self.filter_clauses, self.should_clauses, self.must_not_clauses = [], [], [], []
        self._msm = None       # the minimum_should_match spec as given, or None
        self._adjust = True    # adjust_pure_negative

    def must(self, q):
        self.must_clauses.append(q)
        return self

    def filter(self, q):
        self.filter_clauses.append(q)
        return self

    def should(self, q):
        self.should_clauses.append(q)
        return self

    def mustNot(self, q):  # noqa: N802
        self.must_not_clauses.append(q)
        return self

    def minimumShouldMatch(self, spec):  # noqa: N802
        self._msm = None if spec is None else str(spec)
        return self

    def adjustPureNegative(self, adjust):  # noqa: N802
        self._adjust = bool(adjust)
        return self

    must_not = mustNot
    minimum_should_match = minimumShouldMatch
    adjust_pure_negative = adjustPureNegative


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def calculate_min_should_match(optional_clause_count, spec):
    """Queries.calculateMinShouldMatch (common/lucene/search/Queries.java:142-177), its float32 arithmetic and its
    truncation toward zero included.  A malformed spec raises ValueError, as Integer.parseInt throws."""
    result = n = int(optional_clause_count)
    spec = str(spec).strip()
    if "<" in spec:  # conditional spec(s)
        spec = re.sub(r"(\s+<\s*)|(\s*<\s+)", "<", spec)
        for s in spec.split(" "):
            parts = [x for x in s.split("<")]
            while parts and parts[-1] == "":  # String.split(regex, 0) drops trailing empty strings
                parts.pop()
            upper = int(parts[0])
            if n <= upper:
                return result
            result = calculate_min_should_match(n, parts[1])
        return result
    if "%" in spec:
        percent = int(spec[:-1])
        calc = _f32(_f32(float(result * percent)) * _f32(1 / _f32(100.0)))
        result = result + int(calc) if calc < 0 else int(calc)  # (int) of a float truncates toward zero, as int() does
    else:
        calc = int(spec)
        result = result + calc if calc < 0 else calc
    return n if n < result else (0 if result < 0 else result)


class QueryBuilders:
    @staticmethod
    def termQuery(field, value):  # noqa: N802
        return TermQuery(field, value)

    @staticmethod
    def rangeQuery(field):  # noqa: N802
        return RangeQuery(field)

    @staticmethod
    def termsQuery(field, values):  # noqa: N802
        return TermsQuery(field, values)

    @staticmethod
    def existsQuery(field):  # noqa: N802
        return ExistsQuery(field)

    @staticmethod
    def missingQuery(field):  # noqa: N802 -- MissingQueryBuilder's defaults (existence true, null_value false)
        return BoolQuery().mustNot(ExistsQuery(field))

    @staticmethod
    def boolQuery():  # noqa: N802
        return BoolQuery()

    term_query = termQuery
    range_query = rangeQuery
    terms_query = termsQuery
    exists_query = existsQuery
    missing_query = missingQuery
    bool_query = boolQuery


# ---- flattening -------------------------------------------------------------------------------------------------
def _rounding_params(b):
    """-> (date_unit, interval, offset, zone) with a fixed time-zone offset folded into OffsetRounding; zone is None
    or the (starts, offsets) history of a region zone (DateHistogramParser.java:178-187)."""
    if b.type == N.AGG_HISTOGRAM:
        if b._interval is None or int(b._interval) < 1:
            raise ValueError("[interval] must be 1 or greater for histogram aggregation [%s]" % b.name)
        return N.UNIT_NONE, int(b._interval), int(b._offset), None
    if b._interval is None:
        raise ValueError("Missing required field [interval] for histogram aggregation [%s]" % b.name)
    off = b._offset if isinstance(b._offset, int) else parse_offset(b._offset)
    tz = parse_time_zone(b._tz)
    zone = None
    if isinstance(tz, tuple):
        zone = tz
    elif tz != 0:  # a fixed zone as a one-entry table: Rounding.from_spec folds it into the offset, and the result
        zone = ((0,), (tz,))  # keeps it for printing the keys (key_as_string "...+01:00")
    unit = DATE_FIELD_UNITS.get(str(b._interval))
    if unit is not None:
        return unit, 0, off, zone
    return N.UNIT_NONE, parse_time_value(b._interval), off, zone


# The index mapping behind the synthetic log documents: "@timestamp" is a date field with the
# default date format; every other numeric field is a long / double / murmur3 (NumberFieldType).  A JNI caller reads
# both from the field's MappedFieldType instead.
DATE_FIELDS = {"@timestamp": "strict_date_optional_time||epoch_millis"}  # DateFieldMapper.Defaults.DATE_TIME_FORMATTER


def time_zone_id(tz):
    """DateTimeZone.forID(tz).getID(): "UTC" for a zero offset, "+hh:mm" / "-hh:mm" for a fixed one, a region id as
    given.  None = UTC (ValuesSourceParser's default)."""
    if tz is None:
        return "UTC"
    off = parse_time_zone(tz)
    if isinstance(off, tuple):
        return str(tz)
    if off == 0:
        return "UTC"
    a = abs(off)
    return "%s%02d:%02d" % ("-" if off < 0 else "+", a // 3600000, a // 60000 % 60)


def _value_format(b):
    """ValuesSourceParser.resolveFormat (ValuesSourceParser.java:244-257): (ESGPU_FORMAT_*, pattern)"""
    if b._field in DATE_FIELDS:
        return N.FORMAT_DATE_TIME, b._format or DATE_FIELDS[b._field]
    if b._format is not None:
        return N.FORMAT_NUMBER, b._format
    return N.FORMAT_RAW, None


def _round_bound(spec, v):
    """ExtendedBounds.round: the bound is rounded with the aggregation's own Rounding (esgpu_date_rounding)."""
    if v is None:
        return None
    out = ctypes.c_int64()
    N.check(N.lib().esgpu_date_rounding(ctypes.byref(spec), 0, int(v), ctypes.byref(out)))
    return out.value


def thresholds(size, shard_size, min_doc_count, shard_min_doc_count, order, number_of_shards):
    out = [ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()]
    N.check(N.lib().esgpu_terms_thresholds(size, shard_size, min_doc_count, shard_min_doc_count, order,
                                           number_of_shards, *[ctypes.byref(x) for x in out]))
    return tuple(x.value for x in out)


def flatten(aggs, number_of_shards=1):
    """Builders -> ctypes array of AggSpec (parents before children, parser defaults applied)."""
    specs = []
    keep = []  # keep the encoded names alive

    def enc(s):
        b = s.encode("utf-8") if s is not None else None
        keep.append(b)
        return b

    def visit(b, parent):
        sp = N.AggSpec()
        sp.type = b.type
        sp.parent = parent
        sp.name = enc(b.name)
        sp.field = enc(b._field)
        sp.sigma = 2.0
        sp.precision_threshold = -1
        if b.type != N.AGG_FILTER:
            fmt, pattern = _value_format(b)
            sp.value_format = fmt
            sp.format = enc(pattern)
            # the request time zone reaches the formatter through ValuesSourceParser.Input.timezone: date_histogram only
            sp.time_zone = enc(time_zone_id(b._tz) if b.type == N.AGG_DATE_HISTOGRAM else "UTC")
        if b.type == N.AGG_TERMS:
            code, path = order_code(b._order)
            size, ssize, mn, smn = thresholds(b._size, b._shard_size, b._min, b._shard_min, code, number_of_shards)
            sp.size, sp.shard_size, sp.min_doc_count, sp.shard_min_doc_count = size, ssize, mn, smn
            sp.order = code
            if path is not None:
                sp.order_path = enc(path)
            sp.show_term_doc_count_error = int(b._show_err)
        elif b.type in (N.AGG_HISTOGRAM, N.AGG_DATE_HISTOGRAM):
            unit, interval, off, zone = _rounding_params(b)
            sp.date_unit, sp.interval, sp.offset = unit, interval, off
            if zone is not None:
                starts = (ctypes.c_int64 * len(zone[0]))(*zone[0])
                offs = (ctypes.c_int64 * len(zone[1]))(*zone[1])
                keep.extend([starts, offs])
                sp.tz_starts = ctypes.cast(starts, ctypes.POINTER(ctypes.c_int64))
                sp.tz_offsets_ms = ctypes.cast(offs, ctypes.POINTER(ctypes.c_int64))
                sp.tz_count = len(zone[0])
            sp.min_doc_count = b._min
            sp.order = b._order
            sp.keyed = int(b._keyed)
            lo, hi = b._bounds
            if lo is not None:
                sp.has_extended_bounds_min = 1
                sp.extended_bounds_min = _round_bound(sp, lo)
            if hi is not None:
                sp.has_extended_bounds_max = 1
                sp.extended_bounds_max = _round_bound(sp, hi)
        elif b.type == N.AGG_RANGE:
            sp.keyed = int(b._keyed)
            rs = (N.Range * max(len(b._ranges), 1))()
            for k, (key, lo, hi) in enumerate(b._ranges):
                rs[k].key, rs[k].from_, rs[k].to = enc(key), lo, hi
            keep.append(rs)
            sp.ranges = ctypes.cast(rs, ctypes.POINTER(N.Range))
            sp.n_ranges = len(b._ranges)
        elif b.type == N.AGG_FILTERS:
            keyed, flt = b.filters()
            sp.keyed = int(keyed)
            ks = (ctypes.c_char_p * len(flt))(*[enc(k) for k, _q in flt])
            keep.append(ks)
            sp.filter_keys = ctypes.cast(ks, ctypes.POINTER(ctypes.c_char_p))
            sp.n_filters = len(flt)
            sp.other_bucket = int(b._other)
            sp.other_bucket_key = enc(b._other_key)
        elif b.type == N.AGG_EXTENDED_STATS:
            sp.sigma = b._sigma
        elif b.type == N.AGG_CARDINALITY:
            sp.precision_threshold = b._threshold
        idx = len(specs)
        specs.append(sp)
        for s in b.subs:
            visit(s, idx)

    for a in aggs:
        visit(a, -1)
    arr = (N.AggSpec * max(len(specs), 1))(*specs)
    return arr, len(specs), keep


def _preorder(aggs):
    """(builder, spec index) in flatten()'s order (parents before children, depth first)."""
    out = []

    def visit(b):
        out.append(b)
        for s in b.subs:
            visit(s)

    for a in aggs or []:
        visit(a)
    return [(b, i) for i, b in enumerate(out)]


def _bound_i64(v):
    """lo_i / hi_i of a range bound.  An infinite bound travels in lo_d / hi_d, which every column type reads for it
    (include/esgpu.h); the long beside it only has to fit the field.  A NaN bound raises, as int() does."""
    if isinstance(v, float) and math.isinf(v):
        return (1 << 63) - 1 if v > 0 else -(1 << 63)
    return int(v)


_LEAVES = (TermQuery, RangeQuery, TermsQuery, ExistsQuery)


def _nesting(what):
    return N.UnsupportedOnGpu(N.ERR_UNSUPPORTED, "%s: this bool nesting runs on the CPU path" % what)


def _is_should_group(q):
    """a nested bool of only should leaves whose minimum_should_match is unset or asks for one: it holds when any of its
    leaves holds"""
    if not isinstance(q, BoolQuery) or q.must_clauses or q.filter_clauses or q.must_not_clauses or not q.should_clauses:
        return False
    if not all(isinstance(c, _LEAVES) for c in q.should_clauses):
        return False
    return q._msm is None or calculate_min_should_match(len(q.should_clauses), q._msm) in (0, 1)  # (0: the default, one)


def lower_query(query, keep_empty=False):
    """One owner's query -- a leaf, a list (a conjunction: bool.filter) or a BoolQuery -- in the normal form of
    include/esgpu.h "Query filters": -> ([(leaf, occur, group)], options), options = (resolved minimum_should_match or
    -1, adjust_pure_negative) for bool form and None for plain form (only required term / range leaves; an owner
    without a clause is plain unless keep_empty: a filter aggregation's match_all needs its options record).
    A clause that is itself a bool becomes a group in its position when it is a bool of only should leaves
    (minimum_should_match unset or 1), and is flattened when it is a bool of only must / filter clauses in a must /
    filter position; any other nesting raises UnsupportedOnGpu."""
    while isinstance(query, (list, tuple)) and len(query) == 1:
        query = query[0]  # (a conjunction of one clause is that clause)
    if isinstance(query, (list, tuple)):
        top = BoolQuery()
        top.filter_clauses = list(query)
    elif isinstance(query, BoolQuery):
        top = query
    else:
        top = BoolQuery().filter(query)
    clauses, groups = [], [0]

    def group_of(q, occur):
        groups[0] += 1
        clauses.extend((leaf, occur, groups[0]) for leaf in q.should_clauses)

    def required(q):
        if isinstance(q, _LEAVES):
            clauses.append((q, N.OCCUR_MUST, 0))
        elif isinstance(q, (list, tuple)) and len(q) > 0:
            for c in q:
                required(c)
        elif _is_should_group(q):
            group_of(q, N.OCCUR_MUST)
        elif (isinstance(q, BoolQuery) and (q.must_clauses or q.filter_clauses) and not q.should_clauses
              and not q.must_not_clauses):
            for c in q.must_clauses + q.filter_clauses:
                required(c)
        else:
            raise _nesting("a must / filter clause that is neither a leaf, a conjunction nor a bool of should leaves")

    for c in top.must_clauses + top.filter_clauses:
        required(c)
    for occur, cs, name in ((N.OCCUR_SHOULD, top.should_clauses, "should"), (N.OCCUR_MUST_NOT, top.must_not_clauses, "must_not")):
        for c in cs:
            if isinstance(c, _LEAVES):
                clauses.append((c, occur, 0))
            elif _is_should_group(c):
                group_of(c, occur)
            else:
                raise _nesting("a %s clause that is neither a leaf nor a bool of should leaves" % name)
    plain = all(isinstance(q, (TermQuery, RangeQuery)) and occur == N.OCCUR_MUST and group == 0 for q, occur, group in clauses)
    if plain and (clauses or not keep_empty):
        return clauses, None
    msm = -1 if top._msm is None else calculate_min_should_match(len(top.should_clauses), top._msm)
    return clauses, (msm, top._adjust)


def flatten_filters(queries, ord_lookup=None, aggs=None):
    """Queries -> ctypes array of Filter.  `ord_lookup(field, term) -> ordinal or -1` resolves keyword terms.  With
    `aggs`, the clauses of every filter aggregation follow, each tagged with its owner (spec index + 1), and those of
    every filters aggregation, tagged with the owner and the slot of their filter."""
    out, keep = [], []
    tagged = []  # (leaf or None for an owner's options record, owner, slot, occur, group, (msm, adjust))

    def add_owner(query, owner, slot, keep_empty=False):
        clauses, options = lower_query(query, keep_empty)
        tagged.extend((q, owner, slot, occur, group, None) for q, occur, group in clauses)
        if options is not None:
            tagged.append((None, owner, slot, 0, 0, options))

    add_owner(BoolQuery() if queries is None else queries, 0, 0)
    for b, i in _preorder(aggs):
        if b.type == N.AGG_FILTER:
            q = b._query
            if q is None:
                raise ValueError("[filter] aggregation [%s] requires a filter" % b.name)
            add_owner(q, i + 1, 0, keep_empty=isinstance(q, BoolQuery))  # (an empty bool is match_all)
        elif b.type == N.AGG_FILTERS:
            for slot, (_key, qs) in enumerate(b.filters()[1]):
                add_owner(qs, i + 1, slot)

    def term_value(field, v):
        if isinstance(v, str):
            if ord_lookup is None:
                raise ValueError("keyword term filters need an ordinal lookup")
            v = ord_lookup(field, v)
        return int(v)

    for q, owner, slot, occur, group, options in tagged:
        f = N.Filter()
        f.owner = owner
        f.slot = slot
        f.occur = occur
        f.group = group
        if q is None:  # the owner's options: the resolved minimum_should_match (-1: not given), adjust_pure_negative
            f.type = N.FILTER_BOOL
            f.term, f.include_lower = options[0], int(options[1])
            out.append(f)
            continue
        b = q.field.encode("utf-8")
        keep.append(b)
        f.field = b
        if isinstance(q, ExistsQuery):
            f.type = N.FILTER_EXISTS
        elif isinstance(q, TermsQuery):
            f.type = N.FILTER_TERMS
            vals = (ctypes.c_int64 * max(len(q.values), 1))(*[term_value(q.field, v) for v in q.values])
            keep.append(vals)
            f.terms = ctypes.cast(vals, ctypes.POINTER(ctypes.c_int64))
            f.n_terms = len(q.values)
        elif isinstance(q, TermQuery):
            f.type = N.FILTER_TERM
            v = q.value
            if isinstance(v, str):
                if ord_lookup is None:
                    raise ValueError("keyword term filters need an ordinal lookup")
                v = ord_lookup(q.field, v)
            f.term = int(v)
        else:
            f.type = N.FILTER_RANGE
            if q.lo is not None:
                f.has_lower, f.include_lower = 1, int(q.include_lower)
                if isinstance(q.lo, (str, bytes)):  # TermRangeQuery on a keyword field
                    b = q.lo.encode("utf-8") if isinstance(q.lo, str) else bytes(q.lo)
                    keep.append(b)
                    f.lo_term, f.lo_term_len = b, len(b)
                else:
                    f.lo_i, f.lo_d = _bound_i64(q.lo), float(q.lo)
            if q.hi is not None:
                f.has_upper, f.include_upper = 1, int(q.include_upper)
                if isinstance(q.hi, (str, bytes)):
                    b = q.hi.encode("utf-8") if isinstance(q.hi, str) else bytes(q.hi)
                    keep.append(b)
                    f.hi_term, f.hi_term_len = b, len(b)
                else:
                    f.hi_i, f.hi_d = _bound_i64(q.hi), float(q.hi)
        out.append(f)
    arr = (N.Filter * max(len(out), 1))(*out)
    return arr, len(out), keep
