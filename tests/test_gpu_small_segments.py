"""GPU parity on tiny and ragged segments: every collect path over a ladder of segment sizes from 1 to 16,385 docs.

A shard that is being written to gets a new tiny segment at every refresh, and through global ordinals a 3-doc segment
can come with a 300,000-term dictionary.  The request tables and the column generators live in
tests/small_segment_cases.py (the host-side test runs them through the oracle alone).  Per group, layout and ladder size:
a fresh segment is uploaded -- so its compact copies, block deltas, zone keys, value-count products, term ranks, numeric
ordinals and hot/cold statistics are built at that size --, every request of the group is collected twice (the second
time after plan.reset(), over the cached products), and the shard result and its reduce are compared with the oracle's
under the suite's parity rules (bit-exact; the double column within 1e-12).  The collect path the plan reports is
asserted against the path restated from the gates of esgpu_runtime.cpp (small_segment_cases.path_*).

Long terms and sum / min / max / value_count leaves have no aggregator in the oracle: their reference is the keyword
twin and the stats twin of the request (tests/test_gpu_long_terms.py, tests/single_metric_stream.py).

Where the behaviour at small n differs by design:
  * ranked terms (path 10) and packed cells need the packed layouts; at 1 doc the grid has one key, so the 40-day
    variants take the LDS grid (1) where every larger size takes the key window (2);
  * a high-cardinality terms request is settled by the hot slots (8 / 9) only once shard_size terms occur in the segment;
    below, and with every doc missing, it takes the postings (7) or the scatter form (6);
  * accept bits within one bitset word (n <= 64) always count as "few deletions" (7 instead of 6);
  * terms over @timestamp keep their cells in LDS up to 5,485 distinct values and in global memory (0) above;
  * path 4 (partitioned counting) is not reachable: it runs only where the hot/cold statistics refuse a column, from
    2^25 terms up (esgpu_runtime.cpp:2143-2144).
"""
import contextlib

import pytest

import small_segment_cases as C
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from helpers import assert_same
from small_segment_cases import LADDER
from test_gpu_layouts import layout

pytestmark = pytest.mark.gpu

_seen_paths = set()


@contextlib.contextmanager
def device_errors_end_the_session(what):
    """a device error (a kernel fault surfaces as ESGPU_ERR_DEVICE) leaves the context unusable: nothing more is started
    on the GPU -- the session ends here with the case that met it, instead of every later test failing on a dead device"""
    try:
        yield
    except N.EsGpuError as e:
        if e.code == N.ERR_DEVICE:
            pytest.exit("device error in %s: %s" % (what(), e), returncode=3)
        raise


def _set_env(monkeypatch, case):
    if case.defer_env:  # terms under terms collected breadth-first whatever the grid size (tests/test_gpu_breadth_first.py)
        monkeypatch.setenv("ESGPU_DEFER_CELLS", "1")
    else:
        monkeypatch.delenv("ESGPU_DEFER_CELLS", raising=False)


def _compare(res, want, tag, exact, problems):
    try:
        assert_same(res.to_dict(), want["shards"][0], tag + " shard", exact)
        assert_same(reduce([res]).to_dict(), want["reduced"], tag + " reduced", exact)
    except AssertionError as e:
        problems.append(str(e)[:400])


def _check_case(engine, case, n, seg, name, problems):
    want = C.reference(case, n)
    cols = case.columns(n)
    expect = case.path(n, name, cols)
    bits = case.accept_bits(n)
    engine.set_option("ranked_terms", 1 if case.ranked else 0)
    plan = engine.plan(case.aggs(), filters=case.filters)
    try:
        for turn in ("first collect", "after reset"):
            tag = "%s n=%d %s %s" % (case.name, n, name, turn)
            with device_errors_end_the_session(lambda: tag):
                if turn != "first collect":
                    plan.reset()
                plan.collect(seg, accept_bits=bits)
                path = plan.last_collect_stats()[2]
                _seen_paths.add(path)
                if path != expect:
                    problems.append("%s: collect path %d, expected %d" % (tag, path, expect))
                _compare(plan.build(), want, tag, case.exact, problems)
    finally:
        plan.close()
        engine.set_option("ranked_terms", 1)


def _run_group(engine, monkeypatch, group, name, sizes=LADDER):
    cases = C.GROUPS[group]()
    fields = {}
    for c in cases:  # one segment per column set (dense / 40-day timestamps / a high-cardinality dictionary)
        fields.setdefault((c.wide, c.hc), set()).update(c.fields)
    problems = []
    with layout(engine, name):
        for n in sizes:
            segs = {}
            try:
                for case in cases:
                    key = (case.wide, case.hc)
                    if key not in segs:
                        cols = case.columns(n)
                        with device_errors_end_the_session(lambda: "upload n=%d %s" % (n, name)):
                            segs[key] = engine.upload_segment({f: cols[f] for f in sorted(fields[key])}, n)
                    _set_env(monkeypatch, case)
                    _check_case(engine, case, n, segs[key], name, problems)
            finally:
                for s in segs.values():
                    s.close()
    assert not problems, "%d mismatches, the first ones:\n%s" % (len(problems), "\n".join(problems[:12]))


@pytest.mark.parametrize("name", C.LAYOUTS)
@pytest.mark.parametrize("group", sorted(C.GROUPS))
def test_ladder(engine, monkeypatch, group, name):
    """a: the north star, ranked / every term / filtered, over dense and (a40d_*) 40-day timestamps; b: histogram-only grids; c: terms
    in each order with min_doc_count 0, fewer docs than terms; d: sparse everything and the two extremes; e: the double
    metric (compensated sums); f: multi-valued columns and the value-count product's three sources; g: cardinality at
    the root and under terms, linear counting and HLL; h: LongTerms over the bitmap and the open-addressing ordinals;
    i: 70,000 and 300,000 terms with few docs; j: terms under terms, depth-first and breadth-first, and three levels"""
    _run_group(engine, monkeypatch, group, name)


@pytest.mark.parametrize("name", C.LAYOUTS)
def test_all_ones_product_after_a_sparse_segment(engine, name):
    """a lone value_count whose first segment's metric is sparse (its product: the present bitset) and whose second
    segment's is dense (the all-ones product, value_counts_ones_kernel), in one plan; at the root and under terms"""
    problems = []
    aggs = [AB.terms("t").field("kw12").size(12).subAggregation(AB.count("vc").field("m")), AB.count("all").field("m")]
    case = C.Case("all_ones", lambda F: aggs, ("kw12", "m"), None, sm=True)
    with layout(engine, name):
        for i, n in enumerate(LADDER):
            n2 = LADDER[-1 - i]
            a, b = C.columns(n), C.columns(n2, C.SEED + 1)
            first = {"kw12": a["kw12"], "m": a["rt_s"]}
            second = {"kw12": b["kw12"], "m": b["rt"]}
            one = C.concat_columns([first, second], [n, n2], ["kw12", "m"])
            want = C.run_reference(case, [(one, n + n2)])
            segs = [engine.upload_segment(first, n), engine.upload_segment(second, n2)]
            plan = engine.plan(aggs)
            try:
                for turn in ("first collect", "after reset"):
                    tag = "all-ones n=%d+%d %s %s" % (n, n2, name, turn)
                    with device_errors_end_the_session(lambda: tag):
                        if turn != "first collect":
                            plan.reset()
                        for s in segs:
                            plan.collect(s)
                        _compare(plan.build(), want, tag, True, problems)
            finally:
                plan.close()
                for s in segs:
                    s.close()
    assert not problems, "\n".join(problems[:12])


# ---- many small segments in one plan -----------------------------------------------------------------------------------
def _case(group, name):
    return next(c for c in C.GROUPS[group]() if c.name == name)


def _collect_many(engine, case, uploads, map_fields, first_path=None):
    segs = [engine.upload_segment(c, n) for c, n in uploads]
    maps = [engine.ordinal_map(segs, f) for f in map_fields]
    plan = engine.plan(case.aggs(), filters=case.filters)
    try:
        with device_errors_end_the_session(lambda: "%s over %s docs" % (case.name, [n for _, n in uploads])):
            for k, s in enumerate(segs):
                plan.collect(s)
                if k == 0 and first_path is not None:
                    assert plan.last_collect_stats()[2] == first_path
                if s.max_doc:
                    _seen_paths.add(plan.last_collect_stats()[2])
            return plan.build()
    finally:
        plan.close()
        for m in maps:
            m.close()
        for s in segs:
            s.close()


MANY = {
    # variant: (group, case, keyword fields with per-segment dictionaries, fields under an ordinal map, metric absent)
    "a": ("a", "a_every_term", ("host",), ("host",), False),
    "d": ("d", "d_sparse", ("host_s",), ("host_s",), False),
    "f": ("f", "f0_terms_tags", ("tags0",), ("tags0",), False),
    "h": ("h", "h_status_count_desc", (), ("status",), False),
    "metric_absent_in_the_5_doc_segment": ("a", "a_every_term", ("host",), ("host",), True),
}


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("variant", sorted(MANY))
def test_many_small_segments_in_one_plan(engine, variant, reverse):
    """segments of 1, 8,193, 0, 5, 64, 2,049 and 3 docs collected into one plan, in that order and in reverse, under an
    ordinal map over their differing dictionaries; later segments extend the time range backwards and forwards, so the
    grid grows along the key axis; the expected value is the oracle over the concatenation"""
    group, name, dict_fields, map_fields, absent_metric = MANY[variant]
    case = _case(group, name)
    order = list(range(len(C.MULTI_SIZES)))[::-1 if reverse else 1]
    absent = {(order.index(C.MULTI_SIZES.index(5)), "rt")} if absent_metric else set()
    uploads, (one, total) = C.multi_segments(case, order, dict_fields=dict_fields, absent=absent)
    # the map is built over the uploaded fields only
    uploads = [({f: c for f, c in cols.items() if not f.endswith("_kw")}, n) for cols, n in uploads]
    want = C.run_reference(case, [(one, total)])
    res = _collect_many(engine, case, uploads, map_fields)
    tag = "many %s %s" % (variant, "reversed" if reverse else "in order")
    assert_same(res.to_dict(), want["shards"][0], tag + " shard", case.exact)
    assert_same(reduce([res]).to_dict(), want["reduced"], tag + " reduced", case.exact)


@pytest.mark.parametrize("first", [8193, 5])
def test_ranked_plan_whose_second_segment_holds_one_doc(engine, first):
    """a ranked collect (path 10) of the first segment, then a 1-doc segment with the same dictionary: the retained
    segment is collected again over every term (esgpu_runtime.cpp:4389-4400) and the second one added"""
    case = _case("a", "a_ranked")
    a, b = C.columns(first), C.columns(1, C.SEED + 1)
    b = dict(b, **{"@timestamp": dict(b["@timestamp"], values=b["@timestamp"]["values"] + 3 * C.HOUR)})
    one = C.concat_columns([a, b], [first, 1], list(case.fields))
    want = C.run_reference(case, [(one, first + 1)])
    with layout(engine, "block"):
        uploads = [({f: a[f] for f in case.fields}, first), ({f: b[f] for f in case.fields}, 1)]
        res = _collect_many(engine, case, uploads, (), first_path=10)
    assert_same(res.to_dict(), want["shards"][0], "ranked then one doc (n=%d) shard" % first)
    assert_same(reduce([res]).to_dict(), want["reduced"], "ranked then one doc (n=%d) reduced" % first)


def test_every_collect_path_was_observed():
    """runs after the cases above (file order): every collect path of include/esgpu.h:404-408 was reported at some size
    <= 16,385 -- except 4, partitioned terms counting, which the runtime takes only where the hot/cold statistics refuse a
    column: more than kHcMaxParts = 1,024 partitions of 2^15 ordinals, a dictionary of over 2^25 terms
    (esgpu_runtime.cpp:2143-2144, :3503-3509).  No dictionary of this module (300,000 terms at most) reaches it."""
    assert _seen_paths == set(range(11)) - {4}, "paths seen (the ladder tests of this module run first): %s" % sorted(_seen_paths)
