"""Bool queries on the CPU: the builders' lowering into esgpu_filter (leaves, occurs, groups, the owner's options record),
plain requests lowering to exactly the array they lowered to before, the nesting errors, minimum_should_match worked out by
hand from Queries.calculateMinShouldMatch (common/lucene/search/Queries.java:142-177), the numpy reference on a hand-written
truth table, and esgpu_plan_create's refusals (validation only: no device call is reached).
"""
import ctypes

import numpy as np
import pytest

import bool_query_ref as BR
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import _native as N
from elasticsearch_amd.aggs import calculate_min_should_match as msm
from elasticsearch_amd.aggs import flatten, flatten_filters
from helpers import bits_from_mask

MUST, SHOULD, NOT = N.OCCUR_MUST, N.OCCUR_SHOULD, N.OCCUR_MUST_NOT


def rows(queries, aggs=None, lookup=None):
    flt, n, _keep = flatten_filters(queries, lookup, aggs)
    return [(flt[k].owner, flt[k].type, flt[k].field, flt[k].occur, flt[k].group) for k in range(n)], flt


# ---- lowering ----------------------------------------------------------------------------------------------------------
def test_constants_and_struct_tail():
    assert (N.FILTER_TERMS, N.FILTER_EXISTS, N.FILTER_BOOL) == (3, 4, 5) and (MUST, SHOULD, NOT) == (0, 1, 2)
    names = [f[0] for f in N.Filter._fields_]
    assert names[-6:] == ["slot", "reserved_slot", "occur", "group", "terms", "n_terms"]
    z = N.Filter()
    assert (z.occur, z.group, z.n_terms) == (0, 0, 0) and not z.terms   # zero-initialised: a plain MUST clause
    assert N.lib().esgpu_abi_version() == 7


def test_plain_requests_lower_to_the_same_array_as_before():
    plain = [QB.termQuery("status", 200), QB.rangeQuery("bytes").gte(1024).lt(65536)]
    want, flt = rows(plain)
    assert want == [(0, N.FILTER_TERM, b"status", 0, 0), (0, N.FILTER_RANGE, b"bytes", 0, 0)]
    assert (flt[1].has_lower, flt[1].include_lower, flt[1].lo_i, flt[1].has_upper, flt[1].include_upper, flt[1].hi_i) == (1, 1, 1024, 1, 0, 65536)
    # the same conjunction as a bool of filter / must clauses, nested or not, with options that change nothing
    for q in (QB.boolQuery().filter(plain[0]).must(plain[1]), QB.boolQuery().must(plain[0]).filter(QB.boolQuery().filter(plain[1])),
              [plain[0], QB.boolQuery().must(plain[1])], QB.boolQuery().filter(plain).adjustPureNegative(False).minimumShouldMatch(1)):
        got, _f = rows(q)
        assert sorted(got) == sorted(want), got
    assert rows(None)[0] == [] and rows([])[0] == [] and rows(QB.boolQuery())[0] == []   # no query clause, as before
    assert rows(plain[0])[0] == want[:1]
    aggs = [AB.filter("f", plain), AB.filters("g").filter("a", plain[0]).filter("all", [])]
    assert rows(None, aggs)[0] == [(1, N.FILTER_TERM, b"status", 0, 0), (1, N.FILTER_RANGE, b"bytes", 0, 0), (2, N.FILTER_TERM, b"status", 0, 0)]


def test_each_builder_form():
    q = (QB.boolQuery().must(QB.rangeQuery("rt").gte(5)).filter(QB.termQuery("status", 200)).mustNot(QB.termQuery("status", 404))
         .should(QB.existsQuery("price")).should(QB.termsQuery("bytes", [3, 1, 2])).minimumShouldMatch("2"))
    got, flt = rows(q)
    assert got == [(0, N.FILTER_RANGE, b"rt", MUST, 0), (0, N.FILTER_TERM, b"status", MUST, 0), (0, N.FILTER_EXISTS, b"price", SHOULD, 0),
                   (0, N.FILTER_TERMS, b"bytes", SHOULD, 0), (0, N.FILTER_TERM, b"status", NOT, 0), (0, N.FILTER_BOOL, None, 0, 0)]
    assert flt[3].n_terms == 3 and [flt[3].terms[k] for k in range(3)] == [3, 1, 2]
    assert (flt[5].term, flt[5].include_lower) == (2, 1)               # the resolved minimum_should_match, adjust_pure_negative
    got, flt = rows(QB.missingQuery("price"))
    assert got == [(0, N.FILTER_EXISTS, b"price", NOT, 0), (0, N.FILTER_BOOL, None, 0, 0)] and (flt[1].term, flt[1].include_lower) == (-1, 1)
    got, flt = rows(QB.boolQuery().mustNot(QB.termQuery("a", 1)).adjustPureNegative(False))
    assert (flt[1].type, flt[1].term, flt[1].include_lower) == (N.FILTER_BOOL, -1, 0)
    got, flt = rows(QB.termsQuery("kw", ["b", "zz", "a"]), lookup=lambda f, t: {"a": 0, "b": 1}.get(t, -1))
    assert got[0][:4] == (0, N.FILTER_TERMS, b"kw", MUST) and [flt[0].terms[k] for k in range(3)] == [1, -1, 0]
    got, flt = rows(QB.termsQuery("v", []))
    assert got == [(0, N.FILTER_TERMS, b"v", MUST, 0), (0, N.FILTER_BOOL, None, 0, 0)] and flt[0].n_terms == 0
    # snake_case aliases
    s = QB.bool_query().must_not(QB.exists_query("a")).should(QB.terms_query("b", [1])).minimum_should_match("1").adjust_pure_negative(True)
    assert rows(s)[0] == rows(QB.boolQuery().mustNot(QB.existsQuery("a")).should(QB.termsQuery("b", [1])).minimumShouldMatch("1"))[0]
    assert rows(QB.missing_query("a"))[0] == rows(QB.missingQuery("a"))[0]


def test_groups_and_owners():
    grp = lambda: QB.boolQuery().should(QB.termQuery("a", 1)).should(QB.existsQuery("b"))  # noqa: E731
    q = QB.boolQuery().must(grp()).should(grp()).should(QB.termQuery("c", 3)).mustNot(grp().minimumShouldMatch(1))
    got, flt = rows(q, [AB.filter("f", QB.boolQuery().should(QB.existsQuery("x"))), AB.filter("e", QB.boolQuery())])
    assert got == [(0, N.FILTER_TERM, b"a", MUST, 1), (0, N.FILTER_EXISTS, b"b", MUST, 1),
                   (0, N.FILTER_TERM, b"a", SHOULD, 2), (0, N.FILTER_EXISTS, b"b", SHOULD, 2), (0, N.FILTER_TERM, b"c", SHOULD, 0),
                   (0, N.FILTER_TERM, b"a", NOT, 3), (0, N.FILTER_EXISTS, b"b", NOT, 3), (0, N.FILTER_BOOL, None, 0, 0),
                   (1, N.FILTER_EXISTS, b"x", SHOULD, 0), (1, N.FILTER_BOOL, None, 0, 0),
                   (2, N.FILTER_BOOL, None, 0, 0)]                      # an empty bool in a filter aggregation: match_all
    assert flt[7].term == -1


def test_nesting_errors():
    leaf = QB.termQuery("a", 1)
    conj = QB.boolQuery().must(leaf).must(QB.existsQuery("b"))
    bad = [QB.boolQuery().should(conj), QB.boolQuery().mustNot(conj), QB.boolQuery().should([leaf, leaf]),
           QB.boolQuery().must(QB.boolQuery().should(QB.boolQuery().should(leaf))),                     # deeper nesting
           QB.boolQuery().should(QB.boolQuery().should(leaf).should(leaf).minimumShouldMatch(2)),       # msm >= 2 on a nested bool
           QB.boolQuery().must(QB.boolQuery().mustNot(leaf)), QB.boolQuery().must(QB.boolQuery().must(leaf).should(leaf)),
           QB.boolQuery().must(QB.boolQuery())]
    for q in bad:
        with pytest.raises(N.UnsupportedOnGpu) as e:
            flatten_filters(q)
        assert "bool nesting runs on the CPU path" in str(e.value)


# ---- minimum_should_match by hand --------------------------------------------------------------------------------------
def test_minimum_should_match_kats():
    assert msm(5, "-25%") == 4                  # 5 * -25 * 0.01f = -1.25 -> (int) -1 -> 5 - 1
    assert msm(3, "3<90%") == 3                 # 3 <= 3: every clause
    assert msm(4, "3<90%") == 3                 # 4 * 90 * 0.01f = 3.6 -> 3
    assert msm(2, "5") == 2 and msm(0, "1") == 0  # capped at the optional clauses
    assert msm(3, "-7") == 0 and msm(1, "-100%") == 0  # negative results give 0
    assert msm(5, "2") == 2 and msm(5, "-1") == 4 and msm(4, "75%") == 3 and msm(3, "75%") == 2  # 2.25 -> 2
    assert msm(10, "2<-25% 9<-3") == 7 and msm(5, "2<-25% 9<-3") == 4 and msm(2, "2<-25% 9<-3") == 2
    assert msm(7, " 3 < 50% ") == 3
    assert msm(100, "29%") == 29                # 2900 * 0.01f is 28.9999993... exactly and rounds to 29.0 in float32
    for bad in ("x", "50%%", "2<"):
        with pytest.raises((ValueError, IndexError)):
            msm(3, bad)


# ---- the numpy reference on a hand-written truth table -----------------------------------------------------------------
def test_reference_truth_table():
    nan = float("nan")
    cols = {"a": {"type": N.COL_I64, "values": np.array([1, 1, 2, 2, 1, 1, 2, 2], np.int64)},
            "b": {"type": N.COL_I64, "values": np.array([5, 6, 5, 6, 5, 6, 5, 6], np.int64),
                  "present": bits_from_mask(np.array([1, 1, 1, 1, 0, 0, 1, 1], bool))},
            "d": {"type": N.COL_F64, "values": np.array([0.0, -0.0, nan, 1.0, nan, 2.0, 3.0, 0.0]),
                  "present": bits_from_mask(np.array([1, 1, 1, 1, 0, 1, 1, 1], bool))},
            "k": {"type": N.COL_ORD_U32, "values": np.array([0, 1, 0xFFFFFFFF, 1, 0, 0xFFFFFFFF, 1, 0], np.uint32), "terms": ["x", "y"]}}
    a1, b5, kx = QB.termQuery("a", 1), QB.termQuery("b", 5), QB.termQuery("k", "x")
    T = lambda q: [int(v) for v in BR.mask(cols, q, 8)]  # noqa: E731
    assert T(a1) == [1, 1, 0, 0, 1, 1, 0, 0] and T(b5) == [1, 0, 1, 0, 0, 0, 1, 0] and T(kx) == [1, 0, 0, 0, 1, 0, 0, 1]
    assert T(QB.existsQuery("b")) == [1, 1, 1, 1, 0, 0, 1, 1] and T(QB.existsQuery("k")) == [1, 1, 0, 1, 1, 0, 1, 1]
    assert T(QB.existsQuery("d")) == [1, 1, 1, 1, 0, 1, 1, 1]                       # the NaN of doc 2 is a value
    assert T(QB.missingQuery("d")) == [0, 0, 0, 0, 1, 0, 0, 0]
    assert T(QB.termsQuery("d", [0, 3])) == [1, 1, 0, 0, 0, 0, 1, 1] and T(QB.termsQuery("a", [])) == [0] * 8
    assert T(QB.existsQuery("nowhere")) == [0] * 8 and T(QB.boolQuery().mustNot(QB.existsQuery("nowhere"))) == [1] * 8
    assert T(QB.boolQuery()) == [1] * 8
    assert T(QB.boolQuery().mustNot(a1)) == [0, 0, 1, 1, 0, 0, 1, 1] and T(QB.boolQuery().mustNot(a1).adjustPureNegative(False)) == [0] * 8
    assert T(QB.boolQuery().should(a1).should(b5)) == [1, 1, 1, 0, 1, 1, 1, 0]       # should-only: at least one
    assert T(QB.boolQuery().must(a1).should(b5)) == [1, 1, 0, 0, 1, 1, 0, 0]         # beside must: optional
    assert T(QB.boolQuery().must(a1).should(b5).minimumShouldMatch(1)) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert T(QB.boolQuery().should(a1).should(b5).should(kx).minimumShouldMatch(2)) == [1, 0, 0, 0, 1, 0, 0, 0]
    assert T(QB.boolQuery().should(a1).should(b5).should(kx).minimumShouldMatch("-34%")) == [1, 0, 0, 0, 1, 0, 0, 0]  # 3 - 1
    grp = QB.boolQuery().should(b5).should(kx)
    assert T(QB.boolQuery().must(grp)) == [1, 0, 1, 0, 1, 0, 1, 1] and T(QB.boolQuery().mustNot(grp)) == [0, 1, 0, 1, 0, 1, 0, 0]
    assert T([a1, QB.boolQuery().mustNot(b5)]) == [0, 1, 0, 0, 1, 1, 0, 0]


# ---- esgpu_plan_create (validation only: the checks throw before any use of the context) -----------------------------------
def _create_raw(specs, n, flt, nf):
    ctx = ctypes.create_string_buffer(1 << 16)
    plan = ctypes.c_void_p()
    lib = N.lib()
    rc = lib.esgpu_plan_create(ctypes.cast(ctx, ctypes.c_void_p), specs, n, flt, nf, ctypes.byref(plan))
    buf = ctypes.create_string_buffer(1024)
    lib.esgpu_last_error(buf, 1024)
    return rc, buf.value.decode()


def _create(aggs, filters=None):
    specs, n, _keep = flatten(aggs)
    flt, nf, _fk = flatten_filters(filters, None, aggs)
    return _create_raw(specs, n, flt, nf)


def test_plan_create_refusals():
    neg = lambda: QB.boolQuery().mustNot(QB.termQuery("status", 404))  # noqa: E731
    for aggs in ([AB.filters("f").filter("a", neg())], [AB.filters("f").filter("a", [QB.termQuery("status", 1), QB.existsQuery("b")])],
                 [AB.terms("t").field("host").subAggregation(AB.filter("f", neg()))],
                 [AB.filter("p", QB.termQuery("status", 200)).subAggregation(AB.filter("f", QB.existsQuery("bytes")))]):
        rc, msg = _create(aggs)
        assert rc == N.ERR_UNSUPPORTED and "bool query" in msg, msg
    specs, n, _keep = flatten([AB.stats("s").field("bytes")])
    grp = QB.boolQuery().should(QB.boolQuery().should(QB.termQuery("a", 1)).should(QB.termQuery("b", 2)))
    flt, nf, _fk = flatten_filters(grp)
    flt[1].occur = N.OCCUR_MUST_NOT                                         # a group whose leaves disagree on occur
    assert _create_raw(specs, n, flt, nf)[0] == N.ERR_INVALID
    flt, nf, _fk = flatten_filters(QB.boolQuery().mustNot(QB.termQuery("a", 1)))
    two = (N.Filter * 3)(flt[0], flt[1], flt[1])                             # two option records for one owner
    assert _create_raw(specs, n, two, 3)[0] == N.ERR_INVALID
    flt, nf, _fk = flatten_filters(QB.termsQuery("a", [1, 2]))
    flt[0].terms = None                                                       # values announced, none given
    assert _create_raw(specs, n, flt, nf)[0] == N.ERR_INVALID
    flt, nf, _fk = flatten_filters(QB.existsQuery("a"))
    flt[0].occur = 3
    assert _create_raw(specs, n, flt, nf)[0] == N.ERR_INVALID
