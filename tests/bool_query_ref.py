"""numpy restatement of the bool query semantics, evaluated on the builder objects themselves (never on the lowered
esgpu_filter array): BoolQueryBuilder.doToQuery, Queries.applyMinimumShouldMatch / fixNegativeQueryIfNeeded and
BooleanQuery's matching rules.

    mask(cols, query, n) -> [n] bool: the docs of the first n the query matches

A query is a leaf (TermQuery, RangeQuery, TermsQuery, ExistsQuery), a list (a conjunction: bool.filter) or a BoolQuery of
any nesting.  A bool matches a doc iff every must / filter clause holds, no must_not clause holds and at least m should
clauses hold; m = calculateMinShouldMatch(S, spec) when a spec is given and that is > 0, else 1 when there is no must /
filter clause and S > 0, else 0.  No clause: match_all.  Only must_not clauses: the docs none holds for when
adjust_pure_negative, else none.  A leaf over a field the columns lack holds for no doc.  term and range leaves are
tests/filters_ref.clause_mask; terms is the union of its values' term leaves (none for an empty list); exists is a set
present bit and an ordinal other than the missing one -- a NaN double is a value.
"""
import numpy as np

import filters_ref as FR
from elasticsearch_amd import _native as N
from elasticsearch_amd.aggs import (BoolQuery, ExistsQuery, TermQuery, TermsQuery, calculate_min_should_match)


def leaf_mask(cols, q, n):
    c = cols.get(q.field)
    if c is None:
        return np.zeros(n, dtype=bool)
    if isinstance(q, ExistsQuery):
        has = np.ones(n, dtype=bool) if c.get("present") is None else FR.mask_from_bits(c["present"], n)
        if c["type"] == N.COL_ORD_U32:
            has = has & (np.asarray(c["values"])[:n] != FR.MISSING_ORD)
        return has
    if isinstance(q, TermsQuery):
        m = np.zeros(n, dtype=bool)
        for v in q.values:
            m |= FR.clause_mask(cols, TermQuery(q.field, v), n)
        return m
    return FR.clause_mask(cols, q, n)


def mask(cols, query, n):
    if isinstance(query, (list, tuple)):
        m = np.ones(n, dtype=bool)
        for c in query:
            m &= mask(cols, c, n)
        return m
    if not isinstance(query, BoolQuery):
        return leaf_mask(cols, query, n)
    required = query.must_clauses + query.filter_clauses
    if not required and not query.should_clauses and not query.must_not_clauses:
        return np.ones(n, dtype=bool)
    if not required and not query.should_clauses and not query._adjust:
        return np.zeros(n, dtype=bool)
    m = np.ones(n, dtype=bool)
    for c in required:
        m &= mask(cols, c, n)
    for c in query.must_not_clauses:
        m &= ~mask(cols, c, n)
    s = len(query.should_clauses)
    need = calculate_min_should_match(s, query._msm) if query._msm is not None else 0
    if need <= 0:
        need = 1 if not required and s > 0 else 0
    held = np.zeros(n, dtype=np.int64)
    for c in query.should_clauses:
        held += mask(cols, c, n)
    return m & (held >= need)
