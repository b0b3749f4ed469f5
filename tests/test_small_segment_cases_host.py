"""The small-segment case tables (tests/small_segment_cases.py) without a GPU: every group builds and runs through the
oracle at every ladder size, and the oracle itself is pinned at these sizes by three-line numpy restatements -- per-term
bincount, fixed-interval keys by floor division, per-bucket int64 sum / min / max / value count, and the number of
distinct values for cardinality while linear counting is exact.  Calendar rounding and HLL estimates are not restated.
"""
import numpy as np
import pytest

import small_segment_cases as C
from small_segment_cases import HOUR, LADDER, MISSING


def _case(group, name):
    return next(c for c in C.GROUPS[group]() if c.name == name)


@pytest.mark.parametrize("group", sorted(C.GROUPS))
def test_every_case_builds_and_runs_through_the_oracle(group):
    for case in C.GROUPS[group]():
        for n in LADDER:
            want = C.reference(case, n)
            assert len(want["shards"]) == 1 and set(want["reduced"]) == {a.name for a in case.aggs()}, (case.name, n)
            cols = case.columns(n)
            assert all(len(cols[f]["values"]) == n for f in case.fields if cols[f].get("offsets") is None), (case.name, n)
            for layout in C.LAYOUTS:
                assert case.path(n, layout, cols) in range(11), (case.name, n, layout)


def test_generators_are_pure_and_the_last_doc_alternates():
    for n in LADDER:
        a = C.columns(n)
        C._cols_cache.pop((n, C.SEED, False))
        b = C.columns(n)
        for f in a:
            assert np.array_equal(a[f]["values"], b[f]["values"]), (f, n)
        for f in ("ts_s", "rt_s"):
            assert C.mask_of(a[f], n)[-1] == (n % 2 == 1), (f, n)
        assert (a["host_s"]["values"][-1] != MISSING) == (n % 2 == 1), n
        assert C.mask_of(a["rt_last"], n).sum() == 1 and C.mask_of(a["rt_none"], n).sum() == 0, n
        assert len(a["tags0"]["offsets"]) == n + 1 and np.diff(a["tags0"]["offsets"].astype(np.int64))[-1] == 0, n
        assert np.diff(a["nums3"]["offsets"].astype(np.int64))[-1] == 3, n
        ts = a["@timestamp"]["values"]
        assert np.all(np.diff(ts) >= 0), n
        assert len(np.unique(ts // HOUR)) == (1 if n == 1 else 2), n
        for r in range(0, n, 2048):  # every run of 2,048 docs spans less than 2^16 ms: the block-delta layout applies
            assert ts[r:r + 2048].max() - ts[r:r + 2048].min() < (1 << 16), (n, r)
        wide = C.columns(n, wide=True)["@timestamp"]["values"]
        assert n == 1 or wide[-1] - wide[0] == 40 * C.DAY - 1, n


def test_predicted_paths_cover_every_form_but_the_partitioned_one():
    """Every collect path of include/esgpu.h:404-408 is expected at some ladder size, except 4 (partitioned terms
    counting): it runs only where the hot/cold statistics refuse a column, from 2^25 terms up (kHcMaxParts partitions of
    2^15 ordinals, esgpu_runtime.cpp:2143-2144) -- no dictionary of 300,000 terms gets there."""
    seen = set()
    for group in C.GROUPS:
        for case in C.GROUPS[group]():
            for n in LADDER:
                cols = case.columns(n)
                seen |= {case.path(n, layout, cols) for layout in C.LAYOUTS}
    assert seen == set(range(11)) - {4}


@pytest.mark.parametrize("field,T", [("kw12", 12), ("host", C.HOST_TERMS)])
def test_terms_counts_are_the_bincount(field, T):
    for n in LADDER:
        counts = np.bincount(C.columns(n)[field]["values"], minlength=T)
        got = C.reference(_case("c", "c_%s_term_asc" % field), n)["reduced"]["t"]["buckets"]
        assert [b["doc_count"] for b in got] == counts[:10].tolist(), n  # min_doc_count 0: the first ten terms, empty or not
        order = np.lexsort((np.arange(T), -counts))[:10]                  # _count desc, ties by term
        got = C.reference(_case("c", "c_%s_count_desc" % field), n)["reduced"]["t"]["buckets"]
        assert [b["doc_count"] for b in got] == counts[order].tolist(), n
        terms = ["k%02d" % i for i in range(12)] if field == "kw12" else ["host-%04d" % i for i in range(T)]
        assert [b["key"] for b in got] == [terms[i] for i in order], n


def test_high_cardinality_counts_are_the_bincount():
    for T in C.HC_TERMS:
        for n in LADDER:
            counts = np.bincount(C.hc_columns(n, T)["kw"]["values"], minlength=T)
            order = np.lexsort((np.arange(T), -counts))[:2]
            got = C.reference(_case("i%d" % T, "i%d_kw_count" % T), n)["reduced"]["t"]["buckets"]
            assert [(b["key"], b["doc_count"]) for b in got] == [("u%07d" % i, int(counts[i])) for i in order if counts[i]], (T, n)
            assert C.reference(_case("i%d" % T, "i%d_kw_none_term" % T), n)["reduced"]["t"]["buckets"] == [], (T, n)


def test_hourly_keys_and_bucket_metrics_are_floor_division_and_int64_sums():
    for n in LADDER:
        cols = C.columns(n)
        ts, rt = cols["@timestamp"]["values"], cols["rt"]["values"]
        keys = ts // HOUR * HOUR
        got = C.reference(_case("b", "b_four_single_values"), n)["reduced"]["d"]["buckets"]
        assert [b["key"] for b in got] == np.unique(keys).tolist(), n
        for b in got:
            v = rt[keys == b["key"]]
            assert (b["doc_count"], b["s"]["value"], b["mn"]["value"], b["mx"]["value"], b["vc"]["value"]) == \
                (len(v), float(v.sum()), float(v.min()), float(v.max()), len(v)), (n, b["key"])
        got = C.reference(_case("b", "b_extended_stats"), n)["reduced"]["d"]["buckets"]
        for b in got:
            v = rt[keys == b["key"]]
            e = b["e"]
            assert (e["count"], e["sum"], e["min"], e["max"], e["sum_of_squares"]) == \
                (len(v), float(v.sum()), float(v.min()), float(v.max()), float((v * v).sum())), (n, b["key"])
        # histogram(interval 50, offset 7) over rt: keys by floor division around the offset
        hk = (rt - 7) // 50 * 50 + 7
        got = C.reference(_case("b", "b_histogram_avg"), n)["reduced"]["h"]["buckets"]
        # (a histogram's min_doc_count defaults to 0: the reduce fills the empty keys between the extremes in)
        assert [b["key"] for b in got] == list(range(int(hk.min()), int(hk.max()) + 1, 50)), n
        assert [(b["key"], b["doc_count"]) for b in got if b["doc_count"]] == [(int(k), int((hk == k).sum())) for k in np.unique(hk)], n
        # sparse: the docs whose timestamp is present, the values whose metric is present
        mt, mr = C.mask_of(cols["ts_s"], n), C.mask_of(cols["rt_s"], n)
        got = C.reference(_case("d", "d_hist_sparse"), n)["reduced"]["d"]["buckets"]
        assert [(b["key"], b["doc_count"]) for b in got] == [(int(k), int((mt & (keys == k)).sum())) for k in np.unique(keys[mt])], n
        for b in got:
            assert b["e"]["count"] == int((mt & mr & (keys == b["key"])).sum()), (n, b["key"])


def test_cardinality_is_the_distinct_count_while_linear_counting_is_exact():
    for n in LADDER:
        cols = C.columns(n)
        for field in ("h", "rt", "host"):
            distinct = len(np.unique(cols[field]["values"]))
            got = C.reference(_case("g", "g_root_%s_40000" % field), n)["reduced"]["c"]["value"]
            # linear counting over m = 2^25 encoded hashes estimates m ln(m / (m - d)) = d + d^2 / 2m + ...: it rounds to
            # d while d^2 / 2m < 1 / 2, d < 5,792 -- asserted to 4,096 (an excess of 0.25); above, within that excess
            if distinct <= 4096:
                assert got == distinct, (field, n)
            else:
                assert distinct <= got <= distinct + distinct * distinct // (1 << 26) + 1, (field, n)
            if distinct <= 100:
                assert C.reference(_case("g", "g_root_%s_100" % field), n)["reduced"]["c"]["value"] == distinct, (field, n)


def test_long_terms_twins_are_the_unique_counts():
    for n in LADDER:
        for field in ("status", "ids", "@timestamp"):
            keys, counts = np.unique(C.columns(n)[field]["values"], return_counts=True)
            got = C.reference(_case("h", "h_%s_term_asc" % field.strip("@")), n)["reduced"]["t"]["buckets"]
            assert [(b["key"], b["doc_count"]) for b in got] == list(zip(keys[:7].tolist(), counts[:7].tolist())), (field, n)


def test_many_small_segments_concatenate():
    """the multi-segment construction: per-segment dictionaries differ, their docs map onto one union dictionary, the
    key range grows both ways, and the oracle runs over the concatenation in both collect orders"""
    case = _case("a", "a_every_term")
    for order in (list(range(len(C.MULTI_SIZES))), list(range(len(C.MULTI_SIZES)))[::-1]):
        uploads, (one, total) = C.multi_segments(case, order, dict_fields=("host",))
        assert total == sum(C.MULTI_SIZES) and [n for _, n in uploads] == [C.MULTI_SIZES[k] for k in order]
        dicts = [tuple(c["host"]["terms"]) for c, _ in uploads]
        assert len(set(dicts)) > 1
        # every doc names the same term through its segment's dictionary and through the union
        at = 0
        for c, n in uploads:
            local = [c["host"]["terms"][o] for o in c["host"]["values"]]
            assert local == [one["host"]["terms"][o] for o in one["host"]["values"][at:at + n]]
            at += n
        assert len(np.unique(one["@timestamp"]["values"] // HOUR)) >= 6
        want = C.run_reference(case, [(one, total)])
        assert sum(b["doc_count"] for b in want["reduced"]["hosts"]["buckets"]) > 0
