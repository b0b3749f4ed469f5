"""GPU parity of the selection routines on crafted count vectors (tests/topk_ref.py): every branch of launch_topk,
launch_topk_candidates, row_topk_kernel, colo_select_kernel and the two hot/cold gates, exactly.

Random Zipf or uniform counts do not put two counts of one histogram sub-bin at the k-th position, a tie at the cut over
more candidates than one 4096-key chunk, a winner into load_counts4's scalar tail, two tied ordinals into one lane's
share of a row, or a hot slot's count exactly onto max_cold.  Each case here does, and that it does is arithmetic on its
input, asserted by tests/test_topk_cases_host.py (the build has no counter for it).  Every request's buckets are compared
with the numpy selection exactly -- term, doc_count, order, sum_other_doc_count -- and the whole result with the oracle.
The collect path is asserted where a case depends on it (8 / 9: the deferred cold lists; a metric child: 64-bit counts);
the build-side gate is restated from the request: value_count > 65,536 and min(size, value_count) <= 1024 select on the
device, anything else on the host.

A segment is uploaded once per module and shared by its requests.
"""
import functools

import numpy as np
import pytest

import long_terms_stream as LT
import oracle as O
import topk_ref as R
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import build_reduce, colocated, reduce
from helpers import assert_same, bits_from_mask
from test_gpu_small_segments import device_errors_end_the_session

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uploaded(engine):
    """key, builder of (columns, docs) -> the segment, uploaded once"""
    cache = {}

    def get(key, build):
        if key not in cache:
            cols, n = build()
            cache[key] = engine.upload_segment(cols, n)
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


def _terms(req, name, shard_size=None):
    order, size, mdc, smdc = req
    return (AB.terms(name).field("kw").size(size).shardSize(size if shard_size is None else shard_size).order(order)
            .minDocCount(mdc).shardMinDocCount(smdc))


def _assert_buckets(got, picks, counts, other, tag):
    assert got["sum_other_doc_count"] == other, "%s: other %d, expected %d" % (tag, got["sum_other_doc_count"], other)
    have = [(b["key"], b["doc_count"]) for b in got["buckets"]]
    want = [("u%07d" % o, int(c)) for o, c in zip(picks, counts)]
    if have != want:
        i = next((i for i, (h, w) in enumerate(zip(have, want)) if h != w), min(len(have), len(want)))
        raise AssertionError("%s: %d buckets, expected %d; the first difference at %d: got %s, expected %s"
                             % (tag, len(have), len(want), i, have[i:i + 1], want[i:i + 1]))


# ---- a - e: the top-level selection ----------------------------------------------------------------------------------
def _case_aggs(case, i):
    t = _terms(case["requests"][i], "r%d" % i)
    if case["mode"] == "stats":
        return [t.subAggregation(AB.stats("s").field("v"))]
    if case["mode"] == "beside":
        return [t, AB.terms("z").field("kw").size(2).shardSize(2).order(R.TERM_ASC)]
    return [t]


@functools.lru_cache(maxsize=4)
def _case_oracle(name):
    """the oracle's results of all of a case's requests, from one run"""
    case = R.CASES[name]
    cols, n, mask = R.segment(case["vector"], case["T"])
    aggs = [_case_aggs(case, i)[0] for i in range(len(case["requests"]))]
    aggs.append(AB.terms("z").field("kw").size(2).shardSize(2).order(R.TERM_ASC))
    return O.run([(cols, n)], aggs, accept=[bits_from_mask(mask)] if mask is not None else None)


def _run_case(engine, uploaded, name):
    case = R.CASES[name]
    T, mode = case["T"], case["mode"]
    cols, n, mask = R.segment(case["vector"], T)
    counts = R.vector(case["vector"], T)
    seg = uploaded((case["vector"], T), lambda: (cols, n))
    accept = bits_from_mask(mask) if mode == "accept" else None
    assert (mask is not None) == (mode == "accept")
    want = _case_oracle(name)
    results = {}
    for i, req in enumerate(case["requests"]):
        order, size, mdc, smdc = req
        tag = "%s (%s) %s size %d min_doc_count %d shard_min_doc_count %d" % (name, case["branch"], R.ORDER_NAMES[order],
                                                                             size, mdc, smdc)
        # build_terms_root's gate, restated: this request's selection runs on the device, or (1025) on the host
        assert (T > R.GPU_TOPK_ABOVE and min(size, T) <= R.TOPK_MAX) == (size != 1025), tag
        key = "r%d" % i
        with device_errors_end_the_session(lambda: tag):
            plan = engine.plan(_case_aggs(case, i))
            try:
                plan.collect(seg, accept_bits=accept)
                path = plan.last_collect_stats()[2]
                if mode == "lone":
                    assert path == 8, "%s: collect path %d, expected the deferred cold lists (8)" % (tag, path)
                elif mode == "accept":
                    assert path == 9, "%s: collect path %d, expected the filtered deferral (9)" % (tag, path)
                elif mode == "stats":
                    assert path not in (4, 6, 7, 8, 9), "%s: collect path %d counts into u32" % (tag, path)
                else:
                    assert path not in (8, 9), "%s: collect path %d defers the cold lists" % (tag, path)
                res = plan.build()
                got = res.to_dict()
                red = reduce([res]).to_dict()
            finally:
                plan.close()
        picks, pc, other = R.select(counts, order, size, mdc, smdc)
        _assert_buckets(got[key], picks, pc, other, tag)
        assert_same(got[key], want["shards"][0][key], tag + " shard")
        assert_same(red[key], want["reduced"][key], tag + " reduced")
        if mode == "beside":
            assert_same(got["z"], want["shards"][0]["z"], tag + " second aggregation")
        results[size] = got[key]["buckets"]
    return results


@pytest.mark.parametrize("name", R.case_names("a"))
def test_count_desc(engine, uploaded, name):
    """launch_topk, count desc: all equal (17 chunks of candidates), two counts in one sub-bin at every cut, the octave
    seams, a 5-way tie at the cut across chunk seams, fewer eligible ordinals than size, shard_min_doc_count, the winner
    at T - 1 for T % 4 = 1, 3, 0, and sizes 1023 / 1024 / 1025 across the host gate"""
    got = _run_case(engine, uploaded, name)
    if name == "a_gate_1024":
        assert got[1025][:1024] == got[1024] and got[1024][:1023] == got[1023]


@pytest.mark.parametrize("name", R.case_names("b"))
def test_count_asc(engine, uploaded, name):
    """the reversed histogram: a tie on count 1 over > 60,000 ordinals, zeros first under min_doc_count 0, the sub-bin
    and octave cuts from the small end"""
    got = _run_case(engine, uploaded, name)
    if name == "b_gate_1024":
        assert got[1025][:1024] == got[1024] and got[1024][:1023] == got[1023]


@pytest.mark.parametrize("name", R.case_names("c"))
def test_term_orders(engine, uploaded, name):
    """topk_kernel<true> per workgroup, then the merge: one eligible ordinal per workgroup, all inside one workgroup,
    k = 1, 16, 17, 1000, 1024, min_doc_count 0 and shard_min_doc_count 2"""
    _run_case(engine, uploaded, name)


@pytest.mark.parametrize("name", R.case_names("d"))
def test_64_bit_counts(engine, uploaded, name):
    """the same vectors with a stats child on a long field: the collect counts into u64 and the top-k reads 8 bytes per
    ordinal"""
    _run_case(engine, uploaded, name)


@pytest.mark.parametrize("name", R.case_names("e"))
def test_deferred_hot_cold_gates(engine, uploaded, name):
    """hot_topk_check_kernel: settled (the k-th hot count one above max_cold), not settled (equal to it), and under
    accept bits a cold ordinal that wins the tie at max_cold"""
    _run_case(engine, uploaded, name)


# ---- f: rows ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _rows_oracle(T):
    cols, n = R.row_segment(T)
    h = AB.dateHistogram("h").field("@timestamp").interval("1h")
    for i, r in enumerate(R.row_requests(T)):
        h.subAggregation(_terms(r, "r%d" % i))
    return O.run([(cols, n)], [h])


@pytest.mark.parametrize("T", R.ROW_T)
def test_rows_under_a_date_histogram(engine, uploaded, T):
    """row_topk_kernel<LROW>: 3 hour rows (ties between t and t + 64, all equal, all zero) over T = 5, 64, 65, 4096 (keys
    in LDS) and 4097 (re-read from memory), both count orders, shard_size 1, 3, T, 1024 and -- on the host -- 1025, 4096 and 4097"""
    seg = uploaded(("rows", T), lambda: R.row_segment(T))
    want = _rows_oracle(T)
    m = R.row_matrix(T)
    prefix = {}
    for i, req in enumerate(R.row_requests(T)):
        order, size, mdc, smdc = req
        key = "r%d" % i
        tag = "T %d %s shard_size %d min_doc_count %d shard_min_doc_count %d" % (T, R.ORDER_NAMES[order], size, mdc, smdc)
        # build_hist's gate, restated: up to 1024 picks per row on the device, beyond (1025, T = 4096 and 4097) on the host
        assert (min(size, T) <= R.ROW_TOPK_MAX) == (size <= 1024), tag
        with device_errors_end_the_session(lambda: tag):
            plan = engine.plan([AB.dateHistogram("h").field("@timestamp").interval("1h").subAggregation(_terms(req, key))])
            try:
                plan.collect(seg)
                res = plan.build()
                got, red = res.to_dict(), reduce([res]).to_dict()
            finally:
                plan.close()
        rows = got["h"]["buckets"]
        assert [b["key"] for b in rows] == [R.T0 + r * R.HOUR for r in range(3)], tag
        for r, b in enumerate(rows):
            assert b["doc_count"] == int(m[r].sum()) + R.ROW_MISSING[r], tag
            picks, pc, other = R.select(m[r], order, size, mdc, smdc)
            _assert_buckets(b[key], picks, pc, other, "%s row %d" % (tag, r))
            assert_same(b[key], want["shards"][0]["h"]["buckets"][r][key], "%s row %d shard" % (tag, r))
            assert_same(red["h"]["buckets"][r][key], want["reduced"]["h"]["buckets"][r][key], "%s row %d reduced" % (tag, r))
        if mdc == 1 and smdc == 0:
            prefix[(order, size)] = [b[key]["buckets"] for b in rows]
    if T == 4097:
        for order in (R.COUNT_DESC, R.COUNT_ASC):
            for r in range(3):
                assert prefix[(order, 1025)][r][:1024] == prefix[(order, 1024)][r], (order, r)


# ---- g: breadth-first replay rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [R.COUNT_DESC, R.COUNT_ASC])
@pytest.mark.parametrize("shard_size", [10, 1500])
def test_replayed_inner_rows(engine, uploaded, monkeypatch, order, shard_size):
    """3 outer terms x 65,537 inner terms, replayed (ESGPU_DEFER_CELLS): the outer terms' inner vectors are all-equal, the
    shared sub-bin and the tie at the cut; inner shard_size 10 (launch_topk per row; count desc may settle from the hot
    slots, replay_hot) and 1,500 (launch_topk_candidates and the host sort)"""
    monkeypatch.setenv("ESGPU_DEFER_CELLS", "1000")
    cols, n = R.replay_segment()
    seg = uploaded(("replay",), lambda: (cols, n))
    m = R.replay_matrix()
    assert (shard_size <= R.TOPK_MAX) == (shard_size == 10) and m.shape[1] > R.GPU_TOPK_ABOVE
    inner = _terms(R.req(order, shard_size), "B")
    aggs = [AB.terms("A").field("a").size(3).shardSize(3).subAggregation(inner)]
    want = O.run([(cols, n)], aggs)
    tag = "replay %s shard_size %d" % (R.ORDER_NAMES[order], shard_size)
    with device_errors_end_the_session(lambda: tag):
        plan = engine.plan(aggs)
        try:
            plan.collect(seg)
            assert plan.deferred_segments() == 1, tag
            res = plan.build()
            got, red = res.to_dict(), reduce([res]).to_dict()
        finally:
            plan.close()
    totals = m.sum(axis=1) + np.array([50, 0, 3])
    outer = sorted(range(3), key=lambda r: (-int(totals[r]), r))
    assert [b["key"] for b in got["A"]["buckets"]] == ["a%04d" % r for r in outer], tag
    for b, r in zip(got["A"]["buckets"], outer):
        assert b["doc_count"] == int(totals[r]), tag
        picks, pc, other = R.select(m[r], order, shard_size)
        _assert_buckets(b["B"], picks, pc, other, "%s outer %s (%s)" % (tag, b["key"], R.REPLAY_VECTORS[r]))
    assert_same(got, want["shards"][0], tag + " shard")
    assert_same(red, want["reduced"], tag + " reduced")


# ---- h: the co-located reduce's selection ----------------------------------------------------------------------------
@pytest.mark.parametrize("V", R.COLO_V)
def test_colocated_selection(engine, uploaded, V):
    """colo_select_kernel: terms{date_histogram{stats}} over two shards' plans, value_count 1, 2, 3, 4095, 4096 (the
    bitonic sort over the next power of two) and 4097 (host selection), every order, zeros, ties at the cut and
    shard_min_doc_count; the reduced terms against the reference reduce of the two numpy selections and the oracle"""
    shards = R.colo_segments(V)
    segs = [uploaded(("colo", V, s), lambda s=s: shards[s]) for s in range(2)]
    vec = [2 * c for c in R.colo_vectors(V)]  # each vector's docs twice: two hours
    for order, size, shard_size, mdc, smdc in R.colo_requests(V):
        tag = "V %d %s size %d shard_size %d min_doc_count %d shard_min_doc_count %d" % (V, R.ORDER_NAMES[order], size,
                                                                                       shard_size, mdc, smdc)
        aggs = [_terms((order, size, mdc, smdc), "t", shard_size).subAggregation(
            AB.dateHistogram("h").field("@timestamp").interval("1h").subAggregation(AB.stats("s").field("v")))]
        want = O.run(shards, aggs, number_of_shards=2)
        with device_errors_end_the_session(lambda: tag):
            plans = [engine.plan(aggs, number_of_shards=2) for _ in segs]
            try:
                assert colocated(plans), tag
                for p, s in zip(plans, segs):
                    p.collect(s)
                fused = build_reduce(plans).to_dict()
                for p, s in zip(plans, segs):
                    p.reset()
                    p.collect(s)
                plain = reduce([p.build() for p in plans]).to_dict()
            finally:
                for p in plans:
                    p.close()
        per_shard = []
        for c in vec:
            picks, pc, other = R.select(c, order, min(shard_size, V), mdc, smdc)
            per_shard.append(([(int(o), int(k)) for o, k in zip(picks, pc)], other))
        buckets, _, other = LT.reduce_terms(per_shard, size, shard_size, order, min_doc_count=mdc)
        _assert_buckets(fused["t"], [b[0] for b in buckets], [b[1] for b in buckets], other, tag)
        assert_same(fused, want["reduced"], tag + " fused vs oracle")
        assert_same(fused, plain, tag + " fused vs builds")
