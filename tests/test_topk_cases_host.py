"""The crafted selection cases (tests/topk_ref.py) without a GPU.

Three things are settled here, before tests/test_gpu_topk_crafted.py trusts the cases on the GPU: the constants and gates
the case table restates are the ones in the sources (a retuned constant fails here instead of silently moving a case off
its branch); the numpy selection and the oracle agree on every case (keys, counts, sum_other_doc_count), and with the row
loop of long_terms_stream.top_k on the small ones; and every case's stated precondition holds by arithmetic on its input
-- the build exposes no counter for "the threshold bin held more than one chunk".
"""
import os
import re

import numpy as np
import pytest

import long_terms_stream as LT
import oracle as O
import topk_ref as R
from elasticsearch_amd import _native as N

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "elasticsearch_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr (?:uint32_t|int) %s = (\d+);" % name, text)
    assert m, name
    return int(m.group(1))


def test_restated_constants_and_gates_are_the_sources():
    hpp, hip, rt = _src("esgpu_kernels.hpp"), _src("esgpu_kernels.hip"), _src("esgpu_runtime.cpp")
    assert _const(hpp, "kTopkMax") == R.TOPK_MAX
    assert _const(hpp, "kRowTopkMax") == R.ROW_TOPK_MAX
    assert _const(hip, "kRowTopkLdsKeys") == R.ROW_LDS_KEYS
    assert _const(hip, "kTopkChunk") == R.TOPK_CHUNK
    assert _const(hip, "kTopkBins") == R.TOPK_BINS
    assert _const(hpp, "kColoSelMax") == R.COLO_SEL_MAX
    assert int(re.search(r"^#define ESGPU_HOT_MAX (\d+)\b", rt, re.M).group(1)) == R.HOT_MAX
    assert (N.COL_ORD_U32, N.COL_I64) == (R.COL_ORD_U32, R.COL_I64)
    assert (N.ORDER_COUNT_DESC, N.ORDER_COUNT_ASC, N.ORDER_TERM_ASC, N.ORDER_TERM_DESC) == (0, 1, 2, 3)
    # build_terms_root's gate, replay_child's, the rows', the co-located selection's and the deferral's, as text
    assert ("const bool gpu_topk = !agg_order && P0.value_count > %d && k_req <= kTopkMax && (P0.H == 1 || count_order) &&"
            % R.GPU_TOPK_ABOVE) in rt
    assert "B0.value_count2 <= %d" % R.GPU_TOPK_ABOVE in rt
    assert "count_order && B0.value_count == B0.T && S > 0 &&\n            S <= kRowTopkMax) {" in rt
    assert "if (T <= kRowTopkLdsKeys)" in hip
    assert "r.dev = r.dev && P0.value_count <= kColoSelMax && p->docs_seen < (1ull << 31);" in rt
    assert "(uint64_t)tn.s.shard_size <= std::min<uint64_t>(hs.hot_n, kTopkMax) && pl.value_count > %d && pl.H == 1 &&" \
        % R.GPU_TOPK_ABOVE in rt
    assert "K.n_wg = std::min<uint32_t>(512, (K.T + 4095) / 4096);" in rt
    assert "const uint32_t per1 = (uint32_t)(((uint64_t)p.T + p.n_wg - 1) / p.n_wg);" in hip
    assert "ok = order == 0 && k_req >= 1 && last != 0 && ((last >> 32) & 0x7FFFFFFFull) > max_cold;" in _src("esgpu_hotcold.hip")
    # count_bin's body, as text
    body = """    uint32_t b;
    if (c < 32) {
        b = (uint32_t)c;
    } else {
        const uint32_t e = 63u - (uint32_t)__clzll((long long)c);  // >= 5
        b = (e - 4) * 32 + (uint32_t)((c >> (e - 5)) & 31u);       // 32 sub-bins per octave, >= 32
    }
    b = min(b, kTopkBins - 1);
    return order == 0 ? b : kTopkBins - 1 - b;  // COUNT_ASC: fewer docs = better
"""
    assert body in hip
    # and as numbers: monotone, exact below 32, 32 sub-bins per octave
    bins = [R.count_bin(0, c) for c in range(0, 5000)]
    assert bins == sorted(bins) and bins[:33] == list(range(33)) and R.count_bin(0, 63) == 63 and R.count_bin(0, 64) == 64
    assert R.count_bin(0, 1007) == R.count_bin(0, 992) == R.count_bin(0, 1008) - 1
    assert R.count_bin(0, 2048) == R.count_bin(0, 2111) == R.count_bin(0, 2112) - 1
    assert R.count_bin(1, 7) == R.TOPK_BINS - 1 - 7 and R.count_bin(0, (1 << 63) - 1) < R.TOPK_BINS


def _terms_agg(order, size, mdc, smdc, name="c", field="kw"):
    from elasticsearch_amd import AggregationBuilders as AB
    return AB.terms(name).field(field).size(size).shardSize(size).order(order).minDocCount(mdc).shardMinDocCount(smdc)


def _assert_buckets(got, picks, counts, other, tag):
    assert got["sum_other_doc_count"] == other, "%s: other %d, expected %d" % (tag, got["sum_other_doc_count"], other)
    have = [(b["key"], b["doc_count"]) for b in got["buckets"]]
    want = [("u%07d" % o, int(c)) for o, c in zip(picks, counts)]
    assert have == want, "%s: buckets differ, first at %d" % (
        tag, next((i for i, (h, w) in enumerate(zip(have, want)) if h != w), min(len(have), len(want))))


@pytest.mark.parametrize("name", list(R.CASES))
def test_select_against_the_oracle(name):
    case = R.CASES[name]
    cols, n, mask = R.segment(case["vector"], case["T"])
    counts = R.vector(case["vector"], case["T"])
    if mask is not None:  # the accepted counts are what the request counts
        o = cols["kw"]["values"][mask]
        assert np.array_equal(np.bincount(o[o != R.MISSING], minlength=case["T"]), counts)
    else:
        o = cols["kw"]["values"]
        assert np.array_equal(np.bincount(o[o != R.MISSING].astype(np.int64), minlength=case["T"]), counts)
    from helpers import bits_from_mask
    accept = [bits_from_mask(mask)] if mask is not None else None
    aggs = [_terms_agg(*r, name="r%d" % i) for i, r in enumerate(case["requests"])]
    want = O.run([(cols, n)], aggs, accept=accept)["shards"][0]
    for i, (order, size, mdc, smdc) in enumerate(case["requests"]):
        picks, pc, other = R.select(counts, order, size, mdc, smdc)
        _assert_buckets(want["r%d" % i], picks, pc, other, "%s request %d" % (name, i))


def test_select_against_the_row_loop_on_small_vectors():
    rng = np.random.default_rng(5)
    for T in (1, 2, 5, 64, 65, 300):
        for counts in (rng.integers(0, 4, size=T), R.row_matrix(T)[0], np.zeros(T, dtype=np.int64)):
            for order in (R.COUNT_DESC, R.COUNT_ASC, R.TERM_ASC, R.TERM_DESC):
                for size in (1, 3, T, T + 2):
                    for smdc in (0, 2):
                        picks, pc, other = R.select(counts, order, size, 1, smdc)
                        kept, oth = LT.top_k(np.arange(T), counts, size, order, min_doc_count=max(smdc, 1))
                        assert kept == [(int(o), int(c)) for o, c in zip(picks, pc)] and oth == other, (T, order, size, smdc)


# ---- preconditions, by arithmetic on the input -----------------------------------------------------------------------
def _cut(name, req):
    """(count of the last pick, count of the best ordinal left out) of a count-ordered request"""
    case = R.CASES[name]
    counts = R.vector(case["vector"], case["T"])
    order, size, mdc, smdc = req
    picks, pc, _ = R.select(counts, order, size + 1, mdc, smdc)
    return (int(pc[size - 1]), int(pc[size])) if len(picks) > size else None


def test_preconditions_group_a_and_b():
    for name in R.case_names("a") + R.case_names("b") + R.case_names("d") + R.case_names("e"):
        case = R.CASES[name]
        assert case["T"] > R.GPU_TOPK_ABOVE, name  # the GPU top-k's gate
        n = R.segment(case["vector"], case["T"])[1]
        assert n < 300_000, (name, n)
    assert (R.T_TAIL1 % 4, R.T_TAIL3 % 4, R.T_NOTAIL % 4) == (1, 3, 0)
    # all equal: every ordinal is a candidate, more than one 4096-key chunk; the winners are 0 .. k-1
    for T in (R.T_TAIL1, R.T_TAIL3, R.T_NOTAIL):
        nc, _ = R.threshold_candidates(R.vector("all_equal", T), 0, 10)
        assert nc == T and -(-nc // R.TOPK_CHUNK) == 17
        assert R.select(R.vector("all_equal", T), 0, 1024)[0].tolist() == list(range(1024))
        assert R.select(R.vector("tail_winner", T), 0, 1)[0].tolist() == [T - 1]
    # shared sub-bin: at every size the counts on both sides of the cut share a bin, but for 1007 | 1008
    for order, cases in ((0, ("a_shared_subbin", "a_one_subbin")), (1, ("b_shared_subbin", "b_one_subbin"))):
        for name in cases:
            straddle = []
            for req in R.CASES[name]["requests"]:
                cut = _cut(name, req)
                if req[1] == 16:
                    assert cut is None or cut[1] == 1, (name, req)  # past the 16: the count-1 ordinals, or nothing
                    continue
                a, b = cut
                assert abs(a - b) == 1
                if R.count_bin(order, a) != R.count_bin(order, b):
                    straddle.append(sorted((a, b)))
            assert straddle == ([[1007, 1008]] if "shared" in name else []), (name, straddle)
    # octave seams: each cut between neighbours of 31 .. 129; 31 | 32 and 32 | 33 are exact bins, 63 | 64 and 127 | 128
    # straddle an octave, 64 | 65 and 128 | 129 share a sub-bin
    for name, order in (("a_octave_seams", 0), ("b_octave_seams", 1)):
        pairs = {tuple(sorted(_cut(name, r))) for r in R.CASES[name]["requests"] if _cut(name, r) and min(_cut(name, r)) > 1}
        assert pairs == {(31, 32), (32, 33), (33, 63), (63, 64), (64, 65), (65, 127), (127, 128), (128, 129)}, pairs
        assert R.count_bin(order, 64) == R.count_bin(order, 65) and R.count_bin(order, 128) == R.count_bin(order, 129)
        assert R.count_bin(order, 63) != R.count_bin(order, 64) and R.count_bin(order, 31) != R.count_bin(order, 32)
    # the tie at the cut: sizes 4 .. 7 cut inside the 5-way tie, after each tied ordinal in turn; the tied ordinals lie in
    # different 4096-chunks of the count vector and 4095 | 4096 on a chunk seam
    T = R.T_TAIL1
    tied = R.tie_ordinals(T)
    for size in range(4, 8):
        assert _cut("a_tie_at_cut", R.req(0, size)) == (50, 50)
        assert R.select(R.vector("tie_at_cut", T), 0, size)[0].tolist()[3:] == tied[:size - 3]
    assert _cut("a_tie_at_cut", R.req(0, 3)) == (80, 50) and _cut("a_tie_at_cut", R.req(0, 8)) == (50, 1)
    assert len({t // R.TOPK_CHUNK for t in tied}) == 4 and tied[1] // R.TOPK_CHUNK != tied[2] // R.TOPK_CHUNK
    # too few: 5 eligible ordinals for size 10; with min_doc_count 0 the zeros fill in by ascending ordinal
    c = R.vector("too_few", T)
    assert int((c > 0).sum()) == 5 < 10
    assert len(R.select(c, 0, 10)[0]) == 5 and R.threshold_candidates(c, 0, 10) == (5, 0)
    assert R.select(c, 0, 10, 0)[0].tolist()[5:] == [0, 1, 2, 3, 4] and R.select(c, 1, 10, 0)[0].tolist() == list(range(9)) + [10]
    # shard_min_doc_count 3: tens of thousands of ordinals below it, counted in other
    c = R.vector("shard_min", T)
    assert int((c < 3).sum()) == T - 20 and R.select(c, 0, 30, 1, 3)[2] == int(c[c < 3].sum()) and len(R.select(c, 0, 30, 1, 3)[0]) == 20
    # the 1024 gate: 1023 is no power of two, 1025 is past kTopkMax
    assert 1023 & 1022 and R.TOPK_MAX == 1024
    for name in ("a_gate_1024", "b_gate_1024"):
        cuts = [_cut(name, req) for req in R.CASES[name]["requests"]]
        assert [r[1] for r in R.CASES[name]["requests"]] == [1023, 1024, 1025]
        assert any(a == b for a, b in cuts[:2]), (name, cuts)  # a device cut inside a tie: the ordinal decides
    # count asc, min_doc_count 1: the tie on count 1 is wider than a chunk, many times
    nc, tb = R.threshold_candidates(R.vector("tie_at_cut", T), 1, 7)
    assert nc > 60_000 and nc > 4 * R.TOPK_CHUNK and tb == R.count_bin(1, 1)
    assert R.select(R.vector("tie_at_cut", T), 1, 7)[0].tolist() == [1, 2, 3, 4, 5, 6, 8]  # (0 and 7 are not at count 1)


def test_preconditions_group_c():
    for T, vec in ((R.T_NOTAIL, "every_4099"), (R.T_TAIL1, "one_workgroup")):
        c = R.vector(vec, T)
        wg = np.nonzero(c >= 2)[0] // R.per_wg(T)
        if vec == "every_4099":
            assert R.n_wg(T) == 17 and R.per_wg(T) == 4096
            assert np.bincount(wg, minlength=17).tolist() == [1] * 16 + [2]  # one per workgroup, T - 1 beside the last
            assert int((c == 1).sum()) == 17 and int((c > 0).sum()) == 35
        else:
            assert R.n_wg(T) == 17 and set((np.nonzero(c)[0] // R.per_wg(T)).tolist()) == {1}
            assert int((c > 0).sum()) == 1100 > 1024 and int((c >= 2).sum()) < 1024
    # min_doc_count 0: the first / last k ordinals, whatever their counts
    assert R.select(R.vector("every_4099", R.T_NOTAIL), R.TERM_ASC, 17, 0)[0].tolist() == list(range(17))
    assert R.select(R.vector("every_4099", R.T_NOTAIL), R.TERM_DESC, 3, 0)[0].tolist() == [R.T_NOTAIL - 1 - i for i in range(3)]


def test_preconditions_group_e():
    T = R.T_TAIL1
    c = R.vector("settled", T)
    p, pc, _ = R.select(c, 0, 11)
    assert pc[9] == 3 and pc[10] == 2 and int((c > 2).sum()) == 10  # the 10th pick one above every other ordinal
    T = R.T_NOTAIL
    c = R.vector("cold_tie", T)
    assert int((c == 1).sum()) > 60_000 > R.HOT_MAX and R.select(c, 0, 10)[1].tolist()[4:] == [10, 1, 1, 1, 1, 1]
    assert R.select(c, 0, 10)[0].tolist()[5:] == [0, 1, 2, 3, 4]
    acc, rej = R.v_cold_winner(T)
    seg = acc + rej
    x = R.COLD_X
    # whatever the hot set's size (at most HOT_MAX, at least 15 for the deferral of size 10): more ordinals at X's count
    # lie below X than any hot set holds, so X is cold; every ordinal above that count is hot; so max_cold = seg[X]
    assert int((seg[:x] == seg[x]).sum()) > R.HOT_MAX and int((seg > seg[x]).sum()) == 15 and seg[x] == 2
    picks, pc, _ = R.select(acc, 0, 10)
    assert x in picks.tolist() and pc[9] == 2 == seg[x]
    hot_only = acc.copy()
    hot_only[seg <= seg[x]] = 0  # the slots every hot set holds: their 10th count ties with max_cold
    assert R.select(hot_only, 0, 10)[1][9] == seg[x]
    acc, rej = R.v_cold_tie_accept(T)
    seg = acc + rej
    assert int((seg > 1).sum()) > R.HOT_MAX and (seg[:5] == 1).all()  # every hot ordinal has 2 docs or more: 0 .. 4 are cold
    assert R.select(acc, 0, 10)[0].tolist()[5:] == [0, 1, 2, 3, 4] and int((acc == 1).sum()) > 60_000
    acc, rej = R.v_settled_accept(R.T_TAIL1)
    assert R.select(acc, 0, 11)[1].tolist()[9:] == [3, 2] and int((acc + rej).max()) == 12 and int(rej.sum()) > 1000


def test_preconditions_rows_replay_and_colo():
    for T in R.ROW_T:
        m = R.row_matrix(T)
        if T > 64:  # two tied ordinals in one lane's strided share
            assert m[0][0] == m[0][64] and m[0][T - 1] == m[0][T - 1 - 64]
        assert len(set(m[1].tolist())) == 1 and not m[2].any() and R.ROW_MISSING[2] > 0
    assert [T <= R.ROW_LDS_KEYS for T in R.ROW_T] == [True, True, True, True, False]
    assert R.REPLAY_T > R.GPU_TOPK_ABOVE and R.replay_segment()[1] < 300_000
    assert 10 <= R.TOPK_MAX < 1500
    assert [V <= R.COLO_SEL_MAX for V in R.COLO_V] == [True] * 5 + [False]
    for V in R.COLO_V[1:]:
        a, b = R.colo_vectors(V)
        assert (a == 0).any() or V < 4
        assert a[0] == a[V - 1] == a.max()  # the first and last ordinal tied at the top of shard 0


@pytest.mark.parametrize("T", R.ROW_T)
def test_rows_against_the_oracle(T):
    from elasticsearch_amd import AggregationBuilders as AB
    cols, n = R.row_segment(T)
    reqs = R.row_requests(T)
    h = AB.dateHistogram("h").field("@timestamp").interval("1h")
    for i, r in enumerate(reqs):
        h.subAggregation(_terms_agg(*r, name="r%d" % i))
    rows = O.run([(cols, n)], [h])["shards"][0]["h"]["buckets"]
    assert [b["key"] for b in rows] == [R.T0 + r * R.HOUR for r in range(3)]
    m = R.row_matrix(T)
    for i, (order, size, mdc, smdc) in enumerate(reqs):
        for r, b in enumerate(rows):
            assert b["doc_count"] == int(m[r].sum()) + R.ROW_MISSING[r]
            picks, pc, other = R.select(m[r], order, size, mdc, smdc)
            _assert_buckets(b["r%d" % i], picks, pc, other, "T %d request %d row %d" % (T, i, r))


@pytest.mark.parametrize("order", [R.COUNT_DESC, R.COUNT_ASC])
def test_replay_rows_against_the_oracle(order):
    from elasticsearch_amd import AggregationBuilders as AB
    cols, n = R.replay_segment()
    m = R.replay_matrix()
    aggs = [AB.terms("A").field("a").size(3).shardSize(3).subAggregation(_terms_agg(order, s, 1, 0, name="B%d" % s))
            for s in (10,)]
    aggs[0].subAggregation(_terms_agg(order, 1500, 1, 0, name="B1500"))
    got = O.run([(cols, n)], aggs)["shards"][0]["A"]["buckets"]
    totals = m.sum(axis=1) + np.array([50, 0, 3])
    outer = sorted(range(3), key=lambda r: (-int(totals[r]), r))
    assert [b["key"] for b in got] == ["a%04d" % r for r in outer]
    for b, r in zip(got, outer):
        for s in (10, 1500):
            picks, pc, other = R.select(m[r], order, s)
            _assert_buckets(b["B%d" % s], picks, pc, other, "outer %d shard_size %d" % (r, s))
            # 1,500 is past the final sort; its threshold bin holds more candidates than picks: the host sorts them
            assert R.threshold_candidates(m[r], order, s)[0] >= min(s, int((m[r] > 0).sum()))


@pytest.mark.parametrize("V", R.COLO_V)
def test_colocated_reduce_against_the_oracle(V):
    from elasticsearch_amd import AggregationBuilders as AB
    shards = R.colo_segments(V)
    vec = [2 * c for c in R.colo_vectors(V)]
    for s, (cols, n) in enumerate(shards):
        o = cols["kw"]["values"]
        assert np.array_equal(np.bincount(o[o != R.MISSING].astype(np.int64), minlength=V), vec[s])
    for order, size, shard_size, mdc, smdc in R.colo_requests(V):
        aggs = [AB.terms("t").field("kw").size(size).shardSize(shard_size).order(order).minDocCount(mdc).shardMinDocCount(smdc)]
        want = O.run(shards, aggs, number_of_shards=2)["reduced"]["t"]
        per_shard = []
        for c in vec:
            picks, pc, other = R.select(c, order, min(shard_size, V), mdc, smdc)
            per_shard.append(([(int(o), int(k)) for o, k in zip(picks, pc)], other))
        buckets, _, other = LT.reduce_terms(per_shard, size, shard_size, order, min_doc_count=mdc)
        _assert_buckets(want, [b[0] for b in buckets], [b[1] for b in buckets], other, "V %d %s" % (V, (order, size, shard_size, mdc, smdc)))
