"""The ranked kernel over 12-bit metric deltas (esgpu_ranked.hip, the column product d12): host wiring and kernel parity.

Every case uploads explicit columns on the block layout whose metric spans less than 4096, and collects the request four
times: ranked_terms = 1 (the ranked kernel over rank8 and d12: 1 + 1.5 bytes per doc), = 4 (the same kernel over rank8
and the 16-bit deltas), = 3 (over the 16-bit ranks and deltas) and = 2 (path 10 on the generic collect kernel).  Each is
compared with the CPU oracle under helpers.assert_same, the shard result and the reduced one; the four dicts must be
equal; all four report path 10; Plan.last_collect_kernel() is 1, 1, 1 and 0; the layout's bytes (last_collect_stats) are
the same for all four, and last_collect_read_bytes() is those bytes less n + n // 2 for option 1, less n for option 4 and
exactly those bytes for options 3 and 2.

Shapes: a thread of the kernel loads its 8 deltas of a buffer as one group of three words (es_pack12.hpp), so the sizes
end inside that group, on it and one past it, and around the zone block's 8,192 docs; the deltas 0 and 4095 -- the
column's extremes, which every cell's min, max and sum feel -- visit each of the group's 8 positions, in a full
single-key block (the unrolled body) and in the last, partial block (the per-doc body).
"""
import numpy as np
import pytest

import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Engine
from elasticsearch_amd import reduce
from helpers import assert_same
from test_gpu_layouts import layout
from test_gpu_ranked_kernel import BLOCK, HOUR, T0, across_boundary, eligible, request, shard, spaced, uniform

pytestmark = pytest.mark.gpu

OPTIONS = (1, 4, 3, 2)
KERNEL = {1: 1, 4: 1, 3: 1, 2: 0}
SPAN = 4096  # d12 holds deltas below this


def narrower(option, n, d12=True):
    """bytes the kernel of `option` streams less than the layout counts"""
    return {1: n + (n // 2 if d12 else 0), 4: n, 3: 0, 2: 0}[option]


def n_pad(n):
    return -(-n // BLOCK) * BLOCK


def narrow(n, base=1, span=SPAN - 1, seed=0):
    """n values in [base, base + span], both ends occurring once n >= 2"""
    rng = np.random.default_rng([n, span, seed])
    rt = rng.integers(base, base + span + 1, size=n).astype(np.int64)
    if n >= 2:
        lo, hi = rng.choice(n, size=2, replace=False)
        rt[lo], rt[hi] = base, base + span
    return rt


def collect(engine, plan, seg, option):
    """-> (path, kernel, layout bytes, read bytes)"""
    engine.set_option("ranked_terms", option)
    try:
        plan.collect(seg)
    finally:
        engine.set_option("ranked_terms", 1)
    _, nbytes, path = plan.last_collect_stats()
    return path, plan.last_collect_kernel(), nbytes, plan.last_collect_read_bytes()


def check(engine, cols, n, aggs, shards=1, d12=True):
    want = O.run([(cols, n)], aggs, number_of_shards=shards)
    got, stats = {}, {}
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        try:
            for option in OPTIONS:
                plan = engine.plan(aggs, number_of_shards=shards)
                try:
                    path, kid, nbytes, rbytes = collect(engine, plan, seg, option)
                    assert path == 10, "option %d: path %d" % (option, path)
                    assert kid == KERNEL[option], "option %d: kernel %d" % (option, kid)
                    assert rbytes == nbytes - narrower(option, n, d12), "option %d: %d of %d" % (option, rbytes, nbytes)
                    stats[option] = nbytes
                    res = plan.build()
                    got[option] = (res.to_dict(), reduce([res]).to_dict())
                    assert_same(got[option][0], want["shards"][0], "option %d shard" % option)
                    assert_same(got[option][1], want["reduced"], "option %d reduced" % option)
                finally:
                    plan.close()
        finally:
            seg.close()
    assert got[1] == got[4] == got[3] == got[2]
    assert stats[1] == stats[4] == stats[3] == stats[2]


# ---- sizes: the thread's first group of 8 deltas, the block boundary; bases above, across and far from zero ----
@pytest.mark.parametrize("base", [1, -2000, 1_000_000])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 3 * BLOCK + 5])
def test_sizes(engine, n, base):
    ts = across_boundary(n)
    assert eligible(ts)
    rt = narrow(n, base)
    assert n < 2 or (rt.min(), rt.max()) == (base, base + SPAN - 1)
    check(engine, shard(n, uniform(n, 40), 40, ts, rt=rt), n, request())


# ---- the span boundary: 4095 is the last span d12 holds ----
N_T = 2 * BLOCK + 77


def test_span_4095_takes_the_12_bit_form(engine):
    rt = narrow(N_T, base=-7, span=4095)
    assert rt.max() - rt.min() == 4095
    check(engine, shard(N_T, uniform(N_T, 40), 40, across_boundary(N_T), rt=rt), N_T, request())


def test_span_4096_keeps_the_16_bit_deltas(engine):
    """option 1 then streams rank8 and d16, and the column gets no d12: HBM does not grow after the option-4 collect"""
    n = N_T
    rt = narrow(n, base=-7, span=4096)
    assert rt.max() - rt.min() == 4096
    cols = shard(n, uniform(n, 40), 40, across_boundary(n), rt=rt)
    check(engine, cols, n, request(), d12=False)
    aggs = request()
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        plan = engine.plan(aggs)
        try:
            path, kid, nbytes, rbytes = collect(engine, plan, seg, 4)
            assert (path, kid, rbytes) == (10, 1, nbytes - n)
            plan.build()
            plan.reset()
            used = engine.hbm_used()
            path, kid, nbytes1, rbytes = collect(engine, plan, seg, 1)
            assert (path, kid, nbytes1, rbytes) == (10, 1, nbytes, nbytes - n)
            plan.build()
            plan.reset()
            assert engine.hbm_used() == used
        finally:
            plan.close()
            seg.close()


# ---- every position of the packed group ----
@pytest.mark.parametrize("pos", range(8))
def test_every_position_of_the_group(engine, pos):
    """Two full blocks inside one hour and a partial block inside the next.  The deltas 4095 and 0 sit at docs
    BLOCK + pos and BLOCK + 8 + pos (block 1: full, single-key -- the unrolled body) and at the same places of the last
    block (the per-doc body), nowhere else; the other docs alternate 0x5A5 / 0xA5A with period 7.  Each of the two hours
    has cells of its own, so a wrong shift or mask at `pos` in either body moves a min, a max or a sum."""
    tail = 100
    n = 2 * BLOCK + tail
    ts = np.concatenate([spaced(2 * BLOCK, 20, T0 + HOUR + 60_000), spaced(tail, 20, T0 + 2 * HOUR + 60_000)])
    assert eligible(ts) and ts[2 * BLOCK - 1] // HOUR == ts[0] // HOUR and ts[2 * BLOCK] // HOUR == ts[0] // HOUR + 1
    base = 100
    i = np.arange(n)
    rt = np.where(i % 7 < 3, base + 0x5A5, base + 0xA5A).astype(np.int64)
    for first in (BLOCK, 2 * BLOCK):
        rt[first + pos] = base + 4095
        rt[first + 8 + pos] = base
    assert np.count_nonzero(rt == base) == 2 and np.count_nonzero(rt == base + 4095) == 2
    # 5 terms, all collected: every doc's delta reaches a cell
    check(engine, shard(n, uniform(n, 5), 5, ts, rt=rt), n, request())


# ---- the per-doc body's metric unpack ----
def test_more_hours_than_the_window(engine):
    """12 blocks, each inside an hour of its own: the 8-key window slides (and is flushed) on the way"""
    n = 12 * BLOCK + 3
    ts = np.concatenate([spaced(min(BLOCK, n - b * BLOCK), 20, T0 + b * HOUR + 60_000) for b in range(13)])
    assert eligible(ts) and ts[-1] // HOUR - ts[0] // HOUR == 12
    check(engine, shard(n, uniform(n, 40), 40, ts, rt=narrow(n)), n, request())


def test_one_block_spans_more_keys_than_the_window(engine):
    """11 blocks in an hour each, but block 4 spreads over 12 hours: its docs outside the 8-key window reach the grid
    by global atomics"""
    n = 11 * BLOCK
    parts = [spaced(BLOCK, 20, T0 + (b if b < 4 else b + 12) * HOUR + 60_000) for b in range(11)]
    parts[4] = spaced(BLOCK, (12 * HOUR) // BLOCK, T0 + 4 * HOUR + 1)
    ts = np.concatenate(parts)
    assert eligible(ts) and (ts[5 * BLOCK - 1] - ts[4 * BLOCK]) // HOUR >= 11
    check(engine, shard(n, uniform(n, 40), 40, ts, rt=narrow(n, base=-2000)), n, request())


def test_hour_boundary_inside_a_block(engine):
    """four full blocks, the hour turning in the middle of block 1: that block takes the per-doc body, its neighbours
    the unrolled one"""
    n = 4 * BLOCK
    ts = spaced(n, 20, T0 + 5 * HOUR - (BLOCK + BLOCK // 2) * 20)
    assert eligible(ts) and ts[BLOCK] // HOUR < ts[2 * BLOCK - 1] // HOUR
    assert ts[0] // HOUR == ts[BLOCK - 1] // HOUR and ts[2 * BLOCK] // HOUR == ts[-1] // HOUR
    check(engine, shard(n, uniform(n, 40), 40, ts, rt=narrow(n, base=1_000_000)), n, request())


# ---- leaves and ranks ----
def test_avg_leaf(engine):
    cols = shard(N_T, uniform(N_T, 40), 40, across_boundary(N_T), rt=narrow(N_T))
    check(engine, cols, N_T, request(leaf=AB.avg("rt").field("rt")))


def test_missing_ordinals(engine):
    ords = uniform(N_T, 300).astype(np.uint32)
    ords[np.random.default_rng(4).random(N_T) < 0.15] = 0xFFFFFFFF
    ords[-1] = 0xFFFFFFFF
    check(engine, shard(N_T, ords, 300, across_boundary(N_T), rt=narrow(N_T)), N_T, request())


@pytest.mark.parametrize("size,shards", [(128, 1), (10, 8)])
def test_sizes_of_the_request(engine, size, shards):
    """128 ranks over 300 Zipf terms, and size 10 of 8 shards (shard_size 25)"""
    ords = np.minimum(np.random.default_rng(3).zipf(1.2, size=N_T) - 1, 299)
    check(engine, shard(N_T, ords, 300, across_boundary(N_T), rt=narrow(N_T)), N_T, request(size), shards=shards)


# ---- lifecycle: d12 is built by the first option-1 collect, on a column that already has rank8 and d16 ----
def test_lifecycle(engine):
    n = 3 * BLOCK + 5
    cols = shard(n, uniform(n, 40), 40, across_boundary(n), rt=narrow(n))
    aggs = request()
    want = O.run([(cols, n)], aggs)["shards"][0]
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        plan = engine.plan(aggs)
        other = None
        try:
            path, kid, nbytes, rbytes = collect(engine, plan, seg, 4)
            assert (path, kid, rbytes) == (10, 1, nbytes - n)
            assert_same(plan.build().to_dict(), want, "option 4")
            plan.reset()
            with_rank8 = engine.hbm_used()
            for turn in range(2):
                path, kid, nbytes1, rbytes = collect(engine, plan, seg, 1)
                assert (path, kid, nbytes1, rbytes) == (10, 1, nbytes, nbytes - n - n // 2)
                assert_same(plan.build().to_dict(), want, "option 1, turn %d" % turn)
                plan.reset()
                # the product: 1.5 bytes per doc of the padded segment, allocated once
                assert engine.hbm_used() - with_rank8 == n_pad(n) * 3 // 2, "turn %d" % turn
            cached = engine.hbm_used()
            other = engine.plan(aggs)
            path, kid, nbytes2, rbytes = collect(engine, other, seg, 1)
            assert (path, kid, nbytes2, rbytes) == (10, 1, nbytes, nbytes - n - n // 2)
            assert_same(other.build().to_dict(), want, "a second plan")
            other.close()
            other = None
            assert engine.hbm_used() == cached  # (the plan's own buffers are gone again: nothing was added to the segment)
            path, kid, nbytes4, rbytes = collect(engine, plan, seg, 4)
            assert (path, kid, nbytes4, rbytes) == (10, 1, nbytes, nbytes - n)
            assert_same(plan.build().to_dict(), want, "option 4 again")
            plan.reset()
            assert engine.hbm_used() == cached
        finally:
            if other is not None:
                other.close()
            plan.close()
            seg.close()


# ---- over the HBM budget the request keeps the ranked kernel, over rank8 and d16 ----
def _collect4_build(e, cols, n, aggs):
    seg = e.upload_segment(cols, n)
    plan = e.plan(aggs)
    collect(e, plan, seg, 4)
    res = plan.build().to_dict()
    plan.reset()
    return seg, plan, res


def test_budget_fallback(engine):
    """The budget: what a fresh context holds after the upload, an option-4 collect and its build (measured on a probe
    context of its own, so that the context's own buffers and the plan's are counted), plus one byte less than the
    n_pad * 3 / 2 that d12 needs"""
    n = 4 * BLOCK
    cols = shard(n, uniform(n, 40), 40, across_boundary(n), rt=narrow(n))
    aggs = request()
    want = O.run([(cols, n)], aggs)["shards"][0]
    probe = Engine(0)
    try:
        with layout(probe, "block"):
            seg, plan, res = _collect4_build(probe, cols, n, aggs)
            need = probe.hbm_used()
            plan.close()
            seg.close()
    finally:
        probe.close()
    assert_same(res, want, "probe")
    small = Engine(0, hbm_budget_bytes=need + n_pad(n) * 3 // 2 - 1)
    try:
        with layout(small, "block"):
            seg, plan, res = _collect4_build(small, cols, n, aggs)
            try:
                assert_same(res, want, "option 4")
                assert small.hbm_used() == need
                path, kid, nbytes, rbytes = collect(small, plan, seg, 1)
                assert (path, kid) == (10, 1) and rbytes == nbytes - n, "rank8 and the 16-bit deltas"
                assert_same(plan.build().to_dict(), want, "option 1 over the budget")
                assert small.hbm_used() == need
            finally:
                plan.close()
                seg.close()
    finally:
        small.close()
