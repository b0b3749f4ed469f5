"""The ranked kernel (esgpu_ranked.hip): collect path 10 over block-delta keys of time-sorted data, stats or avg leaves.

Every case uploads explicit columns, collects the request with the context option ranked_terms = 1 (the ranked kernel
where the shape is eligible) and = 2 (path 10 on the generic collect kernel), and compares both with the CPU oracle under
helpers.assert_same (counts, keys and the integer-valued metric's sums bit-exact), the shard result and the reduced one;
the two options' dicts must be equal, both report path 10, and Plan.last_collect_kernel() names the kernel that ran.

Eligibility restated from esgpu_runtime.cpp (`rkk`): on top of path 10, the block layout (block-delta keys), 16-bit
metric deltas, and the segment's typical zone block inside one key -- zspan, the 90th percentile of the blocks' value
ranges (small_segment_cases.zone_keys), below the interval.  `eligible()` computes that from the timestamps; a case that
is ineligible by design asserts kernel 0 explicitly.

Shapes: the zone block holds 8,192 docs and a thread of the kernel 16 of them; the sizes put the segment's end inside
the first thread's docs, on a block's last doc, on a block boundary and one doc past it.  The window holds 8 keys.

Not constructible through the API: docs whose key lies outside the grid (the grid's key range is taken from the
segment's own extremes, so every doc of a first segment has a key in [0, H)); the kernel drops such docs by the same
range test that sends a doc past the window to the grid.
"""
import numpy as np
import pytest

import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import _native as N
from elasticsearch_amd import reduce
from helpers import assert_same
from small_segment_cases import zone_keys
from test_gpu_layouts import layout

pytestmark = pytest.mark.gpu

T0 = 1_441_065_600_000  # 2015-09-01T00:00:00Z
HOUR = 3_600_000
BLOCK = 8192
FIELDS = ("host", "@timestamp", "rt")


def request(size=10, leaf=None):
    leaf = leaf if leaf is not None else AB.stats("rt").field("rt")
    return [AB.terms("hosts").field("host").size(size).subAggregation(
        AB.dateHistogram("per_hour").field("@timestamp").interval("1h").subAggregation(leaf))]


def spaced(n, step_ms, start):
    """sorted timestamps `step_ms` apart with a little noise below the step"""
    noise = np.random.default_rng([n, step_ms]).integers(0, max(step_ms, 1), size=n)
    return (start + np.arange(n, dtype=np.int64) * step_ms + noise).astype(np.int64)


def across_boundary(n, step_ms=20):
    """an hour boundary in the middle of the docs: 20 ms apart, a run of 2,048 docs spans 41 s (16-bit deltas)"""
    return spaced(n, step_ms, T0 + 5 * HOUR - (n * step_ms) // 2)


def shard(n, ords, nterms, ts, rt=None):
    rt = rt if rt is not None else np.random.default_rng([n, 17]).integers(1, 30_000, size=n)
    assert len(ords) == n and len(ts) == n and len(rt) == n and np.all(np.diff(ts) >= 0)
    return {"host": {"type": N.COL_ORD_U32, "values": np.asarray(ords, dtype=np.uint32), "terms": ["h%04d" % i for i in range(nterms)]},
            "@timestamp": {"type": N.COL_I64, "values": np.asarray(ts, dtype=np.int64)},
            "rt": {"type": N.COL_I64, "values": np.asarray(rt, dtype=np.int64)}}


def uniform(n, nterms, seed=1):
    return np.random.default_rng([n, nterms, seed]).integers(0, nterms, size=n)


def eligible(ts):
    return zone_keys(ts, HOUR) == 0


def collect(engine, plan, seg, option):
    engine.set_option("ranked_terms", option)
    try:
        plan.collect(seg)
    finally:
        engine.set_option("ranked_terms", 1)
    return plan.last_collect_stats()[2], plan.last_collect_kernel()


def check(engine, cols, n, aggs, kernel, shards=1, name="block"):
    """both options against the oracle and each other; `kernel`: what option 1 must report"""
    want = O.run([(cols, n)], aggs, number_of_shards=shards)
    got = {}
    with layout(engine, name):
        seg = engine.upload_segment(cols, n)
        try:
            for option in (1, 2):
                plan = engine.plan(aggs, number_of_shards=shards)
                try:
                    path, kid = collect(engine, plan, seg, option)
                    assert path == 10, "option %d: path %d" % (option, path)
                    assert kid == (kernel if option == 1 else 0), "option %d: kernel %d" % (option, kid)
                    res = plan.build()
                    got[option] = (res.to_dict(), reduce([res]).to_dict())
                    assert_same(got[option][0], want["shards"][0], "option %d shard" % option)
                    assert_same(got[option][1], want["reduced"], "option %d reduced" % option)
                finally:
                    plan.close()
        finally:
            seg.close()
    assert got[1] == got[2]


# ---- docs: the tail block, one full block, a block boundary ----
@pytest.mark.parametrize("n", [1, 7, 8, 8191, 8192, 8193, 16384, 3 * BLOCK + 5])
def test_sizes(engine, n):
    ts = across_boundary(n)
    assert eligible(ts)
    check(engine, shard(n, uniform(n, 40), 40, ts), n, request(), 1)


# ---- terms and sizes ----
N_T = 2 * BLOCK + 77


@pytest.mark.parametrize("size,shards", [(1, 1), (10, 1), (128, 1), (10, 8)])
def test_sizes_of_the_request(engine, size, shards):
    """shard_size 1, 10 and 128 ranks over 300 terms, and size 10 of 8 shards (shard_size 25)"""
    ords = np.minimum(np.random.default_rng(3).zipf(1.2, size=N_T) - 1, 299)
    check(engine, shard(N_T, ords, 300, across_boundary(N_T)), N_T, request(size), 1, shards=shards)


def test_fewer_terms_than_shard_size(engine):
    check(engine, shard(N_T, uniform(N_T, 7), 7, across_boundary(N_T)), N_T, request(), 1)


def test_missing_ordinals(engine):
    ords = uniform(N_T, 60).astype(np.uint32)
    ords[np.random.default_rng(4).random(N_T) < 0.15] = 0xFFFFFFFF
    ords[-1] = 0xFFFFFFFF
    check(engine, shard(N_T, ords, 60, across_boundary(N_T)), N_T, request(), 1)


def test_one_term_holds_most_docs(engine):
    ords = uniform(N_T, 50)
    ords[np.random.default_rng(5).random(N_T) < 0.93] = 17
    assert (ords == 17).mean() > 0.9
    check(engine, shard(N_T, ords, 50, across_boundary(N_T)), N_T, request(), 1)


def test_uniform_terms_all_collected(engine):
    check(engine, shard(N_T, uniform(N_T, 10), 10, across_boundary(N_T)), N_T, request(), 1)


# ---- time ----
N_3 = 3 * BLOCK + 5


def test_one_hour(engine):
    ts = spaced(N_3, 20, T0 + 2 * HOUR + 1000)
    assert ts[0] // HOUR == ts[-1] // HOUR
    check(engine, shard(N_3, uniform(N_3, 40), 40, ts), N_3, request(), 1)


def test_hour_boundary_on_a_block_boundary(engine):
    ts = np.concatenate([spaced(BLOCK, 20, T0 + 3 * HOUR - BLOCK * 20 - 20), spaced(N_3 - BLOCK, 20, T0 + 3 * HOUR)])
    assert ts[BLOCK - 1] // HOUR + 1 == ts[BLOCK] // HOUR
    assert eligible(ts)
    check(engine, shard(N_3, uniform(N_3, 40), 40, ts), N_3, request(), 1)


def test_more_hours_than_the_window(engine):
    """12 blocks, each inside an hour of its own: the 8-key window slides (and is flushed) on the way"""
    n = 12 * BLOCK + 3
    ts = np.concatenate([spaced(min(BLOCK, n - b * BLOCK), 20, T0 + b * HOUR + 60_000) for b in range(13)])
    assert eligible(ts) and ts[-1] // HOUR - ts[0] // HOUR == 12
    check(engine, shard(n, uniform(n, 40), 40, ts), n, request(), 1)


def test_one_block_spans_more_keys_than_the_window(engine):
    """11 blocks in an hour each, but block 4 spreads over 12 hours (runs of 24-bit deltas): its docs outside the 8-key
    window reach the grid by global atomics"""
    n = 11 * BLOCK
    parts = [spaced(BLOCK, 20, T0 + (b if b < 4 else b + 12) * HOUR + 60_000) for b in range(11)]
    parts[4] = spaced(BLOCK, (12 * HOUR) // BLOCK, T0 + 4 * HOUR + 1)
    ts = np.concatenate(parts)
    assert eligible(ts) and (ts[5 * BLOCK - 1] - ts[4 * BLOCK]) // HOUR >= 11
    check(engine, shard(n, uniform(n, 40), 40, ts), n, request(), 1)


def test_block_whose_keys_span_2_to_the_32(engine):
    """one block whose first run of 2,048 docs lies 2^32 - 10^6 ms (49.7 days) before the rest -- the widest a column
    with block deltas allows: the block's 1,194 keys x interval pass 2^32, so the kernel's per-doc body divides in 64
    bits there"""
    n = 11 * BLOCK + 5  # (12 blocks: the wide one is past the 90th percentile)
    jump = (1 << 32) - 1_000_000
    ts = spaced(n, 5, T0 + jump + HOUR // 2)
    ts[:BLOCK + 2048] -= jump
    keys = ts[2 * BLOCK - 1] // HOUR - ts[BLOCK] // HOUR + 1
    assert eligible(ts) and ts[-1] - ts[0] < 1 << 32 and keys * HOUR >= 1 << 32
    check(engine, shard(n, uniform(n, 12), 12, ts), n, request(), 1)


def test_24_bit_runs(engine):
    """docs 50 ms apart: a run of 2,048 docs spans 102 s, past 16-bit deltas, so the key column carries the high-byte
    plane, which the hour-boundary block unpacks"""
    n = N_3
    ts = across_boundary(n, 50)
    assert eligible(ts) and ts[2047] - ts[0] >= 1 << 16
    check(engine, shard(n, uniform(n, 40), 40, ts), n, request(), 1)


def test_blocks_wider_than_the_interval_keep_the_generic_kernel(engine):
    """every block spans two hours: zspan >= interval, ineligible by design"""
    n = N_3
    ts = spaced(n, (2 * HOUR) // BLOCK, T0 + 1)
    assert not eligible(ts)
    check(engine, shard(n, uniform(n, 40), 40, ts), n, request(), 0)


# ---- metric ----
def test_constant_metric(engine):
    check(engine, shard(N_T, uniform(N_T, 40), 40, across_boundary(N_T), rt=np.full(N_T, 4321)), N_T, request(), 1)


def test_extrema_on_the_first_and_the_last_doc(engine):
    rt = np.random.default_rng(6).integers(1000, 2000, size=N_3)
    rt[0], rt[-1] = 1, 60_000
    ords = uniform(N_3, 40)
    ords[0] = ords[-1] = 5
    check(engine, shard(N_3, ords, 40, spaced(N_3, 20, T0 + 2 * HOUR + 1000), rt=rt), N_3, request(), 1)


def test_avg_leaf(engine):
    check(engine, shard(N_T, uniform(N_T, 40), 40, across_boundary(N_T)), N_T, request(leaf=AB.avg("rt").field("rt")), 1)


# ---- lifecycle ----
def test_collect_build_reset_collect(engine):
    n = N_3
    cols = shard(n, uniform(n, 40), 40, across_boundary(n))
    aggs = request()
    want = O.run([(cols, n)], aggs)
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        plan = engine.plan(aggs)
        try:
            for turn in range(2):
                assert collect(engine, plan, seg, 1) == (10, 1)
                assert_same(plan.build().to_dict(), want["shards"][0], "turn %d" % turn)
                plan.reset()
            assert collect(engine, plan, seg, 2) == (10, 0)
            assert_same(plan.build().to_dict(), want["shards"][0], "generic kernel after the ranked one")
        finally:
            plan.close()
            seg.close()


def test_second_segment_is_collected_again_over_every_term(engine):
    n = N_T
    parts = [shard(n, (uniform(n, 40, seed=k) * (7 if k else 1)) % 40, 40, across_boundary(n) + k * HOUR) for k in range(2)]
    one = {f: dict(parts[0][f], values=np.concatenate([p[f]["values"] for p in parts])) for f in parts[0]}
    aggs = request()
    want = O.run([(one, 2 * n)], aggs)
    with layout(engine, "block"):
        segs = [engine.upload_segment(p, n) for p in parts]
        plan = engine.plan(aggs)
        try:
            assert collect(engine, plan, segs[0], 1) == (10, 1)
            path, kid = collect(engine, plan, segs[1], 1)
            assert path != 10 and kid == 0
            res = plan.build()
            assert_same(res.to_dict(), want["shards"][0], "two segments")
            assert_same(reduce([res]).to_dict(), want["reduced"], "two segments reduced")
            plan.reset()
            path, kid = collect(engine, plan, segs[0], 1)  # ranked_off: the plan stays off the path
            assert path != 10 and kid == 0
        finally:
            plan.close()
            for s in segs:
                s.close()


# ---- layouts ----
def test_packed_layout_keeps_the_generic_kernel(engine):
    """32-bit timestamp deltas (block_deltas = 0): path 10 on the generic kernel, the same result"""
    n = N_3
    check(engine, shard(n, uniform(n, 40), 40, across_boundary(n)), n, request(), 0, name="packed")


def test_block_layout_takes_the_ranked_kernel(engine):
    n = N_3
    check(engine, shard(n, uniform(n, 40), 40, across_boundary(n)), n, request(), 1, name="block")
