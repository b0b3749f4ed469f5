"""The ranked kernel over 8-bit ranks (esgpu_ranked.hip, the segment product rank8): host wiring and kernel parity.

Every case uploads explicit columns on the block layout and collects the request three times: ranked_terms = 1 (the
ranked kernel over rank8, one byte per doc: min(rank, 255)), = 3 (the same kernel over the 16-bit ranks) and = 2 (path 10
on the generic collect kernel).  Each is compared with the CPU oracle under helpers.assert_same, the shard result and
the reduced one; the three dicts must be equal; all three report path 10; Plan.last_collect_kernel() is 1, 1 and 0; the
layout's bytes (last_collect_stats) are the same for all three, and last_collect_read_bytes() is those bytes less one per
doc for option 1 and exactly those bytes for options 2 and 3.

Shapes: a thread of the kernel loads its 8 ranks of a buffer as one 8-byte word, so the sizes end inside that word, on
it and one past it, and around the zone block's 8,192 docs.

The saturation case wants strictly decreasing term counts, which T terms admit only from T (T + 1) / 2 docs on: its
n = 2 * 8192 + 77 holds for 128 and 129 terms, and grows by whole blocks (k * 8192 + 77) for 254 terms and more.
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

OPTIONS = (1, 3, 2)
KERNEL = {1: 1, 3: 1, 2: 0}


def collect(engine, plan, seg, option):
    """-> (path, kernel, layout bytes, read bytes)"""
    engine.set_option("ranked_terms", option)
    try:
        plan.collect(seg)
    finally:
        engine.set_option("ranked_terms", 1)
    _, nbytes, path = plan.last_collect_stats()
    return path, plan.last_collect_kernel(), nbytes, plan.last_collect_read_bytes()


def check(engine, cols, n, aggs, shards=1):
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
                    assert rbytes == nbytes - (n if option == 1 else 0), "option %d: %d of %d" % (option, rbytes, nbytes)
                    stats[option] = nbytes
                    res = plan.build()
                    got[option] = (res.to_dict(), reduce([res]).to_dict())
                    assert_same(got[option][0], want["shards"][0], "option %d shard" % option)
                    assert_same(got[option][1], want["reduced"], "option %d reduced" % option)
                finally:
                    plan.close()
        finally:
            seg.close()
    assert got[1] == got[3] == got[2]
    assert stats[1] == stats[3] == stats[2]


# ---- sizes: the thread's first 8-byte rank word, the block boundary ----
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 3 * BLOCK + 5])
def test_sizes(engine, n):
    ts = across_boundary(n)
    assert eligible(ts)
    check(engine, shard(n, uniform(n, 40), 40, ts), n, request())


# ---- the saturation boundary: ranks 127 | 128 (collected or not) and 254 | 255 (a rank of its own, or 0xFF) ----
FEW = 3


def decreasing(nterms):
    """-> (n, ords): term of rank r holds nterms - r + FEW - 1 docs (strictly decreasing, FEW at the last rank); n is the
    smallest k * 8192 + 77, k >= 2, that holds them, the docs left over go half to rank 0 and half to the missing
    ordinal.  Ordinals are a permutation of the ranks and the docs are shuffled."""
    counts = np.arange(nterms, 0, -1) + FEW - 1
    k = max(2, -(-(int(counts.sum()) - 77) // BLOCK))
    n = k * BLOCK + 77
    spare = n - int(counts.sum())
    assert spare >= 0
    counts[0] += spare - spare // 2
    assert np.all(np.diff(counts) < 0) and counts.min() >= FEW
    rng = np.random.default_rng([nterms, 8])
    ord_of_rank = rng.permutation(nterms).astype(np.uint32)
    ords = np.concatenate([np.repeat(ord_of_rank, counts), np.full(spare // 2, 0xFFFFFFFF, dtype=np.uint32)])
    rng.shuffle(ords)
    return n, ords


@pytest.mark.parametrize("nterms", [128, 129, 254, 255, 256, 257, 600])
def test_saturation_boundary(engine, nterms):
    """shard_size 128: ranks 128.. are not collected; ranks 255.. and the missing ordinal all read 0xFF"""
    n, ords = decreasing(nterms)
    assert (n == 2 * BLOCK + 77) == (nterms <= 129)
    ts = across_boundary(n)
    assert eligible(ts)
    check(engine, shard(n, ords, nterms, ts), n, request(128))


N_T = 2 * BLOCK + 77


def test_missing_ordinals(engine):
    ords = uniform(N_T, 300).astype(np.uint32)
    ords[np.random.default_rng(4).random(N_T) < 0.15] = 0xFFFFFFFF
    ords[-1] = 0xFFFFFFFF
    check(engine, shard(N_T, ords, 300, across_boundary(N_T)), N_T, request())


def test_avg_leaf(engine):
    check(engine, shard(N_T, uniform(N_T, 40), 40, across_boundary(N_T)), N_T, request(leaf=AB.avg("rt").field("rt")))


# ---- the per-doc body's rank unpack ----
def test_more_hours_than_the_window(engine):
    """12 blocks, each inside an hour of its own: the 8-key window slides (and is flushed) on the way"""
    n = 12 * BLOCK + 3
    ts = np.concatenate([spaced(min(BLOCK, n - b * BLOCK), 20, T0 + b * HOUR + 60_000) for b in range(13)])
    assert eligible(ts) and ts[-1] // HOUR - ts[0] // HOUR == 12
    check(engine, shard(n, uniform(n, 40), 40, ts), n, request())


def test_one_block_spans_more_keys_than_the_window(engine):
    """11 blocks in an hour each, but block 4 spreads over 12 hours: its docs outside the 8-key window reach the grid
    by global atomics"""
    n = 11 * BLOCK
    parts = [spaced(BLOCK, 20, T0 + (b if b < 4 else b + 12) * HOUR + 60_000) for b in range(11)]
    parts[4] = spaced(BLOCK, (12 * HOUR) // BLOCK, T0 + 4 * HOUR + 1)
    ts = np.concatenate(parts)
    assert eligible(ts) and (ts[5 * BLOCK - 1] - ts[4 * BLOCK]) // HOUR >= 11
    check(engine, shard(n, uniform(n, 40), 40, ts), n, request())


# ---- lifecycle: rank8 is built by the first option-1 collect, on a column that already has its ranks ----
def test_lifecycle(engine):
    n = 3 * BLOCK + 5
    cols = shard(n, uniform(n, 40), 40, across_boundary(n))
    aggs = request()
    want = O.run([(cols, n)], aggs)["shards"][0]
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        plan = engine.plan(aggs)
        other = None
        try:
            used = engine.hbm_used()
            path, kid, nbytes, rbytes = collect(engine, plan, seg, 3)
            assert (path, kid, rbytes) == (10, 1, nbytes)
            assert_same(plan.build().to_dict(), want, "option 3")
            plan.reset()
            with_rank16 = engine.hbm_used()
            assert with_rank16 > used
            for turn in range(2):
                path, kid, nbytes1, rbytes = collect(engine, plan, seg, 1)
                assert (path, kid, nbytes1, rbytes) == (10, 1, nbytes, nbytes - n)
                assert_same(plan.build().to_dict(), want, "option 1, turn %d" % turn)
                plan.reset()
                # the product: one byte per doc of the padded segment, allocated once
                assert engine.hbm_used() - with_rank16 == -(-n // BLOCK) * BLOCK, "turn %d" % turn
            cached = engine.hbm_used()
            other = engine.plan(aggs)
            path, kid, nbytes2, rbytes = collect(engine, other, seg, 1)
            assert (path, kid, nbytes2, rbytes) == (10, 1, nbytes, nbytes - n)
            assert_same(other.build().to_dict(), want, "a second plan")
            other.close()
            other = None
            assert engine.hbm_used() == cached  # (the plan's own buffers are gone again: nothing was added to the segment)
        finally:
            if other is not None:
                other.close()
            plan.close()
            seg.close()


# ---- over the HBM budget the request keeps the ranked kernel, over rank16 ----
def _collect3_build(e, cols, n, aggs):
    seg = e.upload_segment(cols, n)
    plan = e.plan(aggs)
    collect(e, plan, seg, 3)
    res = plan.build().to_dict()
    plan.reset()
    return seg, plan, res


def test_budget_fallback(engine):
    """The budget: what a fresh context holds after the upload, an option-3 collect and its build (measured on a probe
    context of its own, so that the context's own buffers and the plan's are counted), plus less than n / 2 bytes --
    rank8 needs n"""
    n = 4 * BLOCK
    cols = shard(n, uniform(n, 40), 40, across_boundary(n))
    aggs = request()
    want = O.run([(cols, n)], aggs)["shards"][0]
    probe = Engine(0)
    try:
        with layout(probe, "block"):
            seg, plan, res = _collect3_build(probe, cols, n, aggs)
            need = probe.hbm_used()
            plan.close()
            seg.close()
    finally:
        probe.close()
    assert_same(res, want, "probe")
    small = Engine(0, hbm_budget_bytes=need + n // 2 - 1)
    try:
        with layout(small, "block"):
            seg, plan, res = _collect3_build(small, cols, n, aggs)
            try:
                assert_same(res, want, "option 3")
                assert small.hbm_used() == need
                path, kid, nbytes, rbytes = collect(small, plan, seg, 1)
                assert (path, kid) == (10, 1) and rbytes == nbytes, "the 2-byte form"
                assert_same(plan.build().to_dict(), want, "option 1 over the budget")
                assert small.hbm_used() == need
            finally:
                plan.close()
                seg.close()
    finally:
        small.close()
