"""The grouped ranked kernel (esgpu_ranked_grouped.hip) over rank-grouped 12-bit deltas (es_group12.hpp, the product g12).

Every case uploads explicit columns on the block layout and collects the request three times: ranked_terms = 5 (the
grouped form), = 1 (the ranked kernel over rank8 and d12) and = 2 (path 10 on the generic collect kernel).  Each is
compared with the CPU oracle under helpers.assert_same, the shard result and the reduced one; the three dicts must be
equal; all report path 10; Plan.last_collect_kernel() is 2, 1 and 0; the layout's bytes (last_collect_stats) are the same
for all three, and last_collect_read_bytes() of option 5 is the figure `grouped_read_bytes` computes from the columns by
the header's definition: the layout's bytes, less the 4 bytes of rank16 and d16 per doc of the zone blocks inside one
hour, plus for every block the 12 bytes of each group of 8 positions below off[K] and the block's 260 bytes of offsets.

The session's engine is shared and the other tests leave the option at 1: every collect here sets the option it wants
and puts back the value it found.
"""
import numpy as np
import pytest

import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import Engine
from elasticsearch_amd import reduce
from helpers import assert_same
from test_gpu_layouts import layout
from test_gpu_ranked_block_carry import FORMS, SEQUENCES, case
from test_gpu_ranked_d12 import N_T, SPAN, n_pad, narrow
from test_gpu_ranked_kernel import BLOCK, HOUR, T0, across_boundary, eligible, request, shard, spaced, uniform

pytestmark = pytest.mark.gpu

OPTIONS = (5, 1, 2)
MISSING = 0xFFFFFFFF
# es_group12.hpp / es_pack12.hpp
GROUP_DOCS, GROUP_BYTES = 8, 12
OFF_BYTES = 260
BLOCK_BYTES = BLOCK // GROUP_DOCS * GROUP_BYTES


def product_bytes(n):
    return n_pad(n) // BLOCK * (BLOCK_BYTES + OFF_BYTES)


def ranks_of(ords, nterms):
    """each doc's frequency rank (es_term_rank.hpp: count descending, then the ordinal ascending); -1: no term"""
    ords = np.asarray(ords, dtype=np.int64)
    have = ords != MISSING
    counts = np.bincount(ords[have], minlength=nterms)
    ord_of_rank = np.lexsort((np.arange(nterms), -counts))
    rank_of = np.empty(nterms, dtype=np.int64)
    rank_of[ord_of_rank] = np.arange(nterms)
    return np.where(have, rank_of[np.where(have, ords, 0)], -1)


def grouped_read_bytes(nbytes, cols, n, k):
    """what the grouped form reads of a segment whose layout counts `nbytes`, collecting the ranks below k"""
    ords, ts = cols["host"]["values"], cols["@timestamp"]["values"]
    rank = ranks_of(ords, len(cols["host"]["terms"]))
    total = nbytes
    for b in range(0, n, BLOCK):
        keys = ts[b:b + BLOCK] // HOUR
        if keys.min() == keys.max():
            total -= 4 * len(keys)
        r = rank[b:b + BLOCK]
        off_k = int(np.count_nonzero((r >= 0) & (r < k)))
        total += -(-off_k // GROUP_DOCS) * GROUP_BYTES + OFF_BYTES
    return total


def collect(engine, plan, seg, option):
    """-> (path, kernel, layout bytes, read bytes)"""
    found = engine.get_option("ranked_terms")
    engine.set_option("ranked_terms", option)
    try:
        plan.collect(seg)
    finally:
        engine.set_option("ranked_terms", found)
    _, nbytes, path = plan.last_collect_stats()
    return path, plan.last_collect_kernel(), nbytes, plan.last_collect_read_bytes()


def check(engine, cols, n, aggs, k, shards=1, grouped=True, want=None, d12=True):
    """k: the ranks the request collects (min(shard_size, terms)); grouped False: option 5 must run as option 1 does,
    over d12 or (d12 False) the 16-bit deltas"""
    want = want if want is not None else O.run([(cols, n)], aggs, number_of_shards=shards)
    kernel = {5: 2 if grouped else 1, 1: 1, 2: 0}
    got, stats = {}, {}
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        try:
            for option in OPTIONS:
                plan = engine.plan(aggs, number_of_shards=shards)
                try:
                    path, kid, nbytes, rbytes = collect(engine, plan, seg, option)
                    assert path == 10, "option %d: path %d" % (option, path)
                    assert kid == kernel[option], "option %d: kernel %d" % (option, kid)
                    as_1 = nbytes - n - (n // 2 if d12 else 0)
                    expect = {5: grouped_read_bytes(nbytes, cols, n, k) if grouped else as_1, 1: as_1, 2: nbytes}[option]
                    assert rbytes == expect, "option %d: read %d, expected %d of %d" % (option, rbytes, expect, nbytes)
                    stats[option] = nbytes
                    res = plan.build()
                    got[option] = (res.to_dict(), reduce([res]).to_dict())
                    assert_same(got[option][0], want["shards"][0], "option %d shard" % option)
                    assert_same(got[option][1], want["reduced"], "option %d reduced" % option)
                finally:
                    plan.close()
        finally:
            seg.close()
    assert got[5] == got[1] == got[2]
    assert stats[5] == stats[1] == stats[2]


# ---- sizes: inside the first group of 8, around the zone block, pad docs in the last block's group 128 ----
@pytest.mark.parametrize("n", [1, 7, 8, 9, 8191, 8192, 8193, 3 * BLOCK + 5])
def test_sizes(engine, n):
    ts = across_boundary(n)
    assert eligible(ts)
    check(engine, shard(n, uniform(n, 40), 40, ts, rt=narrow(n)), n, request(), 10)


# ---- run boundaries at every position of the packed group ----
def crafted_block(counts, missing, rng, base):
    """one block's ordinals (counts[t] docs of term t, `missing` docs without a term, shuffled) and metric values: 0 on
    the first doc of every term's run (in doc order), 4095 on its last, values strictly between elsewhere"""
    assert sum(counts) + missing == BLOCK
    ords = np.concatenate([np.full(c, t, dtype=np.int64) for t, c in enumerate(counts)] + [np.full(missing, MISSING, dtype=np.int64)])
    rng.shuffle(ords)
    rt = base + rng.integers(1, SPAN - 1, size=BLOCK)
    for t, c in enumerate(counts):
        at = np.flatnonzero(ords == t)
        if c >= 1:
            rt[at[0]] = base
        if c >= 2:
            rt[at[-1]] = base + SPAN - 1
    return ords, rt


@pytest.mark.parametrize("size", [5, 3])
@pytest.mark.parametrize("pos", range(8))
def test_run_boundaries_at_every_position(engine, pos, size):
    """Three full blocks inside one hour, 5 terms.  Block 1's runs end at positions pos, pos + 1 + 8 a, ... so that the
    boundary between every two neighbouring ranks, and off[K] itself (some docs have no term), falls at each of the 8
    positions of a packed group as pos goes round; blocks 0 and 2 keep the ranks in the order of the ordinals."""
    rng = np.random.default_rng([pos, 11])
    ordinary = (3000, 2400, 1500, 800, 400)
    runs = (2000 + pos, 1601, 1201, 801, 401)  # boundaries at pos, pos + 1, pos + 2, pos + 3, pos + 4 (mod 8)
    blocks = [crafted_block(ordinary, BLOCK - sum(ordinary), rng, 100),
              crafted_block(runs, BLOCK - sum(runs), rng, 100),
              crafted_block(ordinary, BLOCK - sum(ordinary), rng, 100)]
    ords = np.concatenate([b[0] for b in blocks])
    rt = np.concatenate([b[1] for b in blocks])
    n = len(ords)
    assert [sum(runs[:r + 1]) % 8 for r in range(5)] == [(pos + r) % 8 for r in range(5)]
    assert np.array_equal(ranks_of(ords, 5)[ords != MISSING], ords[ords != MISSING])
    assert (rt.min(), rt.max()) == (100, 100 + SPAN - 1)
    ts = spaced(n, 20, T0 + HOUR + 60_000)
    assert eligible(ts) and ts[0] // HOUR == ts[-1] // HOUR
    check(engine, shard(n, ords.astype(np.uint32), 5, ts, rt=rt), n, request(size), size)


# ---- degenerate runs ----
@pytest.mark.parametrize("size", [5, 3])
def test_degenerate_runs(engine, size):
    """Eight full blocks inside one hour, 5 terms whose ranks are their ordinals: an ordinary block; a rank without a doc;
    two such ranks in a row; runs of 1, 2, 1, 2 and 1 docs (one thread's 8 positions span five ranks and the end of the
    prefix); no collected doc at all (off[K] = 0) between ordinary neighbours; every doc of rank 0 (two passes); and,
    with size 5, the ordinary blocks collect every doc (K = T = 5)."""
    rng = np.random.default_rng(23)
    ordinary = (3000, 2500, 1500, 800, 392)
    per_block = [ordinary, (4000, 0, 2000, 1000, 1192), (6000, 0, 0, 2000, 192), (1, 2, 1, 2, 1), ordinary,
                 (0, 0, 0, 0, 0), ordinary, (BLOCK, 0, 0, 0, 0)]
    blocks = [crafted_block(c, BLOCK - sum(c), rng, -2000) for c in per_block]
    ords = np.concatenate([b[0] for b in blocks])
    rt = np.concatenate([b[1] for b in blocks])
    n = len(ords)
    assert np.array_equal(ranks_of(ords, 5)[ords != MISSING], ords[ords != MISSING])
    ts = spaced(n, 20, T0 + HOUR + 60_000)
    assert eligible(ts) and ts[0] // HOUR == ts[-1] // HOUR
    check(engine, shard(n, ords.astype(np.uint32), 5, ts, rt=rt), n, request(size), size)


# ---- request shapes ----
def test_avg_leaf(engine):
    cols = shard(N_T, uniform(N_T, 40), 40, across_boundary(N_T), rt=narrow(N_T))
    check(engine, cols, N_T, request(leaf=AB.avg("rt").field("rt")), 10)


def test_missing_ordinals(engine):
    ords = uniform(N_T, 300).astype(np.uint32)
    ords[np.random.default_rng(4).random(N_T) < 0.15] = MISSING
    ords[-1] = MISSING
    check(engine, shard(N_T, ords, 300, across_boundary(N_T), rt=narrow(N_T)), N_T, request(), 10)


@pytest.mark.parametrize("size,shards,k", [(128, 1, 128), (10, 8, 80)])
def test_sizes_of_the_request(engine, monkeypatch, size, shards, k):
    """128 ranks over 300 Zipf terms (both registers of offsets), and size 10 of 8 shards (the default shard_size is then
    size x min(10, shards) = 80: offsets in both registers as well)"""
    monkeypatch.setenv("ESGPU_G12_MAX_K", "128")  # (past 16 ranks option 5 runs as option 1 unless the bound is moved)
    ords = np.minimum(np.random.default_rng(3).zipf(1.2, size=N_T) - 1, 299)
    check(engine, shard(N_T, ords, 300, across_boundary(N_T), rt=narrow(N_T)), N_T, request(size), k, shards=shards)


@pytest.mark.parametrize("size,grouped", [(16, True), (17, False)])
def test_the_bound_on_the_ranks(engine, monkeypatch, size, grouped):
    """16 ranks take the grouped form, 17 run as option 1 does (rank8 and d12): the form loses where a wave's positions
    meet many offsets"""
    monkeypatch.delenv("ESGPU_G12_MAX_K", raising=False)
    ords = np.minimum(np.random.default_rng(3).zipf(1.2, size=N_T) - 1, 299)
    check(engine, shard(N_T, ords, 300, across_boundary(N_T), rt=narrow(N_T)), N_T, request(size), size, grouped=grouped)


def test_span_4095_takes_the_grouped_form(engine):
    rt = narrow(N_T, base=-7, span=4095)
    assert rt.max() - rt.min() == 4095
    check(engine, shard(N_T, uniform(N_T, 40), 40, across_boundary(N_T), rt=rt), N_T, request(), 10)


def test_span_4096_runs_as_option_1(engine):
    """rank8 and the 16-bit deltas, and no product: HBM does not grow after an option-1 collect"""
    n = N_T
    rt = narrow(n, base=-7, span=4096)
    assert rt.max() - rt.min() == 4096
    cols = shard(n, uniform(n, 40), 40, across_boundary(n), rt=rt)
    check(engine, cols, n, request(), 10, grouped=False, d12=False)
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        plan = engine.plan(request())
        try:
            path, kid, nbytes, rbytes = collect(engine, plan, seg, 1)
            assert (path, kid, rbytes) == (10, 1, nbytes - n)
            plan.build()
            plan.reset()
            used = engine.hbm_used()
            path, kid, nbytes5, rbytes = collect(engine, plan, seg, 5)
            assert (path, kid, nbytes5, rbytes) == (10, 1, nbytes, nbytes - n)
            plan.build()
            plan.reset()
            assert engine.hbm_used() == used
        finally:
            plan.close()
            seg.close()


# ---- block kinds ----
def test_hour_boundary_inside_a_block(engine):
    """four full blocks, the hour turning in the middle of block 1: that block takes the per-doc body over the original
    columns, its neighbours the grouped one"""
    n = 4 * BLOCK
    ts = spaced(n, 20, T0 + 5 * HOUR - (BLOCK + BLOCK // 2) * 20)
    assert eligible(ts) and ts[BLOCK] // HOUR < ts[2 * BLOCK - 1] // HOUR
    assert ts[0] // HOUR == ts[BLOCK - 1] // HOUR and ts[2 * BLOCK] // HOUR == ts[-1] // HOUR
    check(engine, shard(n, uniform(n, 40), 40, ts, rt=narrow(n, base=1_000_000)), n, request(), 10)


def test_one_block_spans_more_keys_than_the_window(engine):
    """11 blocks in an hour each, but block 4 spreads over 12 hours: its docs outside the 8-key window reach the grid
    by global atomics"""
    n = 11 * BLOCK
    parts = [spaced(BLOCK, 20, T0 + (b if b < 4 else b + 12) * HOUR + 60_000) for b in range(11)]
    parts[4] = spaced(BLOCK, (12 * HOUR) // BLOCK, T0 + 4 * HOUR + 1)
    ts = np.concatenate(parts)
    assert eligible(ts) and (ts[5 * BLOCK - 1] - ts[4 * BLOCK]) // HOUR >= 11
    check(engine, shard(n, uniform(n, 40), 40, ts, rt=narrow(n, base=-2000)), n, request(), 10)


def test_more_hours_than_the_window(engine):
    """12 blocks, each inside an hour of its own: the 8-key window slides (and is flushed) on the way"""
    n = 12 * BLOCK + 3
    ts = np.concatenate([spaced(min(BLOCK, n - b * BLOCK), 20, T0 + b * HOUR + 60_000) for b in range(13)])
    assert eligible(ts) and ts[-1] // HOUR - ts[0] // HOUR == 12
    check(engine, shard(n, uniform(n, 40), 40, ts, rt=narrow(n)), n, request(), 10)


@pytest.mark.parametrize("bpw", [12, 5, 2])
@pytest.mark.parametrize("form", ["d12", "avg_d12"])
@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_block_carry(engine, monkeypatch, seq, form, bpw):
    """test_gpu_ranked_block_carry's sequences of single-key, two-key, wide and partial blocks with 12, 5 and 2 blocks per
    workgroup: the two buffers and the scalar prefetch of keys and off[K] are carried from block to block, over blocks
    that take either body and over the range's end"""
    assert FORMS[form][1] < SPAN
    cols, n, aggs, want = case(seq, form)
    monkeypatch.setenv("ESGPU_DEBUG_BPW", str(bpw))
    check(engine, cols, n, aggs, 10, want=want)


# ---- lifecycle: the product is built by the first option-5 collect, one per metric column ----
def test_lifecycle(engine):
    n = 3 * BLOCK + 5
    cols = shard(n, uniform(n, 40), 40, across_boundary(n), rt=narrow(n))
    cols["rt2"] = {"type": cols["rt"]["type"], "values": narrow(n, base=-300, seed=5)}
    aggs, aggs2 = request(), request(leaf=AB.stats("rt2").field("rt2"))
    wants = [O.run([(cols, n)], a)["shards"][0] for a in (aggs, aggs2)]
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        plans = [engine.plan(aggs), engine.plan(aggs2)]
        other = None
        try:
            # the 16-bit ranks and deltas of both metrics, the keys and the plans' own buffers: everything but the products
            nbytes = []
            for plan, want in zip(plans, wants):
                path, kid, nb, rbytes = collect(engine, plan, seg, 3)
                assert (path, kid, rbytes) == (10, 1, nb)
                assert_same(plan.build().to_dict(), want, "option 3")
                plan.reset()
                nbytes.append(nb)
            before = engine.hbm_used()
            for turn in range(2):
                path, kid, nb, rbytes = collect(engine, plans[0], seg, 5)
                assert (path, kid, nb, rbytes) == (10, 2, nbytes[0], grouped_read_bytes(nbytes[0], cols, n, 10))
                assert_same(plans[0].build().to_dict(), wants[0], "option 5, turn %d" % turn)
                plans[0].reset()
                # the product: data and offsets of every block of the padded segment, allocated once
                assert engine.hbm_used() - before == product_bytes(n), "turn %d" % turn
            cached = engine.hbm_used()
            other = engine.plan(aggs)
            path, kid, nb, rbytes = collect(engine, other, seg, 5)
            assert (path, kid, nb) == (10, 2, nbytes[0])
            assert_same(other.build().to_dict(), wants[0], "a second plan")
            other.close()
            other = None
            assert engine.hbm_used() == cached  # (the plan's own buffers are gone again: nothing was added to the segment)
            # the second metric column gets a product of its own
            path, kid, nb, rbytes = collect(engine, plans[1], seg, 5)
            assert (path, kid, nb, rbytes) == (10, 2, nbytes[1], grouped_read_bytes(nbytes[1], cols, n, 10))
            assert_same(plans[1].build().to_dict(), wants[1], "the second metric")
            plans[1].reset()
            assert engine.hbm_used() - before == 2 * product_bytes(n)
            path, kid, nb, rbytes = collect(engine, plans[0], seg, 5)
            assert (path, kid) == (10, 2)
            assert_same(plans[0].build().to_dict(), wants[0], "the first metric again")
            plans[0].reset()
            assert engine.hbm_used() - before == 2 * product_bytes(n)
            # neither rank8 nor d12 was built on the way: option 1 builds them now
            path, kid, nb, rbytes = collect(engine, plans[0], seg, 1)
            assert (path, kid, rbytes) == (10, 1, nbytes[0] - n - n // 2)
            assert_same(plans[0].build().to_dict(), wants[0], "option 1")
            plans[0].reset()
            assert engine.hbm_used() - before == 2 * product_bytes(n) + n_pad(n) + n_pad(n) * 3 // 2
        finally:
            if other is not None:
                other.close()
            for plan in plans:
                plan.close()
            seg.close()


# ---- over the HBM budget option 5 runs as option 1 ----
def _collect1_build(e, cols, n, aggs):
    seg = e.upload_segment(cols, n)
    plan = e.plan(aggs)
    collect(e, plan, seg, 1)
    res = plan.build().to_dict()
    plan.reset()
    return seg, plan, res


def test_budget_fallback(engine):
    """The budget: what a fresh context holds after the upload, an option-1 collect and its build (measured on a probe
    context of its own), plus one byte less than the product needs"""
    n = 4 * BLOCK
    cols = shard(n, uniform(n, 40), 40, across_boundary(n), rt=narrow(n))
    aggs = request()
    want = O.run([(cols, n)], aggs)["shards"][0]
    probe = Engine(0)
    try:
        with layout(probe, "block"):
            seg, plan, res = _collect1_build(probe, cols, n, aggs)
            need = probe.hbm_used()
            plan.close()
            seg.close()
    finally:
        probe.close()
    assert_same(res, want, "probe")
    small = Engine(0, hbm_budget_bytes=need + product_bytes(n) - 1)
    try:
        with layout(small, "block"):
            seg, plan, res = _collect1_build(small, cols, n, aggs)
            try:
                assert_same(res, want, "option 1")
                assert small.hbm_used() == need
                for turn in range(2):
                    path, kid, nbytes, rbytes = collect(small, plan, seg, 5)
                    assert (path, kid) == (10, 1) and rbytes == nbytes - n - n // 2, "rank8 and d12, turn %d" % turn
                    assert_same(plan.build().to_dict(), want, "option 5 over the budget")
                    plan.reset()
                    assert small.hbm_used() == need
            finally:
                plan.close()
                seg.close()
    finally:
        small.close()
