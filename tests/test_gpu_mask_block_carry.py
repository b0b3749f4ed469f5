"""The mask collects -- range (collect path 11, esgpu_range.hip), filters (12, esgpu_filters.hip) and a date_histogram
under either (13, esgpu_mask_hist.hip) -- with one workgroup walking several zone blocks.

mask_collect_launch gives every workgroup ceil(n_blocks / (CUs x occupancy)) blocks: one, at every size a test can
afford, while a shard of a billion docs gives each about a hundred.  What a workgroup carries from block to block -- the
cells of paths 11 / 12, flushed once; the key window of path 13, its mid-kernel flush, the cells' re-initialisation and
the doc counts growing across flushes -- runs here through the tests-only knob ESGPU_DEBUG_BPW, over
mask_carry_cases.BPWS, on one crafted segment of 13 zone blocks (tests/mask_carry_cases.py;
tests/test_mask_carry_cases_host.py shows without a GPU that every event occurs).

The reference never runs the code under test: the buckets' doc masks from range_ref / filters_ref / mask_hist_ref, and
per bucket the oracle's result for the children at top level with accept = the mask.  Counts and keys are exact,
integer-valued sums bit-exact (helpers.assert_same); the result is identical whatever the blocks per workgroup.
"""
import pytest

import mask_carry_cases as C
from helpers import bits_from_mask

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in C.carry_cases()}


@pytest.fixture(scope="module")
def main_seg(engine):
    s = engine.upload_segment(C.main_columns(), C.NDOCS)
    yield s
    s.close()


@pytest.fixture(scope="module")
def tail_seg(engine):
    cols, n = C.tail_columns()
    s = engine.upload_segment(cols, n)
    yield s
    s.close()


run = C.run_plan


@pytest.mark.parametrize("name,bpw", [(c.name, b) for c in CASES.values() for b in c.bpws])
def test_blocks_per_workgroup(engine, main_seg, monkeypatch, name, bpw):
    case = CASES[name]
    shard, red, stats = run(engine, monkeypatch, case, [(main_seg, C.NDOCS)], bpw)
    C.compare(case, C.reference(case, C.main_segs()), shard, red, 1, "bpw %d" % bpw)
    assert stats[2] == case.path


@pytest.mark.parametrize("name", sorted(CASES))
def test_result_and_bytes_do_not_depend_on_blocks_per_workgroup(engine, main_seg, monkeypatch, name):
    """the knob changes which workgroup adds what, never the result (the sums are integers below 2^53: no addition
    rounds) nor the algorithmic bytes; of extended_stats all but the sums of squares, which pass 2^53 and round in the
    order they are added, and what is derived from them"""
    case = CASES[name]
    part = "plain" if "extended" in name else None
    first = run(engine, monkeypatch, case, [(main_seg, C.NDOCS)], 1)
    for bpw in sorted(set(case.bpws) | {13}):
        shard, red, stats = run(engine, monkeypatch, case, [(main_seg, C.NDOCS)], bpw)
        assert stats[1] == first[2][1] and stats[2] == case.path, bpw
        assert C.part_of(shard, part) == C.part_of(first[0], part) and C.part_of(red, part) == C.part_of(first[1], part), bpw
    monkeypatch.delenv("ESGPU_DEBUG_BPW")
    plan = engine.plan([case.root()], filters=case.query, ord_lookup=C.ord_lookup)
    plan.collect(main_seg, accept_bits=bits_from_mask(case.accept_mask(C.NDOCS)) if case.accept else None)
    res = plan.build()
    assert plan.last_collect_stats()[1] == first[2][1]
    plan.close()
    assert C.part_of(res.to_dict()[case.agg_name], part) == C.part_of(first[0], part)


@pytest.mark.parametrize("bpw", [2, 13])
@pytest.mark.parametrize("order", ["main_first", "tail_first"])
@pytest.mark.parametrize("name", ["filters_hist_stats", "range_hist_stats"])
def test_two_segments_in_both_orders(engine, main_seg, tail_seg, monkeypatch, name, order, bpw):
    """the 13-block segment and a 2-block one whose keys lie above it: the grid grows before or after the long walk"""
    case = CASES[name]
    cols, n = C.tail_columns()
    main, tail = (main_seg, C.NDOCS, C.main_segs()[0]), (tail_seg, n, ("tail", cols, n))
    both = [main, tail] if order == "main_first" else [tail, main]
    shard, red, stats = run(engine, monkeypatch, case, [(s, k) for s, k, _r in both], bpw)
    C.compare(case, C.reference(case, [r for _s, _k, r in both]), shard, red, 2, "%s bpw %d" % (order, bpw))
    assert stats[2] == 13
