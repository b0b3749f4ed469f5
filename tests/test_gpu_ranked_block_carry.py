"""The ranked kernel's block-to-block carry (esgpu_ranked.hip): the two buffers a workgroup reloads for its next block.

A workgroup walks `blocks_per_wg` zone blocks, and for each it holds the block's 16 docs per thread in two buffers that
were loaded while the block before was processed.  The crafted cases of test_gpu_ranked_kernel.py, test_gpu_ranked_rank8.py
and test_gpu_ranked_d12.py all run one block per workgroup (blocks_per_wg is sized for a whole GPU), so none of them
carries a buffer.  Here the tests-only knob ESGPU_DEBUG_BPW sets blocks_per_wg, and segments of a dozen blocks are
walked by one workgroup (12), by three (5), by six (2) and with the computed value (unset: one block each).

The blocks of a segment are of four kinds, named from the timestamps and asserted in every case:
  S  a full block inside one hour: the unrolled single-key body;
  M  a full block holding an hour boundary: the per-doc body, into the LDS window;
  X  a full block spanning more hours than the 8-key window: the per-doc body, docs past the window to the grid;
  P  the segment's last, partial block: the per-doc body with the tail mask.
The sequences hold every pair of neighbours -- S, M and X each followed by S, M, X and P -- and start with S, M and X.
Eligibility (zspan: the 90th percentile of the blocks' value ranges, below the interval) allows one X in twelve blocks,
so the sequences of 12 blocks hold one X each and X X stands in a sequence of 21 blocks.

Ranks and metric values are random, so a buffer that is stale, reloaded early or from the wrong block shows in the
counts, sums and extrema.  Every case collects with ranked_terms = 1 (rank8, and d12 where the metric spans < 4096),
= 3 (the 16-bit ranks) and = 2 (the generic kernel), each against the CPU oracle under helpers.assert_same, the shard
result and the reduced one; the three dicts are equal, all report path 10, the kernel is 1, 1 and 0, and the bytes the
kernel read tell the 12-bit form from the 16-bit one.  The four forms (stats or avg over a metric spanning less, or
not less, than 4096) times the two rank widths reach the kernel's six instantiations.
"""
import functools

import numpy as np
import pytest

import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import reduce
from helpers import assert_same
from test_gpu_layouts import layout
from test_gpu_ranked_kernel import BLOCK, HOUR, T0, eligible, request, shard

pytestmark = pytest.mark.gpu

STEP = 20  # ms between docs: a block spans 164 s
WINDOW = 8  # keys of the kernel's LDS window
SEQUENCES = {
    "starts_S": ("S M S S X S M M S S M P", 3001),
    "starts_M": ("M M X M S S S M S S S P", 4099),
    "starts_X": ("X S M S S M M S S S S P", 8191),
    "X_X_P": ("S M S S S S M S S S S S M S S S S S X X P", 5),
}
FORMS = {  # -> (stats leaf?, the metric's span)
    "d12": (True, 4095),
    "d16": (True, 29_999),
    "avg_d12": (False, 4095),
    "avg_d16": (False, 29_999),
}
OPTIONS = (1, 3, 2)
KERNEL = {1: 1, 3: 1, 2: 0}


def timestamps(kinds, tail):
    """sorted timestamps whose zone blocks are of the given kinds, the last one `tail` docs long"""
    rng = np.random.default_rng([len(kinds), tail])
    parts, t = [], T0 + 2 * HOUR + 1000
    for kind in kinds:
        n = tail if kind == "P" else BLOCK
        step = STEP
        if kind == "M":  # the next hour boundary a third of the way into the block
            first = -(-(t + n * STEP // 3) // HOUR) * HOUR
            t = first - n * STEP // 3
        elif kind == "X":
            step = (12 * HOUR) // BLOCK
        elif t // HOUR != (t + (n + 1) * STEP) // HOUR:  # S and P: inside one hour
            t = -(-t // HOUR) * HOUR + 1000
        ts = t + np.arange(n, dtype=np.int64) * step + rng.integers(0, step, size=n)
        parts.append(ts)
        t = int(ts[-1]) + STEP
    return np.concatenate(parts)


def kinds_of(ts):
    out = []
    for b in range(0, len(ts), BLOCK):
        k = ts[b:b + BLOCK] // HOUR
        span = int(k.max() - k.min())
        out.append("P" if len(k) < BLOCK else "S" if span == 0 else "M" if span == 1 else "X" if span >= WINDOW else "?")
    return out


@functools.lru_cache(maxsize=None)
def case(seq, form):
    """-> (columns, docs, request, the oracle's result): computed once per sequence and form, never modified"""
    text, tail = SEQUENCES[seq]
    kinds = text.split()
    stats, span = FORMS[form]
    ts = timestamps(kinds, tail)
    n = len(ts)
    assert kinds_of(ts) == kinds and n == (len(kinds) - 1) * BLOCK + tail
    assert eligible(ts), "the sequence must keep the ranked kernel"
    rng = np.random.default_rng([n, span, 7])
    ords = rng.integers(0, 40, size=n).astype(np.uint32)  # 25 of the 40 terms are collected
    ords[rng.random(n) < 0.03] = 0xFFFFFFFF
    rt = rng.integers(-7, -7 + span + 1, size=n)
    lo, hi = rng.choice(n, size=2, replace=False)
    rt[lo], rt[hi] = -7, -7 + span
    cols = shard(n, ords, 40, ts, rt=rt)
    aggs = request(leaf=None if stats else AB.avg("rt").field("rt"))
    return cols, n, aggs, O.run([(cols, n)], aggs)


def test_the_sequences_hold_every_pair_of_neighbours():
    pairs = set()
    for text, _ in SEQUENCES.values():
        kinds = text.split()
        pairs |= set(zip(kinds, kinds[1:]))
    assert pairs == {(a, b) for a in "SMX" for b in "SMXP"}
    assert {text[0] for text, _ in SEQUENCES.values()} == set("SMX")


@pytest.mark.parametrize("bpw", [12, 5, 2, None])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_block_carry(engine, monkeypatch, seq, form, bpw):
    cols, n, aggs, want = case(seq, form)
    if bpw is None:
        monkeypatch.delenv("ESGPU_DEBUG_BPW", raising=False)
    else:
        monkeypatch.setenv("ESGPU_DEBUG_BPW", str(bpw))
    d12 = FORMS[form][1] < 4096
    got = {}
    with layout(engine, "block"):
        seg = engine.upload_segment(cols, n)
        try:
            for option in OPTIONS:
                plan = engine.plan(aggs)
                try:
                    engine.set_option("ranked_terms", option)
                    try:
                        plan.collect(seg)
                    finally:
                        engine.set_option("ranked_terms", 1)
                    _, nbytes, path = plan.last_collect_stats()
                    assert path == 10, "option %d: path %d" % (option, path)
                    assert plan.last_collect_kernel() == KERNEL[option], "option %d: kernel" % option
                    narrower = {1: n + (n // 2 if d12 else 0), 3: 0, 2: 0}[option]
                    assert plan.last_collect_read_bytes() == nbytes - narrower, "option %d: the form that ran" % option
                    res = plan.build()
                    got[option] = (res.to_dict(), reduce([res]).to_dict())
                    assert_same(got[option][0], want["shards"][0], "option %d shard" % option)
                    assert_same(got[option][1], want["reduced"], "option %d reduced" % option)
                finally:
                    plan.close()
        finally:
            seg.close()
    assert got[1] == got[3] == got[2]
