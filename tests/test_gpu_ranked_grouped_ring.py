"""The grouped ranked kernel's ring of four prefixes (esgpu_ranked_grouped.hip): units, clamped loads, range ends.

A workgroup walks its zone blocks as units -- a (block, pass) pair: one unit for a block with n = off[K] <= 4096 (n = 0
included), two for a block with more -- and keeps four units in flight in four named slots, each refilled for the unit
four ahead.  Every lane issues every load: a lane with nothing to read loads group 0 of the same block (off[K] for the
offsets, the range's last block past its end) and ignores it.  The crafted cases of test_gpu_ranked_grouped.py run one
block per workgroup, so the ring is never carried there; here ESGPU_DEBUG_BPW sets the blocks per workgroup.

MIX is one segment of 23 blocks given as per-block count vectors over five terms whose ranks are their ordinals
(`crafted_block`), walked with 1 to 9, 13 and 24 blocks per workgroup: every residue of a range's units against the
ring's depth, so the clamped refills past a range's end happen in every slot.  It holds blocks with n = 0, 1, 7, 8,
4088, 4096, 4097, 4104 and 8192; a two-pass block directly before and directly after an n = 0 block; three two-pass
blocks in a row (the units outnumber the blocks); a two-key block (the per-doc body) in each of the four slots between
grouped blocks when one workgroup walks the segment (asserted from the unit sequence); and a partial last block.

Metric values (`sharpen`): every doc of rank 0 holds the column's minimum or its maximum, in turn, so group 0 of a block
-- what a lane with nothing to read loads -- holds delta 0 and delta 4095 (the order inside a group is the recode
kernel's; with eight or more docs of rank 0 the first group misses one of the two values with probability 2^-7 per block,
and the test then only checks less).  Every other rank's values lie strictly inside, so a lane that used its clamped
load for a doc of its own moves a bound of that rank, and its count.

Everything is compared as test_gpu_ranked_grouped.check does: options 5, 1 and 2 against the CPU oracle and each other,
the kernel ids, and the bytes read.
"""
import functools

import numpy as np
import pytest

import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from test_gpu_ranked_block_carry import kinds_of, timestamps
from test_gpu_ranked_d12 import SPAN, narrow
from test_gpu_ranked_grouped import MISSING, check, crafted_block, ranks_of
from test_gpu_ranked_kernel import BLOCK, HOUR, T0, eligible, request, shard, spaced

pytestmark = pytest.mark.gpu

PASS = 4096  # positions of a unit
DEPTH = 4  # slots of the ring
BASE = -2000

ONE = (1500, 1200, 800, 400, 100)  # n = 4000: one unit
TWO = (3000, 2400, 1500, 800, 400)  # n = 8100: two units
# (kind, counts): S a block inside one hour, M a block holding an hour boundary, P the partial last block
MIX = [
    ("S", ONE),
    ("M", ONE),
    ("S", ONE),
    ("S", ONE),
    ("M", ONE),
    ("S", TWO),
    ("S", (0, 0, 0, 0, 0)),  # n = 0 between two two-pass blocks
    ("S", (BLOCK, 0, 0, 0, 0)),  # n = 8192: every doc of rank 0
    ("S", TWO),
    ("S", (4000, 3000, 1000, 100, 50)),  # the third two-pass block in a row
    ("M", ONE),
    ("S", ONE),
    ("S", TWO),
    ("S", ONE),
    ("M", ONE),
    ("S", (2, 2, 1, 1, 1)),  # n = 7
    ("S", (4000, 80, 5, 2, 1)),  # n = 4088
    ("S", (4090, 3, 1, 1, 1)),  # n = 4096
    ("S", (4091, 3, 1, 1, 1)),  # n = 4097
    ("S", (4000, 100, 2, 1, 1)),  # n = 4104
    ("S", (1, 0, 0, 0, 0)),  # n = 1
    ("S", (3, 2, 1, 1, 1)),  # n = 8
    ("P", ONE),
]
TAIL = 5001  # docs of the partial block


def units_of(ns):
    """the unit index at which each block starts, and the number of units"""
    starts, u = [], 0
    for n in ns:
        starts.append(u)
        u += 2 if n > PASS else 1
    return starts, u


def sharpen(ords, rt, base):
    """rank 0 holds the column's bounds on every doc, in turn; every other doc a value strictly inside"""
    rt = np.clip(rt, base + 1, base + SPAN - 2)
    at = np.flatnonzero(ords == 0)
    rt[at[0::2]] = base
    rt[at[1::2]] = base + SPAN - 1
    return rt


def crafted(blocks, tail, seed, base=BASE):
    """-> ordinals, metric values and the per-block n = off[5] of the blocks' count vectors; the last block cut to `tail`"""
    rng = np.random.default_rng(seed)
    parts = [crafted_block(c, BLOCK - sum(c), rng, base) for c in blocks]
    ords = np.concatenate([p[0] for p in parts])[:(len(blocks) - 1) * BLOCK + tail]
    rt = np.concatenate([p[1] for p in parts])[:len(ords)]
    assert np.array_equal(ranks_of(ords, 5)[ords != MISSING], ords[ords != MISSING]), "ranks must be the ordinals"
    rt = sharpen(ords, rt, base)
    ns = [int(np.count_nonzero(ords[b:b + BLOCK] != MISSING)) for b in range(0, len(ords), BLOCK)]
    return ords, rt, ns


@functools.lru_cache(maxsize=None)
def mix(stats, size):
    """-> (columns, docs, request, the oracle's result): computed once per leaf and size, never modified"""
    kinds = [k for k, _ in MIX]
    ords, rt, ns = crafted([c for _, c in MIX], TAIL, 41)
    n = len(ords)
    ts = timestamps(kinds, TAIL)
    assert len(ts) == n and kinds_of(ts) == kinds and eligible(ts)
    assert (rt.min(), rt.max()) == (BASE, BASE + SPAN - 1)
    # what the segment was built to hold (size 5: every term is collected, n = the block's docs with a term)
    assert ns[:-1] == [sum(c) for _, c in MIX[:-1]] and 0 < ns[-1] <= PASS
    assert {0, 1, 7, 8, 4088, 4096, 4097, 4104, 8192} <= set(ns)
    two = [x > PASS for x in ns]
    assert any(two[i - 1] and ns[i] == 0 and two[i + 1] for i in range(1, len(ns) - 1))
    assert any(all(two[i:i + 3]) for i in range(len(ns) - 2))
    starts, total = units_of(ns)
    assert total > len(ns)
    # one workgroup over the segment: the two-key blocks stand in each of the ring's slots, between grouped blocks
    slots = {starts[i] % DEPTH for i, k in enumerate(kinds) if k == "M" and kinds[i - 1] == "S" and kinds[i + 1] == "S"}
    assert slots == set(range(DEPTH))
    cols = shard(n, ords.astype(np.uint32), 5, ts, rt=rt)
    aggs = request(size, leaf=None if stats else AB.avg("rt").field("rt"))
    return cols, n, aggs, O.run([(cols, n)], aggs)


def test_the_bpw_values_end_a_range_in_every_slot():
    """with 1 to 9 and 13 blocks per workgroup the ranges of MIX hold every residue of units against the ring's depth"""
    ns = [sum(c) for _, c in MIX[:-1]] + [TAIL]
    residues = set()
    for bpw in list(range(1, 10)) + [13]:
        for b in range(0, len(ns), bpw):
            residues.add(units_of(ns[b:b + bpw])[1] % DEPTH)
    assert residues == set(range(DEPTH))


@pytest.mark.parametrize("bpw", list(range(1, 10)) + [13, 24])
def test_range_ends_and_unit_mixes(engine, monkeypatch, bpw):
    cols, n, aggs, want = mix(True, 5)
    monkeypatch.setenv("ESGPU_DEBUG_BPW", str(bpw))
    check(engine, cols, n, aggs, 5, want=want)


@pytest.mark.parametrize("bpw", [3, 5, 24])
def test_avg_leaf(engine, monkeypatch, bpw):
    cols, n, aggs, want = mix(False, 5)
    monkeypatch.setenv("ESGPU_DEBUG_BPW", str(bpw))
    check(engine, cols, n, aggs, 5, want=want)


@pytest.mark.parametrize("bpw", [4, 24])
def test_three_of_five_ranks(engine, monkeypatch, bpw):
    """K = 3: the prefixes end inside the blocks' docs with a term, and the last collected rank is rank 2"""
    cols, n, aggs, want = mix(True, 3)
    monkeypatch.setenv("ESGPU_DEBUG_BPW", str(bpw))
    check(engine, cols, n, aggs, 3, want=want)


# ---- a range longer than the 64 blocks whose scalars a wave holds, one per lane ----
def test_range_of_more_than_64_blocks(engine, monkeypatch):
    """66 blocks inside one hour walked by one workgroup: the chunk of 64 ends behind a two-pass block and the next one
    starts with an n = 0 block; the segment has to be this long for the second chunk to exist"""
    blocks = [TWO if b % 5 == 3 else (0, 0, 0, 0, 0) if b % 7 == 1 else ONE for b in range(66)]
    assert blocks[63] == TWO and blocks[64] == (0, 0, 0, 0, 0)
    ords, rt, ns = crafted(blocks, 4099, 47)
    n = len(ords)
    ts = spaced(n, 5, T0 + HOUR + 60_000)
    assert eligible(ts) and ts[0] // HOUR == ts[-1] // HOUR
    monkeypatch.setenv("ESGPU_DEBUG_BPW", "70")
    check(engine, shard(n, ords.astype(np.uint32), 5, ts, rt=rt), n, request(5), 5)


# ---- the window slides and flushes while the ring is full ----
def hourly(n):
    """every block inside an hour of its own"""
    ts = np.concatenate([spaced(min(BLOCK, n - b), 20, T0 + (b // BLOCK) * HOUR + 60_000) for b in range(0, n, BLOCK)])
    assert eligible(ts) and ts[-1] // HOUR - ts[0] // HOUR == (n - 1) // BLOCK
    return ts


def test_sliding_window_one_rank(engine, monkeypatch):
    """K = 1 over 12 blocks, each in its own hour, 5 blocks per workgroup.  n is the block's count of rank 0: a block
    with no doc of rank 0 (but docs of other ranks) between two two-pass blocks, three two-pass blocks in a row, n = 4096
    and 4097, a block with no term at all in front of one with every doc of rank 0"""
    blocks = [ONE, (5000, 1200, 800, 400, 100), (0, 1500, 800, 400, 100), (4500, 1200, 800, 400, 100),
              (6000, 1000, 500, 300, 100), (4097, 2000, 0, 0, 0), ONE, (4096, 2, 1, 1, 1), TWO, (0, 0, 0, 0, 0),
              (BLOCK, 0, 0, 0, 0), ONE]
    ords, rt, _ = crafted(blocks, 777, 43)
    n = len(ords)
    n0 = [int(np.count_nonzero(ords[b:b + BLOCK] == 0)) for b in range(0, n, BLOCK)]
    two = [x > PASS for x in n0]
    assert n0[:-1] == [c[0] for c in blocks[:-1]] and {0, 4096, 4097, BLOCK} <= set(n0)
    assert any(two[i - 1] and n0[i] == 0 and two[i + 1] for i in range(1, len(n0) - 1))
    assert any(all(two[i:i + 3]) for i in range(len(n0) - 2))
    monkeypatch.setenv("ESGPU_DEBUG_BPW", "5")
    check(engine, shard(n, ords.astype(np.uint32), 5, hourly(n), rt=rt), n, request(1), 1)


def test_sliding_window_80_ranks(engine, monkeypatch):
    """K = 80 (size 10 of 8 shards) over 300 Zipf terms, offsets in both registers, each block in its own hour"""
    monkeypatch.setenv("ESGPU_G12_MAX_K", "128")
    monkeypatch.setenv("ESGPU_DEBUG_BPW", "5")
    n = 11 * BLOCK + 77
    ords = np.minimum(np.random.default_rng(3).zipf(1.2, size=n) - 1, 299)
    check(engine, shard(n, ords, 300, hourly(n), rt=narrow(n)), n, request(10), 80, shards=8)
