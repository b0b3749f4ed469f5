"""The mask-carry case tables (tests/mask_carry_cases.py) without a GPU: every block-to-block event of the key window of
collect path 13 and of the cells of paths 11 / 12 is shown to occur for some blocks-per-workgroup value of BPWS, from
the block table and the columns alone; the crafted columns are what the table says; every request builds and runs
through the oracle; and the inputs of the exact-sum cases meet the conditions under which the strict bar is neither
vacuous nor unreachable (no cancelling bucket, no overflow), checked with the oracle alone.

The window rule restated (mask_carry_cases.walk): a workgroup's cells stand for SLOTS consecutive grid rows from w0; a
block moves the window to its first row when w0 is unset, kmn < w0 or kmx >= w0 + SLOTS, flushing the cells if w0 was
set; a block without a key is skipped.
"""
import math

import numpy as np
import pytest

import filters_ref as FR
import mask_carry_cases as C
import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from helpers import bits_from_mask
from mask_carry_cases import BLOCK, BLOCKS, BPWS, HOUR, NB, NDOCS, ROWS, SLOTS, T0, TS


def _steps():
    """every (bpw, workgroup range, position, step) of the walk over BPWS, each with the step before and after it"""
    for bpw in BPWS:
        for blocks in C.ranges_of(bpw):
            steps = C.walk(blocks)
            for i, s in enumerate(steps):
                yield bpw, blocks, i, s, (steps[i - 1] if i else None), (steps[i + 1] if i + 1 < len(steps) else None)


def _single(s):
    return s is not None and s["kind"] == "single"


def test_bpws_give_every_range_shape():
    assert BPWS == (1, 2, 3, 4, 5, 13, 14) and NB == 13 and NDOCS == 12 * BLOCK + 5001
    lens = {bpw: [len(r) for r in C.ranges_of(bpw)] for bpw in BPWS}
    assert lens[13] == [13] and lens[14] == [13]                       # one workgroup exactly; a value above n_blocks
    assert all(lens[b][-1] < b for b in (2, 3, 4, 5))                   # a shorter last workgroup
    assert {n for ls in lens.values() for n in ls} >= {1, 2, 3, 4, 5}  # ranges of every small length
    for bpw in BPWS:
        assert sum(C.ranges_of(bpw), []) == list(range(NB))


def test_timestamps_are_what_the_block_table_says():
    ts, pres = C.timestamps()
    rows = (ts - T0) // HOUR
    for b, (kind, want) in enumerate(BLOCKS):
        sl = C.block_slice(b)
        got = np.unique(rows[sl][pres[sl]])
        assert got.tolist() == sorted(want), b
        assert (kind == "nokey") == (len(want) == 0) and (kind == "single") == (len(want) == 1)
        if kind == "shuffled":
            assert len(want) >= 300 and np.any(np.diff(rows[sl][pres[sl]]) < 0)
        p = pres[sl]
        if b in C.SPARSE_TS:
            words = p[:len(p) // 64 * 64].reshape(-1, 64)
            assert 0.3 < p.mean() < 0.9 and (~words.any(axis=1)).sum() >= 2 and words.all(axis=1).sum() == 0, b
        else:
            assert p.all() or not p.any(), b
    assert rows[pres].min() == 0 and rows[pres].max() == ROWS - 1  # the grid's rows are the table's: H = ROWS
    assert np.all(rows[~pres] >= ROWS)                             # what is stored under an absent doc lies outside
    assert BLOCKS[-1][0] == "multi" and C.block_slice(NB - 1).stop - C.block_slice(NB - 1).start == 5001
    assert not np.all(np.diff(ts[pres]) >= 0)                      # not globally sorted
    c = C.main_columns()[TS]
    assert np.array_equal(c["values"], ts) and np.array_equal(FR.mask_from_bits(c["present"], NDOCS), pres)


def test_every_window_event_occurs_for_some_bpw():
    seen = {}

    def note(ev, bpw):
        seen.setdefault(ev, set()).add(bpw)

    for bpw, blocks, i, s, prev, nxt in _steps():
        kind, rows, w0 = s["kind"], s["rows"], s["w0_before"]
        if kind == "nokey":
            if i == 0 and any(BLOCKS[b][0] != "nokey" for b in blocks):
                note("range begins with a nokey block", bpw)  # (and goes on to a block with keys: w0 unset until then)
            if all(BLOCKS[b][0] == "nokey" for b in blocks):
                note("range holds only nokey blocks", bpw)
                assert s["w0_after"] is None
            if prev and nxt and prev["w0_after"] is not None and not nxt["moved"] and nxt["w0_after"] == prev["w0_after"]:
                note("nokey block between two blocks that share a window", bpw)
            assert s["w0_after"] == w0 and not s["moved"]  # leaves the window alone
            continue
        kmn, kmx = min(rows), max(rows)
        if kind == "single" and _single(prev) and prev["rows"] == rows:
            assert not s["moved"]
            note("two consecutive single-key blocks of one row: no flush", bpw)
        if kind == "single" and w0 is not None and kmn == w0 + SLOTS - 1:
            assert not s["moved"]
            note("single-key block in the last slot: no flush", bpw)
        if kind == "single" and w0 is not None and kmn == w0 + SLOTS:
            assert s["flushed"] and s["w0_after"] == kmn
            note("single-key block at w0 + SLOTS: flush, window moves up", bpw)
        if w0 is not None and kmx < w0:
            assert s["flushed"] and s["w0_after"] == kmn
            note("block below the window: flush, window moves down", bpw)
        if kind == "multi" and 2 <= len(rows) <= 3 and w0 is not None and w0 + 1 <= kmn and kmx <= w0 + SLOTS - 1:
            assert not s["moved"] and i > 0
            note("multi-key block inside a window an earlier block opened: no move", bpw)
        if kind == "multi" and len(rows) == SLOTS and s["moved"]:
            assert s["to_grid"] == []
            note("multi-key block of exactly SLOTS rows fits after the move", bpw)
        if len(rows) > SLOTS:
            name = "shuffled block" if kind == "shuffled" else "block of SLOTS + 1 rows"
            assert s["moved"] and s["to_grid"] == sorted(rows)[SLOTS:]
            if kind == "multi":
                assert len(rows) == SLOTS + 1
            if s["flushed"] and _single(prev):
                note(name + " arrives with a single-key block's live cells", bpw)
            if _single(nxt) and kmn <= nxt["rows"][0] <= kmx and nxt["moved"] and nxt["flushed"]:
                note(name + " is followed by a single-key block in its span, outside its window", bpw)
            if s["flushed"] and _single(prev) and _single(nxt) and nxt["flushed"]:
                note(name + ": both in one range", bpw)
        if s["moved"] and kmn == ROWS - 2:
            assert s["w0_after"] + SLOTS > ROWS
            note("window opened at row H - 2: two slots stand for no row", bpw)
        if kmn == 0:
            note("block at row 0", bpw)
        if s["block"] == NB - 1 and kind == "multi":
            note("the partial last block is multi-key", bpw)
        if s["block"] in C.SPARSE_TS:
            note("sparse present bitset on a %s block" % kind, bpw)
    want = ["two consecutive single-key blocks of one row: no flush", "single-key block in the last slot: no flush",
            "single-key block at w0 + SLOTS: flush, window moves up", "block below the window: flush, window moves down",
            "multi-key block inside a window an earlier block opened: no move",
            "multi-key block of exactly SLOTS rows fits after the move",
            "block of SLOTS + 1 rows arrives with a single-key block's live cells",
            "block of SLOTS + 1 rows is followed by a single-key block in its span, outside its window",
            "block of SLOTS + 1 rows: both in one range",
            "shuffled block arrives with a single-key block's live cells",
            "shuffled block is followed by a single-key block in its span, outside its window", "shuffled block: both in one range",
            "nokey block between two blocks that share a window", "range begins with a nokey block",
            "range holds only nokey blocks", "sparse present bitset on a multi block", "sparse present bitset on a single block",
            "window opened at row H - 2: two slots stand for no row", "block at row 0", "the partial last block is multi-key"]
    assert sorted(seen) == sorted(want), sorted(set(want) ^ set(seen))
    # all of them need more than one block per workgroup, but for those a lone block shows
    alone = {"range holds only nokey blocks", "block at row 0", "the partial last block is multi-key",
             "sparse present bitset on a multi block", "sparse present bitset on a single block",
             "window opened at row H - 2: two slots stand for no row", "multi-key block of exactly SLOTS rows fits after the move"}
    for ev, bpws in seen.items():
        assert (1 in bpws) == (ev in alone), (ev, sorted(bpws))
        assert 13 in bpws or "nokey block" in ev, ev  # the one-workgroup walk shows everything but a range's own shape


def _bucket(keys, key):
    return keys.index(key)


def test_sixty_four_buckets_first_block_last_block_and_extrema():
    cols = C.main_columns()
    for case in [c for c in C.carry_cases() if c.name in ("range_64_stats", "filters_63_other_stats")]:
        keys, masks = case.masks(cols, NDOCS)
        assert len(keys) == 64 and masks[63].sum() > 0                # bit 63 is used
        blocks_of = [sorted(set((np.nonzero(m)[0] // BLOCK).tolist())) for m in masks]
        assert all(len(b) >= 1 for b in blocks_of)
        m = cols["m"]["values"]
        for bpw in (2, 3, 4, 5, 13):
            rs = [r for r in C.ranges_of(bpw) if len(r) > 1]
            # a bucket with docs only in the first block of a workgroup's range, one only in the last
            assert any(bl == [r[0]] for bl in blocks_of for r in rs), (case.name, bpw)
            assert any(bl == [r[-1]] for bl in blocks_of for r in rs), (case.name, bpw)
        # a bucket over the whole segment: its minimum in the first block of the one-workgroup range, its maximum in the last
        wide = max(range(64), key=lambda b: len(blocks_of[b]))
        assert blocks_of[wide] == list(range(NB))
        v = np.where(masks[wide], m, m[masks[wide]][0])
        assert int(v.argmin()) // BLOCK == 0 and int(v.argmax()) // BLOCK == NB - 1, case.name
        assert v.min() == -5 and v.max() == 10_000_000


def test_sparse_metric_leaves_a_bucket_with_docs_and_no_value_in_a_whole_block():
    cols = C.main_columns()
    pres = FR.mask_from_bits(cols["sz"]["present"], NDOCS)
    assert not pres[C.block_slice(7)].any() and 0.4 < pres.mean() < 0.5
    assert not pres[2 * BLOCK + 128:2 * BLOCK + 192].any()  # a whole bitset word
    for case in [c for c in C.carry_cases() if "sparse_metric" in c.name]:
        _keys, masks = case.masks(cols, NDOCS)
        assert sum(1 for m in masks if m[C.block_slice(7)].sum() > 100) >= 3, case.name  # docs of several buckets there
        assert any(m.sum() > 0 and (m & pres).sum() > 0 for m in masks)


def test_every_carry_case_builds_and_runs_through_the_oracle():
    names = set()
    for case in C.carry_cases():
        assert case.name not in names and set(case.bpws) <= set(BPWS) and max(case.bpws) > 1
        names.add(case.name)
        ref = C.reference(case, C.main_segs())
        assert len(ref["keys"]) == len(ref["counts"]) == len(ref["want"])
        assert sum(ref["counts"]) > 0 and case.root().name == case.agg_name
        if case.query:
            _k, masks = case.masks(C.main_columns(), NDOCS)
            assert all(c < int(m.sum()) for c, m in zip(ref["counts"], masks) if m.sum())
        if case.path == 13 and case.kids()[0].subs:  # every row of the table is a histogram key of some bucket
            keys = {b["key"] for w in ref["want"] for b in w["reduced"]["h"]["buckets"] if b["doc_count"]}
            assert keys == {T0 + r * HOUR for _k, rows in BLOCKS for r in rows}, case.name
    # both orders of the two-segment plan
    tail = ("tail",) + C.tail_columns()
    case = C.carry_cases()[0]
    a, b = C.reference(case, C.main_segs() + [tail]), C.reference(case, [tail] + C.main_segs())
    assert a["counts"] == b["counts"] and a["counts"] != C.reference(case, C.main_segs())["counts"]
    rows = (tail[1][TS]["values"] - T0) // HOUR
    assert rows.min() >= ROWS and tail[2] == BLOCK + 300  # the grid grows above the main segment's rows: 2 blocks


def test_compare_accepts_the_reference_and_refuses_one_moved_doc():
    """mask_carry_cases.compare on the oracle's own results put together as the GPU renders them, then with one doc of
    one histogram bucket moved to its neighbour (what a cell flushed to the wrong row looks like)"""
    import copy
    from helpers import strip_exact
    case = next(c for c in C.carry_cases() if c.name == "range_hist_stats")
    ref = C.reference(case, C.main_segs())

    def rendered(which):
        out = {"buckets": []}
        for key, dc, want in zip(ref["keys"], ref["counts"], ref["want"]):
            w = want["reduced"] if which == "reduced" else want["shards"][0]
            out["buckets"].append(dict({"key": key, "doc_count": dc}, **strip_exact(copy.deepcopy(w))))
        return out

    shard, red = rendered("shard"), rendered("reduced")
    C.compare(case, ref, shard, red, 1)
    for which in (shard, red):
        bad = copy.deepcopy(which)
        hb = [b for b in bad["buckets"][0]["h"]["buckets"] if b["doc_count"]]
        hb[1]["doc_count"] -= 1
        hb[2]["doc_count"] += 1
        with pytest.raises(AssertionError):
            C.compare(case, ref, *((bad, red) if which is shard else (shard, bad)), 1)
        bad = copy.deepcopy(which)
        hb = [b for b in bad["buckets"][1]["h"]["buckets"] if b["doc_count"]]
        hb[3]["s"]["sum"] += 1.0
        with pytest.raises(AssertionError):
            C.compare(case, ref, *((bad, red) if which is shard else (shard, bad)), 1)
    bad = copy.deepcopy(red)
    bad["buckets"][2]["doc_count"] += 1
    with pytest.raises(AssertionError):
        C.compare(case, ref, shard, bad, 1)


def test_parts_of_an_extended_stats_leaf_partition_it():
    """plain, squares and derived (mask_carry_cases.PARTS) share no value and leave none out, in the rendered leaf, its
    _internal and its _exact; everything around the leaf stays"""
    case = C.exact_cases("big", True)[2]
    tree = C.reference(case, C.main_segs())["want"][0]["reduced"]
    leaf = next(b for b in tree["h"]["buckets"] if b["doc_count"])["x"]
    assert {"variance", "sum_of_squares", "sum", "_internal", "_exact"} <= set(leaf)
    cut = {p: next(b for b in C.part_of(tree, p)["h"]["buckets"] if b["doc_count"])["x"] for p in C.PARTS}
    for sub in (lambda d: d, lambda d: d["_internal"], lambda d: d["_exact"], lambda d: d["_exact"]["_internal"]):
        keys = [set(sub(cut[p])) - {"_internal", "_exact"} for p in C.PARTS]
        assert set.union(*keys) == set(sub(leaf)) - {"_internal", "_exact"} and sum(map(len, keys)) == len(set.union(*keys))
    assert set(cut["derived"]) - {"_internal", "_exact"} == C.DERIVED and set(cut["squares"]["_internal"]) == C.SQUARES
    assert {"count", "min", "max", "avg", "sum"} <= set(cut["plain"])
    for p in C.PARTS:
        got = C.part_of(tree, p)["h"]["buckets"]
        assert [(b["key"], b["doc_count"]) for b in got] == [(b["key"], b["doc_count"]) for b in tree["h"]["buckets"]]
    assert C.part_of(tree, None) is tree
    stats = C.reference(C.exact_cases("big", True)[1], C.main_segs())["want"][0]["reduced"]
    assert C.part_of(stats, "derived") == stats  # a stats leaf has no part


# ---- the exact-sum cases' inputs -------------------------------------------------------------------------------------------
def _leaves(tree, out):
    """every stats-like leaf (its _internal and _exact values) of an oracle result"""
    if isinstance(tree, dict):
        if "_internal" in tree and "_exact" in tree:
            out.append(tree)
            return
        for v in tree.values():
            _leaves(v, out)
    elif isinstance(tree, list):
        for v in tree:
            _leaves(v, out)


def _abs_columns(segs, field):
    """the segments with |field| beside it (what the oracle sums for the bound on cancellation)"""
    out = []
    for _nm, c, n in segs:
        c = dict(c)
        v = c[field]["values"]
        c["abs"] = dict(c[field], values=np.abs(v))
        out.append((c, n))
    return out


def _check_no_cancelling_bucket(case, segs):
    """every finite, non-empty cell of the request: |exact sum| >= 1e-3 * sum |x| -- the sums the oracle itself makes"""
    field = case.metric
    per = [case.masks(c, n) for _nm, c, n in segs]
    mk = lambda f: [AB.stats("s").field(f)]  # noqa: E731
    kids = (lambda f: [C.dh(mk(f))]) if case.path == 13 else mk
    cells = 0
    for b in range(len(per[0][0])):
        acc = [bits_from_mask(per[s][1][b]) for s in range(len(segs))]
        sums, abss = [], []
        _leaves(O.run(_abs_columns(segs, field), kids(field), accept=acc, exact=True)["reduced"], sums)
        _leaves(O.run(_abs_columns(segs, field), kids("abs"), accept=acc, exact=True)["reduced"], abss)
        assert len(sums) == len(abss)
        for s, a in zip(sums, abss):
            n, tot, ex = s["_internal"]["count"], a["_exact"]["_internal"]["sum"], s["_exact"]["_internal"]["sum"]
            assert n == a["_internal"]["count"]
            if n == 0 or not math.isfinite(tot):
                continue
            cells += 1
            assert abs(ex) >= 1e-3 * tot, (case.name, b, n, ex, tot)
    return cells


@pytest.mark.parametrize("field,exact", C.EXACT_COLUMNS)
def test_exact_inputs_do_not_cancel_or_overflow(field, exact):
    cols = C.main_columns()
    v = cols[field]["values"].astype(np.float64)
    fin = np.isfinite(v)
    assert np.abs(v[fin]).max() ** 2 * NDOCS < 1e308  # no order of additions overflows, the sums of squares included
    cases = C.exact_cases(field, exact)
    assert [c.path for c in cases] == [11, 12, 13, 13] and all(c.strict and c.bpws == (1, 5) for c in cases)
    for case in cases:
        ref = C.reference(case, C.main_segs())
        assert sum(ref["counts"]) > 0
    # the histogram under the filters holds every cell of the other three requests' buckets or a finer one
    assert _check_no_cancelling_bucket(cases[2], C.main_segs()) > 1000
    assert _check_no_cancelling_bucket(cases[3], C.main_segs()) > 800
    assert _check_no_cancelling_bucket(cases[0], C.main_segs()) >= (4 if fin.all() else 1)  # (finite cells only)
    if field == "big":       # the integer rule turns the compensated sums on: n * max |v| >= 2^53
        assert NDOCS * int(cols[field]["values"].max()) >= 2 ** 53
        tops = []
        _leaves(C.reference(cases[0], C.main_segs())["want"], tops)
        assert max(t["_internal"]["sum"] for t in tops) > 2.0 ** 53
    if field == "bytes":     # the sums stay below 2^53, the sums of squares pass it
        tops = []
        _leaves(C.reference(cases[0], C.main_segs())["want"], tops)
        assert max(t["_internal"]["sum"] for t in tops) < 2.0 ** 53 < max(t["_internal"]["sum_of_squares"] for t in tops)
    if field == "sp_mixed":  # -0.0 against 0.0 alone in the tail buckets
        tail = cols[C.RT]["values"] >= C.TAIL_LO
        assert tail.sum() > 100 and np.all(v[tail] == 0.0) and np.signbit(v[tail]).any() and not np.signbit(v[tail]).all()
        keys, _m = cases[0].masks(cols, NDOCS)
        x = C.reference(cases[0], C.main_segs())["want"][keys.index("tail")]["reduced"]["x"]["_internal"]
        assert math.copysign(1.0, x["min"]) == -1.0 and math.copysign(1.0, x["max"]) == 1.0 and x["min"] == 0.0 == x["max"]


def test_plan_level_inputs():
    big, small = ("big",) + C.v_columns("big"), ("small",) + C.v_columns("small")
    # the rule (n * a >= 2^53 over the plan's docs so far) is off after the small segment and on with the large one
    assert small[2] * int(np.abs(small[1]["v"]["values"]).max()) < 2 ** 53
    assert small[2] <= 2 * BLOCK and big[2] == NDOCS
    assert (small[2] + big[2]) * int(big[1]["v"]["values"].max()) >= 2 ** 53
    for case in C.plan_cases():
        for segs in ([small, big], [big, small], [small]):
            assert sum(C.reference(case, segs)["counts"]) > 0
            assert _check_no_cancelling_bucket(case, segs) >= 4
