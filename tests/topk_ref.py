"""Crafted count vectors for the GPU selection routines, and a numpy reference of the selection (no product code).

A terms result passes through a selection: which ordinals win, in what order, what goes to sum_other_doc_count.  Random
Zipf or uniform columns do not put two different counts into one histogram sub-bin at the k-th position, a tie at the cut
over tens of thousands of ordinals, or a tied pair into one lane's share of a row; a count vector written by hand does,
and a count vector is an ordinal column: np.repeat(arange(T), counts), shuffled.

  column / grid_column   count vector (matrix) -> the column dict of Engine.upload_segment / oracle.run
  select                 GlobalOrdinalsStringTermsAggregator.buildAggregation:146-208, vectorised
  count_bin              the device function of the count orders' histogram, restated: proves preconditions only
  VECTORS / CASES        the case table: name -> vector, requests, the branch it is meant to reach

The constants below restate the kernels' (tests/test_topk_cases_host.py compares them with the source text).
"""
import functools

import numpy as np

COL_ORD_U32, COL_I64 = 1, 2  # include/esgpu.h ESGPU_COL_* (asserted against elasticsearch_amd._native on the host test)
COUNT_DESC, COUNT_ASC, TERM_ASC, TERM_DESC = 0, 1, 2, 3  # ESGPU_ORDER_*
ORDER_NAMES = {COUNT_DESC: "count_desc", COUNT_ASC: "count_asc", TERM_ASC: "term_asc", TERM_DESC: "term_desc"}

TOPK_MAX = 1024        # kTopkMax: the largest k of launch_topk's final sort
ROW_TOPK_MAX = 1024    # kRowTopkMax
ROW_LDS_KEYS = 4096    # kRowTopkLdsKeys: a row's keys sit in LDS up to here
TOPK_CHUNK = 4096      # kTopkChunk: keys per bitonic sort
TOPK_BINS = 2048       # kTopkBins
COLO_SEL_MAX = 4096    # kColoSelMax
GPU_TOPK_ABOVE = 65536  # build_terms_root: value_count > 65536
HOT_MAX = 16384        # ESGPU_HOT_MAX: no hot set is larger
MISSING = 0xFFFFFFFF

T_TAIL1, T_TAIL3, T_NOTAIL = 65_537, 65_539, 69_632  # T % 4 = 1, 3, 0: load_counts4's scalar tail
HOUR = 3_600_000
T0 = 1_441_065_600_000  # an hour-aligned timestamp


def terms_of(T):
    return ["u%07d" % i for i in range(T)]


def column(counts, missing=0, seed=1, rejected=None):
    """(columns, docs, accept mask or None): ordinal t in counts[t] docs (+ rejected[t] docs the mask rejects), `missing`
    docs without an ordinal, shuffled; "v" a long field for a metric child"""
    counts = np.asarray(counts, dtype=np.int64)
    T = len(counts)
    parts = [np.repeat(np.arange(T, dtype=np.uint32), counts), np.full(missing, MISSING, dtype=np.uint32)]
    mask = [np.ones(len(parts[0]) + missing, dtype=bool)]
    if rejected is not None:
        parts.append(np.repeat(np.arange(T, dtype=np.uint32), np.asarray(rejected, dtype=np.int64)))
        mask.append(np.zeros(len(parts[-1]), dtype=bool))
    ords, mask = np.concatenate(parts), np.concatenate(mask)
    perm = np.random.default_rng(seed).permutation(len(ords))
    ords, mask = ords[perm], mask[perm]
    cols = {"kw": {"type": COL_ORD_U32, "values": ords, "terms": terms_of(T)},
            "v": {"type": COL_I64, "values": (np.arange(len(ords), dtype=np.int64) * 7) % 1000}}
    return cols, len(ords), (mask if rejected is not None else None)


def grid_column(matrix, row_values, row_field, missing=None, seed=1):
    """the per-row variant: counts[r][t] docs with ordinal t and row value row_values[r] in `row_field` (an hour-aligned
    timestamp for a date_histogram, an outer ordinal for terms under terms); missing[r] docs of row r have no ordinal"""
    matrix = np.asarray(matrix, dtype=np.int64)
    R, T = matrix.shape
    missing = [0] * R if missing is None else missing
    ords, rows = [], []
    for r in range(R):
        o = np.concatenate([np.repeat(np.arange(T, dtype=np.uint32), matrix[r]), np.full(missing[r], MISSING, dtype=np.uint32)])
        ords.append(o)
        rows.append(np.full(len(o), r, dtype=np.int64))
    ords, rows = np.concatenate(ords), np.concatenate(rows)
    perm = np.random.default_rng(seed).permutation(len(ords))
    ords, rows = ords[perm], rows[perm]
    cols = {"kw": {"type": COL_ORD_U32, "values": ords, "terms": terms_of(T)}}
    if row_field == "@timestamp":
        jitter = (np.arange(len(ords), dtype=np.int64) * 7919) % HOUR
        cols[row_field] = {"type": COL_I64, "values": np.asarray(row_values, dtype=np.int64)[rows] + jitter}
    else:
        cols[row_field] = {"type": COL_ORD_U32, "values": rows.astype(np.uint32),
                           "terms": ["a%04d" % i for i in range(len(row_values))]}
    cols["v"] = {"type": COL_I64, "values": (np.arange(len(ords), dtype=np.int64) * 7) % 1000}
    return cols, len(ords)


def select(counts, order, size, min_doc_count=1, shard_min_doc_count=0):
    """(ordinals, counts, other) of one owning bucket -- GlobalOrdinalsStringTermsAggregator.buildAggregation:146-208:
    an ordinal is skipped when min_doc_count > 0 and its count is 0 (:168-170); every other ordinal's count goes to
    otherDocCount (:171) and it is a candidate when shard_min_doc_count <= count (:175); the queue keeps the best
    min(size, candidates) by the order's comparator with the ordinal ascending as tie-break (InternalOrder: _count
    compares counts, then the term ascending; _term desc: the ordinal descending), and the picks' counts leave
    otherDocCount (:193)."""
    c = np.asarray(counts, dtype=np.int64)
    elig = c >= shard_min_doc_count
    if min_doc_count > 0:
        elig &= c > 0
    cand = np.nonzero(elig)[0]
    cc = c[cand]
    if order == COUNT_DESC:
        idx = np.lexsort((cand, -cc))
    elif order == COUNT_ASC:
        idx = np.lexsort((cand, cc))
    elif order == TERM_ASC:
        idx = np.arange(len(cand))
    else:
        idx = np.arange(len(cand))[::-1]
    picks = cand[idx][:max(int(size), 0)]
    return picks, c[picks], int(c.sum() - c[picks].sum())


def count_bin(order, c):
    """the device function count_bin (esgpu_kernels.hip): 32 sub-bins per octave, reversed for _count asc"""
    c = int(c)
    if c < 32:
        b = c
    else:
        e = c.bit_length() - 1
        b = (e - 4) * 32 + ((c >> (e - 5)) & 31)
    b = min(b, TOPK_BINS - 1)
    return b if order == COUNT_DESC else TOPK_BINS - 1 - b


def n_wg(T):
    return min(512, -(-T // TOPK_CHUNK))


def per_wg(T):
    return -(-T // n_wg(T))


def threshold_candidates(counts, order, k, min_doc_count=1, shard_min_doc_count=0):
    """how many candidates topk_compact_kernel appends: the eligible ordinals in bins >= the highest bin whose suffix
    holds k (all of them when fewer than k are eligible)"""
    c = np.asarray(counts, dtype=np.int64)
    elig = c >= shard_min_doc_count
    if min_doc_count > 0:
        elig &= c > 0
    vals, reps = np.unique(c[elig], return_counts=True)
    bins = np.array([count_bin(order, v) for v in vals], dtype=np.int64)
    hist = np.bincount(bins, weights=reps, minlength=TOPK_BINS).astype(np.int64)
    suffix = np.cumsum(hist[::-1])[::-1]
    ok = np.nonzero(suffix >= k)[0]
    tb = int(ok[-1]) if len(ok) else 0
    return int(suffix[tb]), tb


# ---- vectors ---------------------------------------------------------------------------------------------------------
def _scatter(T, n, salt=0):
    """n distinct ordinals spread over [0, T), in no order of their index"""
    step = T // (n + 1)
    return np.array([(1 + ((i * 7 + salt) % n)) * step + (i % 3) for i in range(n)], dtype=np.int64)


def v_all_equal(T):
    return np.full(T, 2, dtype=np.int64)


def v_shared_subbin(T):
    """1000 .. 1015 on scattered ordinals (512 .. 1023 has sub-bins of 16: 992 .. 1007 and 1008 .. 1023), the rest 1"""
    c = np.ones(T, dtype=np.int64)
    c[_scatter(T, 16)] = 1000 + np.arange(16)
    return c


def v_one_subbin(T):
    """2048 .. 2063 on scattered ordinals (2048 .. 4095 has sub-bins of 64: one sub-bin), the rest 1"""
    c = np.ones(T, dtype=np.int64)
    c[_scatter(T, 16, 5)] = 2048 + np.arange(16)
    return c


SEAMS = (31, 32, 33, 63, 64, 65, 127, 128, 129)


def v_octave_seams(T):
    c = np.ones(T, dtype=np.int64)
    c[_scatter(T, 9, 2)] = SEAMS
    return c


def tie_ordinals(T):
    return [0, 4095, 4096, T // 2, T - 1]


def v_tie_at_cut(T):
    """three ordinals above (100, 90, 80), then a 5-way tie at 50 on ordinals 0, 4095, 4096, T / 2, T - 1; the rest 1"""
    c = np.ones(T, dtype=np.int64)
    c[[7, 5000, 60000]] = (100, 90, 80)
    c[tie_ordinals(T)] = 50
    return c


FEW = (9, 70, 4097, 40000, 65536)


def v_too_few(T):
    """five ordinals with docs, the rest 0"""
    c = np.zeros(T, dtype=np.int64)
    c[list(FEW)] = (3, 5, 5, 1, 2)
    return c


def v_shard_min(T):
    """counts 1 and 2 alternating (not candidates under shard_min_doc_count 3, but counted in other), 20 ordinals 3 .. 22"""
    c = 1 + (np.arange(T, dtype=np.int64) & 1)
    c[_scatter(T, 20, 3)] = 3 + np.arange(20)
    return c


def v_tail_winner(T):
    c = np.ones(T, dtype=np.int64)
    c[[T - 1, T - 2, T - 3, T - 4, T - 5]] = (500, 400, 400, 300, 2)
    return c


def v_levels(T):
    """1,100 scattered ordinals with counts 2 + i % 97 (ties at every level), the rest 1: the cut of sizes 1023 .. 1025
    falls inside a tie"""
    c = np.ones(T, dtype=np.int64)
    c[_scatter(T, 1100, 11)] = 2 + np.arange(1100) % 97
    return c


def v_every_4099(T):
    """count 2 on every 4,099th ordinal and on T - 1, count 1 on the ordinal after each, the rest 0"""
    c = np.zeros(T, dtype=np.int64)
    c[np.arange(1, T, 4099)] = 1
    c[np.arange(0, T, 4099)] = 2
    c[T - 1] = 2
    return c


def v_one_workgroup(T):
    """1,100 ordinals with docs, all inside the second workgroup's range: per_wg + 3 i"""
    c = np.zeros(T, dtype=np.int64)
    c[per_wg(T) + 3 * np.arange(1100)] = 1 + np.arange(1100) % 3
    return c


def v_settled(T):
    """ten high ordinals 3 .. 12, every other ordinal 2: the 10th pick is exactly one above every other count"""
    c = np.full(T, 2, dtype=np.int64)
    c[T - 1 - 100 * np.arange(10)] = 3 + np.arange(10)
    return c


def v_cold_tie(T):
    """five high ordinals 10 .. 14, every other ordinal 1: the picks after them tie with > 60,000 ordinals"""
    c = np.ones(T, dtype=np.int64)
    c[T - 1 - 100 * np.arange(5)] = 10 + np.arange(5)
    return c


COLD_X = 20_000


def v_cold_winner(T):
    """(accepted, rejected) counts.  The segment's counts (accepted + rejected): ordinals 0 .. 19,999 and X = 20,000
    have 2, 30,000 .. 30,009 have 3, five high ordinals 10 .. 14, the rest 1.  More than HOT_MAX ordinals at 2 lie below
    X, so X is cold in every hot set, and every ordinal above 2 is hot when the hot set holds 15: max_cold = 2.  The
    accept bits keep one doc of 0 .. 19,999 and two of 30,000 .. 30,009: the request's 10 winners are the five high
    ordinals, X, and 30,000 .. 30,003 -- the hot slots' 10th count equals max_cold, and the cold X wins that tie."""
    acc = np.ones(T, dtype=np.int64)
    rej = np.zeros(T, dtype=np.int64)
    rej[:COLD_X] = 1
    acc[COLD_X] = 2
    acc[30_000:30_010] = 2
    rej[30_000:30_010] = 1
    acc[T - 1 - 100 * np.arange(5)] = 10 + np.arange(5)
    return acc, rej


def v_cold_tie_accept(T):
    """(accepted, rejected): v_cold_tie accepted.  The segment has a second, rejected doc of ordinals 1,000 .. 20,999:
    more than HOT_MAX ordinals above count 1, so every hot ordinal has 2 docs or more and 0 .. 4 (one doc) are cold --
    and they are the request's picks 6 .. 10, tied at count 1 with > 60,000 ordinals"""
    rej = np.zeros(T, dtype=np.int64)
    rej[1_000:21_000] = 1
    return v_cold_tie(T), rej


def v_settled_accept(T):
    """v_settled accepted; rejected: one more doc of every 64th ordinal"""
    rej = np.zeros(T, dtype=np.int64)
    rej[::64] = 1
    return v_settled(T), rej


VECTORS = {
    "all_equal": v_all_equal, "shared_subbin": v_shared_subbin, "one_subbin": v_one_subbin, "octave_seams": v_octave_seams,
    "tie_at_cut": v_tie_at_cut, "too_few": v_too_few, "shard_min": v_shard_min, "tail_winner": v_tail_winner,
    "levels": v_levels, "every_4099": v_every_4099, "one_workgroup": v_one_workgroup, "settled": v_settled,
    "cold_tie": v_cold_tie, "cold_winner": v_cold_winner, "settled_accept": v_settled_accept,
    "cold_tie_accept": v_cold_tie_accept,
}


@functools.lru_cache(maxsize=None)
def vector(name, T):
    """the accepted counts of a vector (what a request counts), read-only"""
    v = VECTORS[name](T)
    v = v[0] if isinstance(v, tuple) else v
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=4)
def segment(name, T):
    """(columns, docs, accept mask or None) of a vector; 1,000 docs without an ordinal"""
    v = VECTORS[name](T)
    if isinstance(v, tuple):
        return column(v[0], missing=1000, seed=T % 1000, rejected=v[1])
    return column(v, missing=1000, seed=T % 1000)


def req(order, size, mdc=1, smdc=0):
    """(order, size = shard_size, min_doc_count, shard_min_doc_count); a shard_min_doc_count above min_doc_count would be
    lowered to it (TermsAggregator.BucketCountThresholds.ensureValidity), so min_doc_count is raised with it here"""
    return (order, size, max(mdc, smdc), smdc)


def _sizes(order, sizes, mdc=1, smdc=0):
    return [req(order, s, mdc, smdc) for s in sizes]


# name -> (group, vector, T, mode, requests, branch); mode: "lone" (one terms aggregation), "beside" (a second terms
# aggregation in the request: the cold lists are not deferred), "stats" (a stats child on a long field: 64-bit counts),
# "accept" (lone, under the vector's accept bits)
CASES = {}


def _case(name, group, vec, T, mode, requests, branch):
    CASES[name] = dict(group=group, vector=vec, T=T, mode=mode, requests=requests, branch=branch)


for _T in (T_TAIL1, T_TAIL3, T_NOTAIL):
    _case("a_all_equal_%d" % _T, "a", "all_equal", _T, "beside", _sizes(COUNT_DESC, (1, 10, 1024)),
          "every ordinal a candidate: %d chunks in topk_final_kernel; T %% 4 = %d" % (-(-_T // TOPK_CHUNK), _T % 4))
    _case("a_tail_winner_%d" % _T, "a", "tail_winner", _T, "beside", _sizes(COUNT_DESC, (1, 3, 4)),
          "the winner at T - 1: load_counts4's scalar tail (T %% 4 = %d)" % (_T % 4))
_case("a_all_equal_lone", "a", "all_equal", T_TAIL1, "lone", _sizes(COUNT_DESC, (1, 10, 1024)),
      "the same through the deferred path's gate (hot k-th count = max_cold)")
_case("a_shared_subbin", "a", "shared_subbin", T_TAIL1, "beside", _sizes(COUNT_DESC, range(1, 17)),
      "the cut between two counts of one sub-bin of 16 (and once between two sub-bins, 1007 | 1008)")
_case("a_one_subbin", "a", "one_subbin", T_TAIL1, "beside", _sizes(COUNT_DESC, range(1, 17)),
      "the cut between two counts of one sub-bin of 64")
_case("a_shared_subbin_lone", "a", "shared_subbin", T_TAIL1, "lone", _sizes(COUNT_DESC, (3, 8, 9, 16)),
      "the same through launch_topk with ord_of (the hot slots' top-k)")
_case("a_octave_seams", "a", "octave_seams", T_TAIL1, "beside", _sizes(COUNT_DESC, range(1, 10)),
      "31 | 32 | 33, 63 | 64 | 65, 127 | 128 | 129: the last exact bin, the first sub-bins, two octave seams")
_case("a_tie_at_cut", "a", "tie_at_cut", T_TAIL1, "beside", _sizes(COUNT_DESC, range(3, 9)),
      "a 5-way tie at the cut over two 4096-chunks' seam (4095 | 4096), T / 2 and T - 1")
_case("a_too_few", "a", "too_few", T_TAIL1, "beside", _sizes(COUNT_DESC, (10,)) + _sizes(COUNT_DESC, (10, 5, 4), mdc=0),
      "fewer eligible ordinals than size (threshold bin 0); min_doc_count 0: zeros fill in by ascending ordinal")
_case("a_shard_min", "a", "shard_min", T_TAIL1, "beside", _sizes(COUNT_DESC, (10, 30), smdc=3),
      "shard_min_doc_count 3: 65,517 ordinals at 1 and 2 are no candidates but count in other")
_case("a_gate_1024", "a", "levels", T_TAIL1, "beside", _sizes(COUNT_DESC, (1023, 1024, 1025)),
      "k = 1023 (not a power of two), 1024 (kTopkMax), 1025 (host selection): equal prefixes")

_case("b_all_equal", "b", "all_equal", T_TAIL3, "beside", _sizes(COUNT_ASC, (1, 10, 1024)), "count asc, every ordinal tied")
_case("b_tie_on_one", "b", "tie_at_cut", T_TAIL1, "beside", _sizes(COUNT_ASC, (1, 7, 1000)),
      "count asc, min_doc_count 1: a tie on count 1 over > 60,000 ordinals (16 chunks of candidates)")
_case("b_zeros_first", "b", "too_few", T_TAIL1, "beside", _sizes(COUNT_ASC, (10, 1024), mdc=0) + _sizes(COUNT_ASC, (3, 10)),
      "count asc, min_doc_count 0: zeros first; min_doc_count 1: the five ordinals with docs")
_case("b_shared_subbin", "b", "shared_subbin", T_TAIL1, "beside", _sizes(COUNT_ASC, range(1, 17), smdc=2),
      "the sub-bin cuts from the small end (the count-1 ordinals kept out by shard_min_doc_count 2)")
_case("b_one_subbin", "b", "one_subbin", T_TAIL1, "beside", _sizes(COUNT_ASC, range(1, 17), smdc=2), "the same, one sub-bin of 64")
_case("b_octave_seams", "b", "octave_seams", T_TAIL1, "beside", _sizes(COUNT_ASC, range(1, 10), smdc=2),
      "the octave seams from the small end")
_case("b_gate_1024", "b", "levels", T_TAIL1, "beside", _sizes(COUNT_ASC, (1023, 1024, 1025), smdc=2),
      "count asc across the 1024 gate")

_TERM_SIZES = (1, 16, 17, 1000, 1024)
for _o in (TERM_ASC, TERM_DESC):
    _n = ORDER_NAMES[_o]
    _case("c_every_4099_%s" % _n, "c", "every_4099", T_NOTAIL, "beside",
          _sizes(_o, _TERM_SIZES) + _sizes(_o, (1, 17, 1024), mdc=0) + _sizes(_o, (5, 18, 40), smdc=2),
          "topk_kernel: one eligible ordinal per workgroup (two in the last); min_doc_count 0: the first / last k ordinals; "
          "shard_min_doc_count 2 drops the count-1 neighbours")
    _case("c_one_workgroup_%s" % _n, "c", "one_workgroup", T_TAIL1, "beside",
          _sizes(_o, _TERM_SIZES) + _sizes(_o, (16, 1024), smdc=2),
          "topk_kernel: every eligible ordinal inside one workgroup's range, the others return no key")

for _name, _vec, _T, _reqs in (
        ("d_all_equal", "all_equal", T_TAIL1, _sizes(COUNT_DESC, (10, 1024)) + _sizes(COUNT_ASC, (10,))),
        ("d_tie_at_cut", "tie_at_cut", T_TAIL1, _sizes(COUNT_DESC, range(3, 9)) + _sizes(COUNT_ASC, (7,))),
        ("d_shared_subbin", "shared_subbin", T_TAIL1, _sizes(COUNT_DESC, (7, 8, 9)) + _sizes(COUNT_ASC, (7, 8, 9), smdc=2)),
        ("d_every_4099", "every_4099", T_NOTAIL, _sizes(TERM_ASC, (1, 17, 18)) + _sizes(TERM_DESC, (1, 17, 18))),
        ("d_one_workgroup", "one_workgroup", T_TAIL1, _sizes(TERM_ASC, (16, 1024)) + _sizes(TERM_DESC, (16, 1024)))):
    _case(_name, "d", _vec, _T, "stats", _reqs, "64-bit counts: load_counts4 over u64 (two 16-byte loads, the scalar tail)")

_case("e_settled", "e", "settled", T_TAIL1, "lone", _sizes(COUNT_DESC, (10, 1, 9)),
      "path 8: the hot slots' 10th count 3 > max_cold 2: settled, the cold lists never counted")
_case("e_unsettled_11", "e", "settled", T_TAIL1, "lone", _sizes(COUNT_DESC, (11, 100)),
      "path 8: the 11th pick has count 2 = max_cold: the cold lists and the full top-k run")
_case("e_cold_tie", "e", "cold_tie", T_NOTAIL, "lone", _sizes(COUNT_DESC, (10, 5, 6)),
      "path 8: size 5 settles (10 > 1); 6 and 10 tie with > 60,000 ordinals at count 1 = max_cold")
_case("e_settled_accept", "e", "settled_accept", T_TAIL1, "accept", _sizes(COUNT_DESC, (10, 1)),
      "path 9: settled under accept bits, counts from the accepted docs")
_case("e_cold_tie_accept", "e", "cold_tie_accept", T_NOTAIL, "accept", _sizes(COUNT_DESC, (10, 5, 6)),
      "path 9: picks 6 .. 10 are cold ordinals 0 .. 4 at count 1, tied with > 60,000 ordinals: the scatter form counts them")
_case("e_cold_winner_accept", "e", "cold_winner", T_NOTAIL, "accept", _sizes(COUNT_DESC, (10, 5, 6)),
      "path 9: the hot slots' 10th count = max_cold = 2 and the cold ordinal X = 20,000 wins the tie")


def case_names(group):
    return [n for n, c in CASES.items() if c["group"] == group]


# ---- rows (f), replay (g), co-located reduce (h) ---------------------------------------------------------------------
ROW_T = (5, 64, 65, 4096, 4097)


@functools.lru_cache(maxsize=None)
def row_matrix(T):
    """3 hour rows: counts 2 + (t % 64) % 5 (ordinals t and t + 64 tie: one lane's share; ties at every level besides),
    an all-equal row of 3, and a row of zeros (its 40 docs have no ordinal)"""
    t = np.arange(T, dtype=np.int64)
    m = np.stack([2 + (t % 64) % 5, np.full(T, 3, dtype=np.int64), np.zeros(T, dtype=np.int64)])
    m.setflags(write=False)
    return m


ROW_MISSING = (7, 0, 40)


@functools.lru_cache(maxsize=2)
def row_segment(T):
    return grid_column(row_matrix(T), [T0 + r * HOUR for r in range(3)], "@timestamp", missing=list(ROW_MISSING), seed=T)


def row_requests(T):
    """(order, shard_size, min_doc_count, shard_min_doc_count)"""
    sizes = sorted({1, 3, T} | ({1024, 1025} if T == 4097 else set()))
    out = []
    for o in (COUNT_DESC, COUNT_ASC):
        out += [req(o, s) for s in sizes]
        out += [req(o, min(T, 7), mdc=0), req(o, T, mdc=0), req(o, min(T, 7), smdc=4), req(o, T, mdc=0, smdc=3)]
    return out


REPLAY_T = T_TAIL1
REPLAY_VECTORS = ("all_equal", "shared_subbin", "tie_at_cut")


@functools.lru_cache(maxsize=1)
def replay_matrix():
    m = np.stack([vector(v, REPLAY_T) for v in REPLAY_VECTORS])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=1)
def replay_segment():
    return grid_column(replay_matrix(), [0, 1, 2], "a", missing=[50, 0, 3], seed=9)


COLO_V = (1, 2, 3, 4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def colo_vectors(V):
    """two shards' count vectors over V ordinals: zeros (every 5th ordinal in shard 0, every 7th in shard 1), counts
    1 .. 4 elsewhere with ties at every level, the first and last ordinal tied at the top"""
    t = np.arange(V, dtype=np.int64)
    a = np.where(t % 5 == 3, 0, 1 + (t % 64) % 4)
    b = np.where(t % 7 == 2, 0, 1 + (t * 3 % 64) % 4)
    a[[0, V - 1]] = 9
    b[[0, V - 1]] = 8
    if V == 1:
        a[0], b[0] = 9, 0
    return a, b


@functools.lru_cache(maxsize=2)
def colo_segments(V):
    """per shard (columns, docs): the vector's docs over two hours"""
    out = []
    for s, c in enumerate(colo_vectors(V)):
        cols, n = grid_column(np.stack([c, c]), [T0, T0 + HOUR], "@timestamp", missing=[5, 0], seed=V + s)
        out.append((cols, n))
    return out


def colo_requests(V):
    out = []
    for o in (COUNT_DESC, COUNT_ASC, TERM_ASC, TERM_DESC):
        for size, shard_size in ((1, 1), (3, 5), (V, V)):
            out.append((o, size, shard_size, 1, 0))
        out.append((o, 4, 6, 0, 0))
        out.append((o, 4, 6, 5, 5))  # shard_min_doc_count 5 of 2 hours x counts 1 .. 4: per-shard totals 2 .. 8, 16 / 18
    return out
