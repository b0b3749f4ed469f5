"""GPU parity of top-level cardinality (collect path 3) on crafted hashes: every HLL register path, exactly.

Uniform hashes cannot fill a raise log or a register range, saturate a snapshot nibble, leave a register below the
stream's floor, land on the LC / HLL threshold, produce a maximal run length or give two values one encoding; a heavily
repeated value, a sorted column or a small precision_threshold can.  mix64 is a bijection, so tests/hll_ref.py inverts it
and writes columns whose every hash has a chosen register, run length and encoding.  That each case reaches its branch is
arithmetic on the input, stated at its builder in tests/hll_ref.py and asserted by tests/test_hll_cases_host.py (the GPU
has no counter for it); here the kernels' results are compared, exactly, with the numpy reference (registers element by
element, or the linear-counting set's size and fingerprint) and, whole, with the oracle.

Which kernels a fresh request over one dense long / double column ran shows in last_collect_stats()[1] at p >= 12: the
enc32 words are 4 bytes per doc, phase 0 reads the 8-byte values of the first 4 * 2^p docs as well -- 4n for the floored
stream, 4n + 4 min(n, 4 * 2^p) for the phases.

The value-reading variants of hll_fs_kernel and of the p >= 12 LDS kernel over a dense column (ESGPU_HLL_E32=0, or a failed
enc32 allocation) are not reached by any case.
"""
import functools

import numpy as np
import pytest

import hll_ref as H
import oracle as O
from elasticsearch_amd import reduce
from helpers import assert_same
from test_gpu_small_segments import device_errors_end_the_session

pytestmark = pytest.mark.gpu


def _names(prefix):
    return [n for n in H.CASES if n.startswith(prefix)]


@functools.lru_cache(maxsize=2)
def _reference(name):
    """the oracle's result and the numpy reference's sketches of a case, computed once"""
    cols, n, kw, _ = H.case(name)
    aggs, filters = H.request(kw)
    accept = [H.bits_of(kw["accept"])] if kw.get("accept") is not None else None
    want = O.run([(cols, n)], aggs, filters=filters, accept=accept)
    hashes = H.case_hashes(name)
    return want, [H.expected(h, kw["p"]) for h in (hashes if isinstance(hashes, list) else [hashes])]


def _assert_registers(got, want, tag):
    assert got is not None and got.shape == want.shape, "%s: no registers of 2^p entries" % tag
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        g = i // H.GROUP
        raise AssertionError("%s: %d registers differ, the first at index %d (group %d, registers %d..%d): got %d, expected %d"
                             % (tag, len(bad), i, g, g * H.GROUP, g * H.GROUP + H.GROUP - 1, got[i], want[i]))


def _check(res, kw, want, refs, tag):
    got = res.to_dict()
    for b, (ref, sk) in enumerate(zip(refs, H.sketches(got, kw))):
        inner = sk["_internal"]
        assert inner["precision"] == kw["p"], "%s: precision %s" % (tag, inner["precision"])
        assert inner["mode"] == ref["mode"], "%s bucket %d: mode %s, expected %s" % (tag, b, inner["mode"], ref["mode"])
        if ref["mode"] == "lc":
            assert (inner["lc_size"], inner["lc_fnv1a64"]) == (ref["lc_size"], ref["lc_fnv1a64"]), "%s bucket %d: lc set" % (tag, b)
        elif kw.get("bucket_field"):
            assert inner["registers_fnv1a64"] == ref["registers_fnv1a64"], "%s bucket %d: registers" % (tag, b)
        else:
            _assert_registers(res.registers(0), ref["registers"], tag)
    assert_same(got, want["shards"][0], tag + " shard")
    assert_same(reduce([res]).to_dict(), want["reduced"], tag + " reduced")


def _segments(cols, n, kw):
    """[(columns, docs, accept bits)]: the whole case, or its two segments"""
    bits = H.bits_of(kw["accept"]) if kw.get("accept") is not None else None
    if not kw.get("split"):
        return [(cols, n, bits)]
    k = kw["split"]
    return [({f: dict(c, values=c["values"][a:b]) for f, c in cols.items()}, b - a, None) for a, b in ((0, k), (k, n))]


def _run(engine, name):
    cols, n, kw, note = H.case(name)
    p = kw["p"]
    if kw.get("threshold") is not None:
        assert O.lib().oracle_precision_from_threshold(kw["threshold"]) == p
    want, refs = _reference(name)
    aggs, filters = H.request(kw)
    parts = _segments(cols, n, kw)
    segs = []

    def upload():
        for s in segs:
            s.close()
        segs[:] = [engine.upload_segment(c, k) for c, k, _ in parts]

    try:
        with device_errors_end_the_session(lambda: name):
            if kw.get("warm"):  # an earlier request over the segment alone leaves its distinct estimate
                upload()
                plan = engine.plan(aggs, filters=filters)
                plan.collect(segs[0])
                _check(plan.build(), kw, want, refs, "%s (%s) first request" % (name, note))
                plan.close()
            for floor in kw.get("floors", [1]):
                if not kw.get("warm"):
                    upload()  # a fresh segment: no estimate
                engine.set_option("hll_floor", floor)
                plan = engine.plan(aggs, filters=filters)
                expect = kw.get("bytes_floor0") if floor == 0 and kw.get("bytes_floor0") else kw.get("bytes", [None])
                for run in range(kw.get("runs", 1)):
                    tag = "%s (%s) hll_floor %d request %d" % (name, note, floor, run)
                    if run:
                        plan.reset()
                    for seg, (_, _, bits) in zip(segs, parts):
                        plan.collect(seg, accept_bits=bits)
                    if expect[run]:
                        got = plan.last_collect_stats()[1]
                        assert got == H.expected_bytes(expect[run], p, n), \
                            "%s: %d bytes read, expected %d (%s)" % (tag, got, H.expected_bytes(expect[run], p, n), expect[run])
                    _check(plan.build(), kw, want, refs, tag)
                plan.close()
    finally:
        engine.set_option("hll_floor", 1)
        for s in segs:
            s.close()


@pytest.mark.parametrize("name", _names("a_long"))
def test_precision_sweep_longs(engine, name):
    """p = 4 .. 18, n = 20 * 2^p + 3 random longs: phase 0 over the first 4 * 2^p docs, LDS phases over [4, 16) * 2^p and
    [16 * 2^p, n), n % 4 = 3.  p >= 12: hll_p0_scatter / hll_p0_gather, then hll_registers_lds_kernel<E32> with the raise
    log; p < 12: hll_registers_fast_kernel, hll_refresh_kernel and the value-reading LDS kernel without a log; p = 4, 5:
    fewer than 64 registers (one group of 2^p in the refresh, the byte-wise snapshot load in the LDS kernel)."""
    _run(engine, name)


@pytest.mark.parametrize("name", _names("a_double"))
def test_precision_sweep_doubles(engine, name):
    """the same over doubles of random bit patterns with, in every phase range, NaNs of six payloads (one hash,
    doubleToLongBits), +0.0 and -0.0 (two hashes), both infinities and three denormals"""
    _run(engine, name)


@pytest.mark.parametrize("name", _names("a_reuse") + _names("a_two_segments"))
def test_precision_sweep_reuse_and_two_segments(engine, name):
    """reuse: the request again on the same plan after reset() (the estimate of 20 values per register is below the
    stream's 2 * (ln m + 5.3): the phases run again).  two segments: 3 * 2^p + 1 and 17 * 2^p + 2 docs into one plan, in
    both orders; the second segment starts at seen > 0 and continues the cut sequence 4, 16, 64 * 2^p -- after the short
    segment inside phase 0's span (cold), after the long one past two cuts (warm: refresh, then one LDS phase)."""
    _run(engine, name)


@pytest.mark.parametrize("name", _names("b_"))
def test_boundary_run_lengths(engine, name):
    """hash 0 (run length 65 - p in register 0), all-ones, one set bit at each position below the index bits, and the
    enc32 seams (bits p .. 24 zero with the first set bit at position 25, 26 or nowhere; bits p .. 24 holding only their
    lowest bit), one copy inside each doc range a different kernel reads, register indices rotated per range so every
    copy raises.  p = 12: 600,003 docs, whose estimate (asserted on the host inside [1.1 * 446,226, 0.9 * 892,453]) makes
    the second request stream with F = 4 -- the byte count shows it."""
    _run(engine, name)


@pytest.mark.parametrize("name", _names("c_"))
def test_lc_hll_threshold(engine, name):
    """threshold(p) = int(float32(2^p / 4) * 0.75) distinct encodings, three copies each: lc with lc_size == threshold;
    one more: hll; a second hash with the first one's even encoding (its lowest bit flipped, the same top 25 bits): still
    lc; the crossing encoding in a second segment: hll; the crossing encoding in the column but hidden by accept bits
    or by a term filter: lc."""
    _run(engine, name)


@pytest.mark.parametrize("name", _names("d_"))
def test_staircases(engine, name):
    """doc i -> register i mod m, run length 1 + i // m: every doc raises, so every floor, group floor and nibble filter
    lets every doc through and an LDS workgroup (at least 16,384 docs) logs 4 times kHllLog raises: the direct-atomic
    path.  desc: only the first m docs raise.  half: odd registers stay at 1, nibbles saturate at +15 and are raised
    again.  one_range: registers 0 .. 63 only: 16,384 phase-0 entries for a range capacity of 544, 4,096 logged raises
    per workgroup for the same 544 slots.  asc_twice: the estimate 0.72 * m * 2^(65 - p) is past 2^64; clamped, the
    second request streams (the byte count) with F = 49 (p = 12) / 48 (p = 13), and with hll_floor 8 at the clamp 64 - p."""
    _run(engine, name)


def test_floored_stream_with_a_real_estimate(engine):
    """p = 12, 1,048,575 docs, ~640K distinct: the first request (phases) leaves an estimate inside the F = 4 window.
    Under hll_floor 0 the phases run again, under 1, 4 and 8 the stream with F = 4, 7, 11: registers 0 .. 7 end at 3 (the
    tail pass finishes them at F = 4; at 7 and 11 it finishes most registers), a 300,000-doc run of one kept hash fills
    the 16,384-entry log of each of the ~18 workgroups inside it (63 of 16,644 docs each) and overflows fs_cap, a 108,000-doc run
    of a hash below the floor is dropped.  Registers equal the reference in all four."""
    _run(engine, "e_stream_p12")


@pytest.mark.parametrize("name", _names("f_"))
def test_not_dense_requests_across_the_cuts(engine, name):
    """p = 12, n = 20 * 2^p + 3: a present bitset, accept bits, a term and a range filter (hll_registers_kernel with the
    floor of hll_floor_kernel); a keyword column of 60,000 terms, 5 % of the docs without an ordinal
    (hll_registers_fast_kernel<HLL_ORD> with group floors); a multi-valued long column (the value array through phase 0
    and the value-reading LDS kernel with the raise log)."""
    _run(engine, name)


def test_per_bucket_sketches(engine):
    """terms(k){cardinality(v)} at the default precision 9 (threshold 96) through card_kernel: a bucket at exactly 96
    encodings (lc), one at 97 (hll), one holding the boundary hashes"""
    _run(engine, "g_buckets_p9")
