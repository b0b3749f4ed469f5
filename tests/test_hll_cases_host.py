"""The crafted-hash HLL cases (tests/hll_ref.py) without a GPU.

Three things are settled here, before tests/test_gpu_hll_crafted.py trusts the cases on the GPU: the runtime constants the
builders restate are the ones in the kernel sources (a retuned constant fails here instead of silently moving a case off
its branch); the numpy reference and the oracle agree on every case (precision, mode, the exact set or the registers, and
the value -- the bias-corrected estimate is the oracle's alone); and every case's preconditions hold for the reference
alone.  The GPU exposes no counter for "the log overflowed": that an input reaches its branch is proved here, by
arithmetic on the input.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import hll_ref as H
import oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "elasticsearch_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define %s (\d+)\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_restated_constants_are_the_sources():
    hpp, hip, rt = _src("esgpu_kernels.hpp"), _src("esgpu_kernels.hip"), _src("esgpu_runtime.cpp")
    assert _define(hpp, "ESGPU_HLL_CUT0") == H.CUT0
    assert _define(hip, "ESGPU_HLL_GROW") == H.GROW
    assert _define(hip, "ESGPU_HLL_FS_LOG") == H.FS_LOG
    assert _define(hip, "ESGPU_HLL_BITS") == 4 and H.NIBBLE_MAX == (1 << 4) - 1
    assert _define(hip, "ESGPU_HLL_FS_WG") == 1024 and _define(hip, "ESGPU_HLL_FS_NBUF") == 2
    assert H.FS_MIN_DOCS == 1024 * 4 * 2 * 2  # kHllFsIter (WG * 4) * 2 enc32 words per slot * NBUF
    assert int(re.search(r"constexpr uint32_t kHllLog = (\d+);", hip).group(1)) == H.LDS_LOG
    assert int(re.search(r"constexpr uint32_t kHllGroup = (\d+);", hip).group(1)) == H.GROUP
    assert int(re.search(r"constexpr uint32_t kHllLdsWG = (\d+);", hip).group(1)) * 4 * 4 == H.LDS_MIN_DOCS
    assert "std::min(cus * per_cu, span / (kHllLdsIter * 4))" in hip and "n / (it_docs * ESGPU_HLL_FS_NBUF)" in hip
    # the formula lines, as text
    assert "hll_p0_ranges(uint32_t m) { return m >= 256u * 64u ? 256u : m / 64u; }" in hpp
    assert "return (cut0 * (m / hll_p0_ranges(m)) * 9u / 8u + 256u + 3u) & ~3u;" in hpp
    assert "const double lam = (double)total / m, need = std::log(m) + 5.3;" in hip
    assert "if (lam < need * 2.0) return 0;" in hip
    assert "const uint32_t f = 1u + (uint32_t)std::floor(std::log2(lam / need));" in hip
    assert "const double e = (double)n / std::ldexp(1.0, (int)f - 1) / R;" in hip
    assert "const double c = e + e / 8 + 8 * std::sqrt(e) + 256;" in hip
    assert re.search(r"ESGPU_HLL_FS_MAXPR.*?: \(uint64_t\)%d;" % H.FS_MAX_PER_REG, rt, re.S)
    assert re.search(r"ESGPU_HLL_FS_MINF.*?: %du;" % H.FS_MIN_F, rt, re.S)
    assert "if (pl.p >= %d) {" % H.FS_MIN_P in rt
    # and as numbers
    assert [H.ranges(1 << p) for p in (12, 13, 14, 18)] == [64, 128, 256, 256]
    assert H.p0_cap(1 << 12) == H.p0_cap(1 << 13) == 544 and H.p0_cap(1 << 18) == 4864
    assert [int(x) for x in H.fs_window(12, 4)] == [446226, 892453]
    assert H.fs_floor(446226, 12) == 0 and H.fs_floor(446227, 12) == 4 and H.fs_floor(892454, 12) == 5
    assert H.fs_floor(2 ** 64 - 2048, 12) == 49 and H.fs_floor(2 ** 64 - 2048, 13) == 48


def test_reference_functions_against_the_oracle_primitives():
    L = O.lib()
    x = np.concatenate([np.array([0, 1, (1 << 64) - 1, 1 << 63, 0x7FF8000000000000], dtype=np.uint64),
                        np.random.default_rng(1).integers(0, 1 << 63, size=200).astype(np.uint64) * np.uint64(2) + np.uint64(1)])
    assert np.array_equal(H.unmix64(H.mix64(x)), x) and np.array_equal(H.mix64(H.unmix64(x)), x)
    assert all(int(m) == L.oracle_mix64(int(v)) for v, m in zip(x, H.mix64(x)))
    for p, thr in H.THRESHOLDS.items():
        assert L.oracle_precision_from_threshold(thr) == p, (p, thr)
    for p in (4, 9, 12, 18):
        h = np.concatenate([H.boundary_hashes(p, 0), H.boundary_hashes(p, 2), H.mix64(x)])
        assert [L.oracle_index(int(v), p) for v in h] == H.index(h, p).tolist(), p
        assert [L.oracle_run_len(int(v), p) for v in h] == H.run_len(h, p).tolist(), p
        assert [L.oracle_encode_hash(int(v), p) & 0xFFFFFFFF for v in h] == H.encode(h, p).tolist(), p
        # craft gives the index and run length it is asked for, whatever the salt
        for rl in (1, 2, 39 - p if p < 38 else 1, 64 - p, 65 - p):
            c = H.craft(p, [0, 3, (1 << p) - 1], max(rl, 1), [0, (1 << 64) - 1, 0x123456789ABCDEF])
            assert H.index(c, p).tolist() == [0, 3, (1 << p) - 1] and set(H.run_len(c, p).tolist()) == {max(rl, 1)}, (p, rl)
    # the keyword hash: murmur3_x64_128 h1 of 8-byte terms
    terms = [b"k%07d" % t for t in (0, 1, 59_999)]
    h1, h2 = ctypes.c_uint64(), ctypes.c_uint64()
    for t, got in zip(terms, H.murmur3_h1_8(np.frombuffer(b"".join(terms), dtype="<u8"))):
        L.oracle_murmur3_128(t, 8, 0, ctypes.byref(h1), ctypes.byref(h2))
        assert h1.value == int(got), t
    assert H.fnv1a64(b"") == "cbf29ce484222325" and H.fnv1a64(b"a") == "af63dc4c8601ec8c"


def _oracle(name):
    cols, n, kw, _ = H.case(name)
    aggs, filters = H.request(kw)
    accept = [H.bits_of(kw["accept"])] if kw.get("accept") is not None else None
    return O.run([(cols, n)], aggs, filters=filters, accept=accept)


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_reference_and_oracle_agree_and_the_preconditions_hold(name):
    cols, n, kw, note = H.case(name)
    p = kw["p"]
    hashes = H.case_hashes(name)
    per = hashes if isinstance(hashes, list) else [hashes]
    want = _oracle(name)
    for tree in (want["shards"][0], want["reduced"]):
        for b, (h, got) in enumerate(zip(per, H.sketches(tree, kw))):
            ref = H.expected(h, p)
            for key in ("precision", "mode", "lc_size", "lc_fnv1a64", "registers_fnv1a64"):
                assert got["_internal"].get(key) == ref.get(key), (name, b, key)
            if ref["mode"] == "lc":  # linear counting over 2^25 slots rounds to the count while lc_size^2 / 2^26 < 1 / 2
                assert ref["lc_size"] <= got["value"] <= ref["lc_size"] + ref["lc_size"] ** 2 // (1 << 26) + 1, (name, b)
    pre = kw.get("pre", {})
    m = 1 << p
    if isinstance(hashes, list):
        for h, d in zip(per, pre["bucket_distinct"]):
            assert d is None or len(H.lc_set(h, p)) == d, name
        return
    regs = H.registers(hashes, p)
    up, before = H.raises(hashes, p)
    if "distinct" in pre:
        assert len(H.lc_set(hashes, p)) == pre["distinct"], name
        assert (H.mode(hashes, p) == "lc") == (pre["distinct"] <= H.threshold(p)), name
        if kw.get("split"):  # the first segment alone is still within the threshold
            assert len(H.lc_set(hashes[:kw["split"]], p)) == H.threshold(p), name
    if pre.get("every_doc_raises"):
        assert int(up.sum()) == n == len(hashes), (name, int(up.sum()), n)
        assert regs.min() == regs.max() == 65 - p, name
    if pre.get("first_sweep_only"):
        assert int(up.sum()) == m and up[:m].all(), name
    for (what, entries, cap), factor in zip(pre.get("overflow", []), pre.get("overflow_factor", [])):
        assert entries >= factor * cap, (name, what, entries, cap, factor)
    if pre.get("saturation"):
        gmin = regs.reshape(-1, H.GROUP).min(axis=1)[H.index(hashes, p) // H.GROUP]
        again = up & (before > gmin + H.NIBBLE_MAX)  # raised though its bound was already saturated
        assert int((regs.astype(np.int64) - np.repeat(regs.reshape(-1, H.GROUP).min(axis=1), H.GROUP) > H.NIBBLE_MAX).sum()) > 0, name
        assert int(again.sum()) > 0, name
    if "sole_top" in pre:  # registers 0 .. 62 each reach 65 - p through one doc alone, a third of them in each phase range
        idx, rl = H.index(hashes, p), H.run_len(hashes, p)
        at = np.nonzero(rl == 65 - p)[0]
        assert sorted(idx[at].tolist()) == list(range(pre["sole_top"])), name
        assert [int(((at >= lo) & (at < hi)).sum()) for lo, hi in H.phase_ranges(p, n)] == [pre["sole_top"] // 3] * 3, name
    if "stream_window" in pre:
        F = pre["stream_window"]
        lo, hi = H.fs_window(p, F)
        est = H.raw_estimate(regs)
        assert 1.1 * lo <= est <= 0.9 * hi, (name, est, lo, hi)
        assert H.fs_floor(est, p) == F and p >= H.FS_MIN_P and n <= H.FS_MAX_PER_REG * m, name
    if "below_floor" in pre:  # registers the stream leaves to the tail pass, each holding some value to find
        low = regs < H.FS_MIN_F
        assert int(low.sum()) == pre["below_floor"] and regs[low].min() >= 1, name
    if kw.get("bytes", [None])[-1] == "stream" and "stream_window" not in pre:
        # the staircase's second request: an estimate past 2^64, a floor near the clamp
        est = H.raw_estimate(regs)
        assert est >= 2.0 ** 64 and H.fs_floor(2 ** 64 - 2048, p) >= 48 and n <= H.FS_MAX_PER_REG * m, (name, est)
    if name.startswith("e_stream"):
        # the heavy hitters: one contiguous run of a kept hash (run length >= F), one of a dropped hash (< F)
        rl = H.run_len(hashes, p)
        vals, counts = np.unique(hashes, return_counts=True)
        top = vals[np.argsort(counts)[-2:]]
        assert sorted(int(H.run_len(t, p)[0]) >= H.FS_MIN_F for t in top) == [False, True], name
        for t in top:
            at = np.nonzero(hashes == t)[0]
            inside = rl[at[0]:at[-1] + 1]  # contiguous but for the kept run's sentinels, which are kept as well
            assert len(at) >= 100_000 and len(inside) - len(at) <= 360, name
            assert (inside >= H.FS_MIN_F).all() or (inside < H.FS_MIN_F).all(), name
        assert rl.max() <= 65 - p
        # the sentinels inside the kept run: each the only hash that gives its register run length 30, ~20 per workgroup
        kept = np.nonzero(hashes == top[np.argmax([H.run_len(t, p)[0] for t in top])])[0]
        sent = kept[0] + np.nonzero(hashes[kept[0]:kept[-1] + 1] != hashes[kept[0]])[0]
        assert (rl[sent] == 30).all(), name
        regs_s = H.index(hashes[sent], p)
        assert len(np.unique(regs_s)) == 360 and (regs[regs_s] == 30).all(), name
        assert all(((H.index(hashes, p) == r) & (rl >= 30)).sum() == 1 for r in regs_s[::40]), name
        assert np.diff(sent).max() * 15 <= H.FS_MIN_DOCS, name
    if name.startswith(("a_", "b_", "f_")) and not kw.get("split"):
        assert n % 4 == 3 and n > H.CUT0 * H.GROW * m, name  # three phases and a ragged tail
    if kw.get("split") and name.startswith("a_"):
        assert {kw["split"], n - kw["split"]} == {3 * m + 1, 17 * m + 2}, name


def test_boundary_values_sit_in_every_phase_range():
    for p in (4, 6, 11, 12, 13, 18):
        cols, n, kw, _ = H.case("b_boundary_p%d" % p)
        hashes = H.case_hashes("b_boundary_p%d" % p)
        for r, (lo, hi) in enumerate(H.phase_ranges(p, n)):
            want = H.boundary_hashes(p, r)
            here = np.isin(want, hashes[lo:hi])
            # at p = 4 the first range has 64 docs for 67 hashes: the single-bit hashes of the 3 highest positions
            # (run lengths 1 .. 3, which the random background holds anyway) stay out
            assert here.all() or (p == 4 and r == 0 and here[:hi - lo].all()), (p, r)
        for extreme in (0, (1 << 64) - 1):
            assert (hashes == np.uint64(extreme)).sum() == 3, p
        assert H.run_len(np.uint64(0), p)[0] == 65 - p and H.registers(hashes, p)[0] == 65 - p


def test_double_specials_hash_as_doubleToLongBits():
    cols, n, kw, _ = H.case("a_double_p12")
    v = cols["v"]["values"]
    bits = v.view(np.uint64)
    assert np.isnan(v).sum() > len(H.phase_ranges(12, n)) * 6  # the placed NaNs and the random patterns' own
    assert len(np.unique(bits[np.isnan(v)])) > 6
    h = H.hashes_of(cols["v"], n)
    assert len(np.unique(h[np.isnan(v)])) == 1 and h[np.isnan(v)][0] == H.mix64(H.NAN_BITS)[0]
    zero = H.hashes_of({"type": cols["v"]["type"], "values": np.array([0.0, -0.0])}, 2)
    assert zero[0] != zero[1]
