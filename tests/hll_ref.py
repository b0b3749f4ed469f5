"""A plain HyperLogLog++ reference in numpy and the crafted-hash case tables of tests/test_gpu_hll_crafted.py.

Long and double values are hashed with mix64 (hppc BitMixer: two xor-shift-multiply rounds by odd constants), a bijection
on 64 bits: `unmix64` inverts it, so a column can be written whose every hash has a chosen register index, run length and
encoding (`craft`).  The reference restates HyperLogLogPlusPlus.java (index, runLen, encodeHash with p2 = 25, the Hashset
threshold) with array operations only -- no GPU and none of the project's native code; the column-type constants are the
only thing taken from the package.  tests/test_hll_cases_host.py checks this reference against the oracle and proves
every case's preconditions; the GPU test compares the kernels with both.

Every builder returns (columns, n, request kwargs, note): the column dicts of Engine.upload_segment / oracle.run, the doc
count, what the request and the runner need (see `case`), and one line naming the branch the case is built for.
"""
import functools
import math

import numpy as np

from elasticsearch_amd import _native as N  # the COL_* type constants only

U = np.uint64
MIX_C1, MIX_C2 = 0x4CD6944C5CC20B6D, 0xFC12C5B19D3259E9
MIX_I1, MIX_I2 = pow(MIX_C1, -1, 1 << 64), pow(MIX_C2, -1, 1 << 64)
P2 = 25                      # HyperLogLogPlusPlus.P2: bits of a hash an encoding keeps
NAN_BITS = 0x7FF8000000000000  # Double.doubleToLongBits of every NaN
MISSING = 0xFFFFFFFF         # a keyword doc without an ordinal

# ---- runtime constants the builders depend on (tests/test_hll_cases_host.py reads them back from the source text) -------
CUT0 = 4           # esgpu_kernels.hpp ESGPU_HLL_CUT0: phase 0 spans a request's first CUT0 * 2^p values
GROW = 4           # esgpu_kernels.hip ESGPU_HLL_GROW: each later phase ends at GROW times the previous cut
LDS_LOG = 4096     # esgpu_kernels.hip kHllLog: raises one LDS phase workgroup logs before it falls back to atomics
FS_LOG = 16384     # esgpu_kernels.hip ESGPU_HLL_FS_LOG: the floored stream's per-workgroup log
GROUP = 64         # esgpu_kernels.hip kHllGroup: registers per group floor
NIBBLE_MAX = 15    # esgpu_kernels.hip kHllMaxDelta with ESGPU_HLL_BITS 4: a snapshot nibble saturates here
FS_MIN_P = 12      # esgpu_runtime.cpp collect_hll: ranges, logs and the floored stream exist from p = 12
FS_MAX_PER_REG = 1024  # esgpu_runtime.cpp collect_hll fs_max_per_reg: the stream takes segments of n <= 1024 * m
FS_MIN_F = 4       # esgpu_runtime.cpp collect_hll fs_minf: the smallest floor the stream runs with
LDS_MIN_DOCS = 4096 * 4  # esgpu_kernels.hip launch_hll: an LDS phase workgroup gets at least kHllLdsIter * 4 docs
FS_MIN_DOCS = 4096 * 4   # launch_hll: a stream workgroup gets at least kHllFsIter * 2 (enc32) * ESGPU_HLL_FS_NBUF docs


def ranges(m):
    """esgpu_kernels.hpp hll_p0_ranges: register ranges of phase 0, the raise logs and the stream"""
    return 256 if m >= 256 * 64 else m // 64


def p0_cap(m, cut0=CUT0):
    """esgpu_kernels.hpp hll_p0_cap: entries per register range of phase 0 and of one LDS phase's log"""
    return (cut0 * (m // ranges(m)) * 9 // 8 + 256 + 3) & ~3


def fs_floor(distinct, p, min_f=FS_MIN_F):
    """esgpu_kernels.hip hll_fs_floor: the stream's floor for an estimate of the distinct values (0: the phases run)"""
    m = float(1 << p)
    lam, need = float(int(distinct)) / m, math.log(m) + 5.3
    if lam < need * 2.0:
        return 0
    f = min(1 + int(math.floor(math.log2(lam / need))), 64 - p)
    return f if f >= min_f else 0


def fs_cap(n, p, f):
    """esgpu_kernels.hip hll_fs_cap: entries per register range of the stream"""
    e = n / 2.0 ** (f - 1) / ranges(1 << p)
    return int(min(e + e / 8 + 8 * math.sqrt(e) + 256, 4.0e9)) & ~3


def fs_window(p, f):
    """the distinct counts [lo, hi) for which fs_floor gives f (below its clamp)"""
    need = math.log(float(1 << p)) + 5.3
    return 2.0 ** (f - 1) * need * (1 << p), 2.0 ** f * need * (1 << p)


# precision_threshold -> p (HyperLogLogPlusPlus.precisionFromThreshold); the tests assert each against the oracle's
THRESHOLDS = {4: 1, 5: 5, 6: 10, 7: 20, 8: 40, 9: 80, 10: 100, 11: 300, 12: 500, 13: 1000, 14: 2000, 15: 4000, 16: 8000,
              17: 16000, 18: 40000}


# ---- the reference -----------------------------------------------------------------------------------------------------
def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def mix64(z):
    z = _u64(z)
    z = (z ^ (z >> U(32))) * U(MIX_C1)
    z = (z ^ (z >> U(29))) * U(MIX_C2)
    return z ^ (z >> U(32))


def unmix64(h):
    """mix64's inverse: x ^ (x >> 32) undoes itself, x ^ (x >> 29) is undone by x ^ (x >> 29) ^ (x >> 58)"""
    z = _u64(h)
    z = (z ^ (z >> U(32))) * U(MIX_I2)
    z = (z ^ (z >> U(29)) ^ (z >> U(58))) * U(MIX_I1)
    return z ^ (z >> U(32))


def _bitlen32(v):  # v < 2^32: exact in a double
    return np.frexp(v.astype(np.float64))[1].astype(np.int64)


def clz64(x):
    x = _u64(x)
    hi, lo = x >> U(32), x & U(0xFFFFFFFF)
    return 64 - np.where(hi != 0, 32 + _bitlen32(hi), _bitlen32(lo))


def index(h, p):
    return (_u64(h) >> U(64 - p)).astype(np.int64)


def run_len(h, p):
    return 1 + np.minimum(clz64(_u64(h) << U(p)), 64 - p)


def encode(h, p):
    """HyperLogLogPlusPlus.encodeHash: the top 25 bits, and the run length below them when bits p .. 24 are all zero"""
    h = _u64(h)
    e = h >> U(64 - P2)
    rl = (1 + np.minimum(clz64(h << U(P2)), 64 - P2)).astype(np.uint64)
    odd = (e << U(7)) | (rl << U(1)) | U(1)
    return np.where((e & U((1 << (P2 - p)) - 1)) == 0, odd, e << U(1)).astype(np.uint32)


def bits_of(mask):
    """bool per doc -> the u64 bitset words of include/esgpu.h (bit d of word d // 64)"""
    b = np.packbits(np.asarray(mask, dtype=bool), bitorder="little")
    out = np.zeros(max((len(b) + 7) // 8, 1) * 8, dtype=np.uint8)
    out[:len(b)] = b
    return out.view("<u8").astype(np.uint64)


def mask_of_bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")[:n].astype(bool)


def murmur3_h1_8(terms8):
    """h1 of MurmurHash3_x64_128 (seed 0) of 8-byte keys, given as little-endian u64: only the tail block runs"""
    k1 = _u64(terms8) * U(0x87C37B91114253D5)
    k1 = ((k1 << U(31)) | (k1 >> U(33))) * U(0x4CF5AD432745937F)
    h1, h2 = k1 ^ U(8), np.full(len(k1), 8, dtype=np.uint64)
    h1 = h1 + h2
    h2 = h2 + h1

    def fmix(k):
        k = (k ^ (k >> U(33))) * U(0xFF51AFD7ED558CCD)
        k = (k ^ (k >> U(33))) * U(0xC4CEB9FE1A85EC53)
        return k ^ (k >> U(33))
    h1, h2 = fmix(h1), fmix(h2)
    return h1 + h2


def hashes_of(col, n, accept=None, query=None, term_hashes=None):
    """the hashes a cardinality aggregation collects from `col`, in doc (and value) order: longs and unsigned longs by
    their bits, doubles by doubleToLongBits (every NaN one pattern, -0.0 and 0.0 apart), keyword ordinals through
    `term_hashes`; docs are dropped by the column's present bitset, the accept mask and the query mask (bool per doc);
    a multi-valued column (CSR offsets) contributes every value of a kept doc"""
    keep = np.ones(n, dtype=bool)
    if col.get("present") is not None:
        keep &= mask_of_bits(col["present"], n)
    if accept is not None:
        keep &= np.asarray(accept, dtype=bool)
    if query is not None:
        keep &= np.asarray(query, dtype=bool)
    v = np.ascontiguousarray(col["values"])
    if col.get("offsets") is not None:
        counts = np.diff(np.asarray(col["offsets"]).astype(np.int64))
        keep = np.repeat(keep, counts)
    else:
        v = v[:n]
    if col["type"] == N.COL_ORD_U32:
        keep = keep & (v != MISSING)
        return np.asarray(term_hashes, dtype=np.uint64)[v[keep].astype(np.int64)]
    if col["type"] == N.COL_F64:
        bits = v.astype(np.float64, copy=False).view(np.uint64).copy()
        bits[np.isnan(v)] = U(NAN_BITS)
    else:
        bits = v.view(np.uint64)
    return mix64(bits[keep])


def registers(hashes, p):
    r = np.zeros(1 << p, dtype=np.uint8)
    np.maximum.at(r, index(hashes, p), run_len(hashes, p).astype(np.uint8))
    return r


def lc_set(hashes, p):
    return np.unique(encode(hashes, p))


def threshold(p):
    """the Hashset's capacity before it upgrades (HyperLogLogPlusPlus.java:437-440, float arithmetic)"""
    return int(np.float32((1 << p) // 4) * np.float32(0.75))


def mode(hashes, p):
    return "lc" if len(lc_set(hashes, p)) <= threshold(p) else "hll"


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def registers_fnv(regs):
    return fnv1a64(np.asarray(regs, dtype=np.uint8).tobytes())


def lc_fnv(s):
    return fnv1a64(np.sort(np.asarray(s, dtype=np.uint32)).astype("<u4").tobytes())


def raw_estimate(regs):
    """alpha m^2 / sum 2^-register, the textbook estimator (used only to choose inputs)"""
    m = len(regs)
    return 0.7213 / (1.0 + 1.079 / m) * m * m / float(np.sum(np.ldexp(1.0, -np.asarray(regs, dtype=np.int64))))


def raises(hashes, p):
    """per hash, in order: (it exceeds the running maximum of its register, that running maximum before it)"""
    idx, rl = index(hashes, p), run_len(hashes, p)
    order = np.argsort(idx, kind="stable")
    key = idx[order] * 128 + rl[order]
    prev = np.concatenate([[-1], np.maximum.accumulate(key)[:-1]])
    up = np.empty(len(key), dtype=bool)
    before = np.empty(len(key), dtype=np.int64)
    up[order] = key > prev
    before[order] = np.maximum(prev - idx[order] * 128, 0)
    return up, before


def expected(hashes, p):
    """what a sketch of `hashes` must hold: its mode and the exact set or the registers, with their fingerprints"""
    s = lc_set(hashes, p)
    if len(s) <= threshold(p):
        return {"precision": p, "mode": "lc", "lc_size": int(len(s)), "lc_fnv1a64": lc_fnv(s)}
    regs = registers(hashes, p)
    return {"precision": p, "mode": "hll", "registers": regs, "registers_fnv1a64": registers_fnv(regs)}


# ---- crafting ----------------------------------------------------------------------------------------------------------
def craft(p, idx, rl, salt=0):
    """hashes with register index `idx` and run length `rl` (1 .. 65 - p); the bits below the terminating 1 are `salt`'s"""
    idx, rl, salt = np.broadcast_arrays(_u64(idx), np.atleast_1d(np.asarray(rl, dtype=np.int64)), _u64(salt))
    assert np.all((rl >= 1) & (rl <= 65 - p)) and np.all(idx < U(1 << p))
    body = 64 - p                                   # bits below the index
    top = np.clip(body - rl, 0, 63).astype(np.uint64)  # position of the terminating 1
    one = np.where(rl <= body, U(1) << top, U(0))
    low = np.where(rl <= body, salt & ((U(1) << top) - U(1)), U(0))
    return (idx << U(body)) | one | low


def _rng(*tag):
    return np.random.default_rng([20261020] + [int(t) if not isinstance(t, str) else sum(map(ord, t)) for t in tag])


def _longs(rng, n):
    return rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64, endpoint=True)


def _i64(vals):
    return {"type": N.COL_I64, "values": np.ascontiguousarray(vals).view(np.int64)}


def _values(hashes):
    return unmix64(hashes).view(np.int64)


def phase_ranges(p, n):
    """the doc ranges a fresh request's kernels read: phase 0, the first LDS phase, the rest"""
    m = 1 << p
    cuts = [0, min(CUT0 * m, n), min(CUT0 * GROW * m, n), n]
    return [(cuts[i], cuts[i + 1]) for i in range(3) if cuts[i + 1] > cuts[i]]


def _place(values, items, p):
    """one copy of every item inside each phase range of `values`, evenly spread (a range shorter than the list holds
    its head: the list is ordered most important first)"""
    for r, (lo, hi) in enumerate(phase_ranges(p, len(values))):
        it = items(r)
        k = min(len(it), hi - lo)
        pos = lo + (np.arange(k) * (hi - lo)) // k
        values[pos] = it[:k]
    return values


def _kw(p, field="v", **more):
    return dict({"field": field, "p": p, "threshold": THRESHOLDS[p]}, **more)


def _bytes_note(p, dense=True):
    return ["phase0"] if dense and p >= FS_MIN_P else [None]


# (a) precision sweep
def sweep_long(p, runs=1, split=None, reverse=False):
    n = 20 * (1 << p) + 3
    v = _longs(_rng("sweep", p), n)
    kw = _kw(p, runs=runs, bytes=_bytes_note(p) * runs)
    if split:
        n1 = 3 * (1 << p) + 1
        assert n - n1 == 17 * (1 << p) + 2
        if reverse:  # the long segment first: the short one continues from seen = 17 * 2^p + 2
            v = np.concatenate([v[n1:], v[:n1]])
            n1 = n - n1
        kw.update(split=n1, bytes=[None])
    return {"v": _i64(v)}, n, kw, ("p = %d: phase 0 over 4m docs, LDS phases over [4m, 16m) and [16m, 20m + 3), n %% 4 = 3; "
                                   "p < 12 reads values without a log, p < 6 has fewer than 64 registers" % p)


DOUBLE_SPECIALS = np.array([
    0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF0000000000123,  # NaNs
    0x0000000000000000, 0x8000000000000000,                       # +0.0, -0.0
    0x7FF0000000000000, 0xFFF0000000000000,                       # +inf, -inf
    0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x8000000000000001,   # denormals
], dtype=np.uint64)


def sweep_double(p):
    n = 20 * (1 << p) + 3
    bits = _longs(_rng("double", p), n).view(np.uint64).copy()  # random patterns: one in 2,048 is a NaN of a random payload
    _place(bits, lambda r: DOUBLE_SPECIALS, p)
    col = {"type": N.COL_F64, "values": bits.view(np.float64)}
    return {"v": col}, n, _kw(p, bytes=_bytes_note(p)), "p = %d doubles: NaN payloads canonicalised, -0.0 != 0.0, inf, denormals" % p


# (b) extreme and boundary run lengths
def boundary_hashes(p, r=0):
    """0, all-ones, the enc32 seams, a maximal run in a register of its own, and one set bit at each position below the
    index bits; `r` rotates the register indices, so every phase range's copies raise registers of their own"""
    m = 1 << p
    rot = lambda i: (i + r * (m // 3 + 1)) % m  # noqa: E731
    body = 64 - p
    out = [0, (1 << 64) - 1]
    j = rot(5)
    out += [j << body | 1 << 38, j << body | 1 << 37,  # bits p .. 24 zero: the first set bit at position 25 / 26 (odd encodings)
            rot(6) << body,                            # ... nowhere: run length 65 - p, the stored count clamps at 39
            rot(7) << body | 1 << 39,                  # bits p .. 24 hold only their lowest bit (the last even encoding)
            rot(8) << body | ((1 << body) - 1)]        # run length 1 with every lower bit set
    out += [rot((pos * 2654435761) % m) << body | 1 << pos for pos in range(body)]  # run length 64 - p - pos
    return np.array(out, dtype=np.uint64)


def boundary(p):
    m = 1 << p
    # p = 12: 600,003 docs, so the first request leaves an estimate inside the F = 4 window and the second one streams
    n = 600_003 if p == 12 else 20 * m + 3
    v = _longs(_rng("boundary", p), n)
    _place(v, lambda r: _values(boundary_hashes(p, r)), p)
    kw = _kw(p, bytes=_bytes_note(p))
    if p == 12:
        kw.update(runs=2, bytes=["phase0", "stream"], pre={"stream_window": FS_MIN_F})
    return {"v": _i64(v)}, n, kw, "p = %d: maximal and minimal run lengths and the enc32 seams in every phase range" % p


# (c) the LC / HLL threshold
def _distinct_encodings(p, k, tag):
    """k + 1 hashes of pairwise distinct encodings; the first has an even encoding (bits p .. 24 not all zero)"""
    h = _longs(_rng("lc", p, tag), 2 * k + 64).view(np.uint64)
    _, first = np.unique(encode(h, p), return_index=True)
    h = h[np.sort(first)][:k + 1]
    assert len(h) == k + 1
    even = np.nonzero((encode(h, p) & 1) == 0)[0][0]
    h[[0, even]] = h[[even, 0]]
    return h


def lc_case(p, kind):
    t = threshold(p)
    h = _distinct_encodings(p, t, 0)
    rng = _rng("lcmix", p)
    base = rng.permutation(np.repeat(h[:t], 3))
    kw = _kw(p, bytes=[None], pre={"distinct": t})
    cols = {}
    note = "p = %d, %d distinct encodings (the threshold)" % (p, t)
    if kind == "at":
        v = base
    elif kind == "above":
        v = np.concatenate([base, h[t:]])
        kw["pre"] = {"distinct": t + 1}
        note += " and one more: hll"
    elif kind == "collide":
        v = np.concatenate([base, h[:1] ^ U(1)])  # another hash, the same top 25 bits: the same even encoding
        note += " and a second hash of an encoding already in the set: still lc"
    elif kind == "upgrade":
        v = np.concatenate([base, h[:2], h[t:], h[2:4]])
        kw.update(split=len(base), pre={"distinct": t + 1})
        note += "; the crossing encoding arrives in a second segment of 5 docs"
    elif kind in ("accept", "query"):
        v = np.concatenate([base, h[t:], h[t:]])
        v[[7 % len(base), len(v) - 2]] = v[[len(v) - 2, 7 % len(base)]]  # one copy early, one last
        hidden = v == h[t]
        if kind == "accept":
            kw["accept"] = ~hidden
        else:
            cols["f"] = _i64(np.where(hidden, 0, 1))
            kw.update(filters=[("term", "f", 1)], query=~hidden)
        note += "; the crossing encoding is in the column but hidden by %s" % ("accept bits" if kind == "accept" else "a term filter")
    cols["v"] = _i64(_values(v))
    return cols, len(v), kw, note


# (d) staircases
def staircase(p, kind):
    m, top = 1 << p, 65 - p
    if kind == "one_range":
        # every doc in registers 0 .. 63 (one register range, one group): register 63 only sees run length 1 (in phase 0), so
        # the group floor stays 1 and every other doc (run length 17 .. 65 - p > 1 + 15) passes the saturated nibble filter:
        # an LDS workgroup (>= 16,384 docs) logs 4,096 raises, all of range 0 (capacity 544), and raises the rest directly
        n = 20 * m + 3
        rng = _rng("one_range", p)
        i = np.arange(n)
        low = (i % 64 == 63) & (i < CUT0 * m)
        idx = np.where(low, 63, rng.integers(0, 63, size=n))
        rl = np.where(low, 1, rng.integers(17, top - 1, size=n, endpoint=True))
        (a0, a1), (b0, b1), (c0, c1) = phase_ranges(p, n)
        # each register's final value, 65 - p, comes from one doc alone, for a third of the registers inside each phase: an
        # entry lost on any overflow path shows in the registers with near certainty (most of a phase's entries overflow)
        for r in range(63):
            lo, hi = phase_ranges(p, n)[r % 3]
            at = lo + ((r // 3) * 2 + 1) * (hi - lo) // 42
            at += int(low[at])
            idx[at], rl[at] = r, top
        h = craft(p, idx, rl, _longs(rng, n).view(np.uint64))
        cap = p0_cap(m)
        passing = int((rl[b0:b0 + LDS_MIN_DOCS] > 1 + NIBBLE_MAX).sum())
        pre = {"overflow": [("phase 0 entries of range 0", a1 - a0, cap),
                            ("phase 1 raises of range 0 logged by one workgroup", min(LDS_LOG, passing), cap),
                            ("phase 1 docs past the nibble filter in one workgroup", passing, LDS_LOG)],
               "overflow_factor": [4, 4, 4], "saturation": True, "sole_top": 63}
        return {"v": _i64(_values(h))}, n, _kw(p, bytes=["phase0"], pre=pre), \
            "p = %d: %d phase-0 entries into one range of capacity %d; every LDS workgroup logs 4,096 raises of that range" % (p, a1 - a0, cap)
    n = m * top
    i = np.arange(n)
    idx, step = i % m, 1 + i // m
    rng = _rng("stairs", p, kind)
    salt = _longs(rng, n).view(np.uint64)
    if kind == "half":
        h = craft(p, idx, np.where(idx % 2 == 1, 1, step), salt)
        pre = {"saturation": True}
        note = "odd registers stay at run length 1, even ones climb to %d: nibbles saturate at +15 and are raised again" % top
    else:
        h = craft(p, idx, step, salt)
        pre = {"every_doc_raises": kind != "desc",
               "overflow": [("raises per LDS workgroup (its docs, all raise)", LDS_MIN_DOCS, LDS_LOG)], "overflow_factor": [4]}
        note = "doc i: register i mod m, run length 1 + i // m up to %d: every doc raises, every log overflows" % top
        if kind == "desc":
            h = h[::-1].copy()
            pre = {"first_sweep_only": True}
            note = "the ascending staircase reversed: after the first m docs nothing raises"
    kw = _kw(p, bytes=["phase0"], pre=pre)
    if kind == "asc2":
        # registers all 65 - p: the raw estimate 0.72 m 2^(65-p) is past 2^64; clamped, the stream runs with F = 49 / 48
        kw.update(runs=2, bytes=["phase0", "stream"], floors=[1, 8])
        note += "; the second request streams with a floor near the clamp from an estimate past 2^64"
    return {"v": _i64(_values(h))}, n, kw, "p = %d: %s" % (p, note)


# (e) the floored stream with a real estimate
def stream_case():
    p, m, F = 12, 1 << 12, FS_MIN_F
    n = FS_LOG * 64 - 1                       # 1,048,575 docs: 63 stream workgroups of 16,644 docs, more than one log each
    n_hit, n_drop, n_low, n_sent = 300_000, 108_000, 64, 360
    rng = _rng("stream")
    bg = _longs(rng, 700_000).view(np.uint64)
    bg = bg[index(bg, p) >= 8][:n - n_hit - n_drop - n_low]   # registers 0 .. 7 are reserved
    assert len(bg) == n - n_hit - n_drop - n_low
    low = craft(p, np.arange(n_low) % 8, np.where(np.arange(n_low) % 8 < 4, 3, np.where(np.arange(n_low) < 32, 1, 3)),
                _longs(rng, n_low).view(np.uint64))  # registers 0 .. 7 end at 3 < F from run lengths 1 and 3
    hit = craft(p, 100, 6, 0x1234567)[0]      # kept by the stream: run length 6 >= F
    drop = craft(p, 200, 2, 0x7654321)[0]     # dropped by it: run length 2 < F
    h = np.empty(n, dtype=np.uint64)
    body = np.concatenate([bg, low])
    body = body[rng.permutation(len(body))]
    a, b = 200_000, 650_000                   # the heavy hitters' contiguous runs start here
    h[:a] = body[:a]
    h[a:a + n_hit] = hit
    # inside the run, every 833rd doc (~20 per workgroup) is the one hash that gives its register (8 + 11 j) run length 30:
    # whichever entries pass the end of a workgroup's log, losing them would show in those registers
    h[a + 1 + np.arange(n_sent) * (n_hit // n_sent)] = craft(p, 8 + 11 * np.arange(n_sent), 30, _longs(rng, n_sent).view(np.uint64))
    h[a + n_hit:b] = body[a:b - n_hit]
    h[b:b + n_drop] = drop
    h[b + n_drop:] = body[b - n_hit:]
    pre = {"stream_window": F, "below_floor": 8,
           "overflow": [("stream entries of the heavy hitter's range", n_hit - n_sent, fs_cap(n, p, F)),
                        # a stream workgroup of a segment this small reads 16,384 .. 32,767 docs, under two logs' worth:
                        # the log is filled (factor 1) and passed by n / 63 - 16,384 = 260 entries, never by 4 times
                        ("kept docs of one stream workgroup inside the heavy hitter's run", -(-n // (n // FS_MIN_DOCS)), FS_LOG + 1)],
           "overflow_factor": [4, 1]}
    kw = _kw(p, warm=True, floors=[0, 1, 4, 8], bytes=["stream"], bytes_floor0=["phase0"], pre=pre)
    return {"v": _i64(_values(h))}, n, kw, \
        ("p = 12, ~640K distinct: F = 4; 8 registers end at 3 (tail pass), a 300,000-doc run of one kept hash fills the "
         "16,384-entry log of every workgroup inside it and overflows the range capacity %d, a 108,000-doc run is dropped"
         % fs_cap(n, p, F))


# (f) requests that are not dense
def not_dense(kind):
    p, m = 12, 1 << 12
    n = 20 * m + 3
    rng = _rng("notdense", kind)
    v = _longs(rng, n)
    cols, kw = {}, _kw(p, bytes=[None])
    if kind == "present":
        mask = rng.random(n) < 0.7
        cols["v"] = dict(_i64(np.where(mask, v, 0)), present=bits_of(mask))
    elif kind == "accept":
        cols["v"] = _i64(v)
        kw["accept"] = rng.random(n) < 0.6
    elif kind == "filters":
        s = rng.choice(np.array([200, 404, 500]), size=n, p=[0.8, 0.1, 0.1])
        r = rng.integers(0, 1000, size=n)
        cols.update(v=_i64(v), s=_i64(s), r=_i64(r))
        kw.update(filters=[("term", "s", 200), ("range", "r", 100, 900)], query=(s == 200) & (r >= 100) & (r < 900))
    elif kind == "keyword":
        T = 60_000
        terms = np.frombuffer(b"".join(b"k%07d" % t for t in range(T)), dtype=np.uint8)
        ords = rng.integers(0, T, size=n).astype(np.uint32)
        ords[rng.random(n) < 0.05] = MISSING
        cols["v"] = {"type": N.COL_ORD_U32, "values": ords,
                     "terms_blob": (terms.copy(), np.arange(0, 8 * (T + 1), 8, dtype=np.uint64))}
        kw["term_hashes"] = murmur3_h1_8(terms.view("<u8"))
    elif kind == "multi":
        counts = rng.integers(0, 4, size=n)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(counts)
        cols["v"] = dict(_i64(_longs(rng, int(offs[-1]))), offsets=offs)
    return cols, n, kw, "p = 12, %s: the generic / fast / ordinal register kernels across the phase cuts" % kind


# (g) per-bucket sketches
def buckets_case():
    p, t = 9, threshold(9)  # terms{cardinality} at the default precision: 14 - 5 = 9, threshold 96
    assert t == 96
    h = _distinct_encodings(p, t, 1)
    parts = [np.repeat(h[:t], 2), np.concatenate([np.repeat(h[:t], 2), h[t:]]),
             np.concatenate([boundary_hashes(p, 0), _longs(_rng("bucket2"), 200).view(np.uint64)])]
    k = np.concatenate([np.full(len(x), b, dtype=np.uint32) for b, x in enumerate(parts)])
    order = _rng("buckets").permutation(len(k))
    cols = {"k": {"type": N.COL_ORD_U32, "values": k[order], "terms": ["b0", "b1", "b2"]},
            "v": _i64(_values(np.concatenate(parts)[order]))}
    kw = {"field": "v", "p": p, "threshold": None, "bucket_field": "k", "buckets": 3, "bytes": [None],
          "pre": {"bucket_distinct": [t, t + 1, None]}}
    return cols, len(k), kw, "terms{cardinality} at p = 9: buckets at 96 and 97 encodings and one with the boundary hashes"


def _cases():
    c = {}
    for p in range(4, 19):
        c["a_long_p%d" % p] = functools.partial(sweep_long, p)
    for p in (4, 5, 6, 11, 12, 18):
        c["a_double_p%d" % p] = functools.partial(sweep_double, p)
    for p in (5, 11, 12, 14):
        c["a_reuse_p%d" % p] = functools.partial(sweep_long, p, runs=2)
        c["a_two_segments_p%d" % p] = functools.partial(sweep_long, p, split=True)
        c["a_two_segments_reversed_p%d" % p] = functools.partial(sweep_long, p, split=True, reverse=True)
    for p in (4, 6, 11, 12, 13, 18):
        c["b_boundary_p%d" % p] = functools.partial(boundary, p)
    for p in (4, 12, 18):
        for kind in ("at", "above", "collide", "upgrade", "accept", "query"):
            c["c_%s_p%d" % (kind, p)] = functools.partial(lc_case, p, kind)
    for p in (12, 13):
        for kind in ("asc", "desc", "half", "one_range"):
            c["d_%s_p%d" % (kind, p)] = functools.partial(staircase, p, kind)
        c["d_asc_twice_p%d" % p] = functools.partial(staircase, p, "asc2")
    c["e_stream_p12"] = stream_case
    for kind in ("present", "accept", "filters", "keyword", "multi"):
        c["f_%s_p12" % kind] = functools.partial(not_dense, kind)
    c["g_buckets_p9"] = buckets_case
    return c


CASES = _cases()


@functools.lru_cache(maxsize=4)
def case(name):
    """(columns, n, kwargs, note) of a case.  kwargs: field, p, threshold; runs (requests on one plan, reset between);
    split (docs of the first of two segments); accept / query (bool per doc) and filters (("term", field, value) /
    ("range", field, gte, lt)); term_hashes (keyword); warm (an earlier request leaves the segment's estimate); floors
    (hll_floor values to run under); bytes (per run: "phase0" / "stream" / None, what last_collect_stats()[1] must show);
    pre (the preconditions tests/test_hll_cases_host.py proves)"""
    return CASES[name]()


def case_hashes(name):
    """the hashes the case's request collects (per bucket for the bucket case), from the reference alone"""
    cols, n, kw, _ = case(name)
    if kw.get("bucket_field"):
        k = cols[kw["bucket_field"]]["values"]
        return [mix64(cols[kw["field"]]["values"].view(np.uint64)[k == b]) for b in range(kw["buckets"])]
    return hashes_of(cols[kw["field"]], n, accept=kw.get("accept"), query=kw.get("query"), term_hashes=kw.get("term_hashes"))


def expected_bytes(kind, p, n):
    """last_collect_stats()[1] of a fresh plan over one dense long / double column at p >= 12"""
    return 4 * n if kind == "stream" else 4 * n + 4 * min(n, CUT0 * (1 << p))


def request(kw):
    """the aggregation builders and query filters of a case (the package's request builders, as a client would)"""
    from elasticsearch_amd import AggregationBuilders as AB
    from elasticsearch_amd import QueryBuilders as QB
    card = AB.cardinality("c").field(kw["field"])
    if kw.get("threshold") is not None:
        card = card.precisionThreshold(kw["threshold"])
    aggs = [AB.terms("t").field(kw["bucket_field"]).size(kw["buckets"]).subAggregation(card)] if kw.get("bucket_field") else [card]
    filters = None
    if kw.get("filters"):
        filters = [QB.termQuery(f[1], f[2]) if f[0] == "term" else QB.rangeQuery(f[1]).gte(f[2]).lt(f[3]) for f in kw["filters"]]
    return aggs, filters


def sketches(tree, kw):
    """the cardinality objects of a parsed shard or reduced result: [c] or, for the bucket case, one per bucket b0, b1, ..."""
    if not kw.get("bucket_field"):
        return [tree["c"]]
    by_key = {b["key"]: b["c"] for b in tree["t"]["buckets"]}
    return [by_key["b%d" % b] for b in range(kw["buckets"])]
