"""Collect kernels that carry a zone block's key range with the prefetch: a workgroup must walk several
blocks, and more than one group of 4, for the carried range or the range loaded a block ahead to go wrong.

A workgroup's block count is bounded by ceil(blocks / resident workgroups); with 256 CUs x 3 workgroups, 31,461,003 docs
(3,841 zone blocks of 8,192, a ragged last one that is no multiple of 4 docs) give every workgroup 5 or 6 blocks, i.e.
two groups.  Every case is compared with the CPU oracle on host copies of the same columns (helpers.assert_same: counts,
keys and the integer-valued metric's sums bit-exact).
"""
import numpy as np
import pytest

import oracle as O
from elasticsearch_amd import AggregationBuilders as AB
from elasticsearch_amd import QueryBuilders as QB
from elasticsearch_amd import reduce
from helpers import assert_same, bits_from_mask, synthetic_columns

pytestmark = pytest.mark.gpu

N_DOCS = 31_461_000 + 3
FIELDS = ("host", "@timestamp", "response_time_ms", "status", "bytes")
_cols = {}


def columns(jitter):
    """host copies of the synthetic shard at a timestamp displacement, generated once per module run"""
    if jitter not in _cols:
        _cols[jitter] = synthetic_columns(FIELDS, N_DOCS, ts_jitter_ms=jitter)
    return _cols[jitter]


def north_star(interval="1h"):
    return [AB.terms("hosts").field("host").size(10).subAggregation(
        AB.dateHistogram("per_hour").field("@timestamp").interval(interval).subAggregation(
            AB.stats("rt").field("response_time_ms")))]


def check(engine, aggs, fields, jitter=0, filters=None, cols=None):
    """the request over the synthetic shard (device-generated, or `cols` uploaded) against the oracle"""
    host = cols if cols is not None else {f: columns(jitter)[f] for f in fields}
    want = O.run([(host, N_DOCS)], aggs, filters=filters)
    if cols is not None:
        seg = engine.upload_segment(cols, N_DOCS)
    else:
        seg = engine.synthetic_segment(N_DOCS, fields=fields, ts_jitter_ms=jitter)
    plan = engine.plan(aggs, filters=filters)
    plan.collect(seg)
    res = plan.build()
    assert_same(res.to_dict(), want["shards"][0], "shard")
    assert_same(reduce([res]).to_dict(), want["reduced"], "reduced")
    plan.close()
    seg.close()


def test_shape_walks_two_groups():
    assert N_DOCS % 8192 != 0 and N_DOCS % 4 != 0
    blocks = -(-N_DOCS // 8192)
    assert -(-blocks // (256 * 3)) >= 5  # more than one group of 4 blocks per workgroup


# time-sorted; +-1 h (multi-pass groups: the prefetch wraps back to the group's first block); +-1 min (the 32-bit-delta
# kernels' single-key block skip)
@pytest.mark.parametrize("jitter", [0, 3_600_000, 60_000])
def test_north_star(engine, jitter):
    check(engine, north_star(), ("host", "@timestamp", "response_time_ms"), jitter=jitter)


def test_config2_date_histogram_extended_stats(engine):
    aggs = [AB.dateHistogram("per_hour").field("@timestamp").interval("1h").subAggregation(
        AB.extendedStats("rt").field("response_time_ms"))]
    check(engine, aggs, ("@timestamp", "response_time_ms"))


def test_config5_folded_bitset(engine):
    aggs = [AB.terms("hosts").field("host").size(10).subAggregation(
        AB.dateHistogram("per_hour").field("@timestamp").interval("1h").subAggregation(AB.avg("rt").field("response_time_ms")))]
    flt = [QB.termQuery("status", 200), QB.rangeQuery("bytes").gte(1024).lte(65536)]
    check(engine, aggs, FIELDS, filters=flt)


def test_blocks_without_a_key(engine):
    """15 % of the timestamps missing, in runs of 20,011 docs (each holds at least one whole zone block: no key at all,
    kmn > kmx) and, for a tenth of them, doc by doc"""
    rng = np.random.default_rng(5)
    run = 20_011
    present = np.repeat(rng.random(-(-N_DOCS // run)) >= 0.135, run)[:N_DOCS]
    present &= rng.random(N_DOCS) >= 0.015
    assert not present.reshape(-1)[: (N_DOCS // 8192) * 8192].reshape(-1, 8192).any(axis=1).all()  # whole blocks missing
    cols = {f: dict(columns(0)[f]) for f in ("host", "@timestamp", "response_time_ms")}
    cols["@timestamp"]["present"] = bits_from_mask(present)
    check(engine, north_star(), None, cols=cols)


def test_one_minute_interval(engine):
    """a zone block of the shard spans more than a minute, so the window slides at nearly every block -- in the first
    tenth of the docs (77 workgroups' ranges); the rest of the timestamps are drawn together 64-fold, which keeps the
    request at 0.7M cells of 1,000 hosts x minutes (5.6M over the whole shard at its own spacing: half a minute of
    oracle time) and adds ranges whose window stays for tens of blocks, and the range in which the two meet"""
    ts = columns(0)["@timestamp"]["values"]
    cut = N_DOCS // 10
    fine = ts[:cut]
    assert (fine[8192::8192] // 60_000 != fine[:-8192:8192] // 60_000).mean() > 0.9
    cols = {f: dict(columns(0)[f]) for f in ("host", "@timestamp", "response_time_ms")}
    cols["@timestamp"]["values"] = np.concatenate([fine, ts[cut] + (ts[cut:] - ts[cut]) // 64])
    check(engine, north_star("1m"), None, cols=cols)
