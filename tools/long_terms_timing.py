"""One-time cost of the numeric-ordinal product (terms over long fields) and the steady-state collect of
terms(status) against terms(host), on one GPU.  Writes JSON lines to stdout and to --out.

    python tools/long_terms_timing.py [--docs 100000000] [--out profiles/long_terms_numord_100m.jsonl]

Product cost: Engine.ordinal_map([segment], field) is timed twice on a fresh segment.  The first call builds the
product, merges the single dictionary and remaps the ordinals; the second finds the product cached and only merges and
remaps.  Their difference is the product alone.  Host wall clock; both calls end in a device synchronise.
Fields: synthetic status and bytes (dense path), synthetic @timestamp (wide path, every doc distinct: needs the cap
raised), and an uploaded column of --wide-distinct values spread over the 64-bit range (wide path under the default cap).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import elasticsearch_amd as ea  # noqa: E402
from elasticsearch_amd import AggregationBuilders as AB  # noqa: E402
from elasticsearch_amd import _native as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wide-distinct", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    e = ea.Engine(0)
    default_cap = e.get_option("numeric_terms_max_distinct")
    rng = np.random.default_rng(1)
    pool = rng.integers(-(1 << 62), 1 << 62, size=a.wide_distinct, dtype=np.int64)
    ids = pool[rng.integers(0, len(pool), size=a.docs)]

    def segment(field, docs):
        if field == "ids":
            return e.upload_segment({"ids": {"type": N.COL_I64, "values": ids[:docs]}}, docs)
        return e.synthetic_segment(docs, fields=(field,))

    # warm-up: every kernel of both paths once, at a small size
    e.set_option("numeric_terms_max_distinct", 1 << 27)
    for f in ("status", "bytes", "@timestamp", "ids"):
        w = segment(f, 1 << 20)
        e.ordinal_map([w], f).close()
        w.close()
    for field in ("status", "bytes", "ids", "@timestamp"):
        e.set_option("numeric_terms_max_distinct", (1 << 27) if field == "@timestamp" else default_cap)
        for rep in range(a.reps):
            seg = segment(field, a.docs)
            used0 = e.hbm_used()
            t0 = time.perf_counter()
            m = e.ordinal_map([seg], field)
            t1 = time.perf_counter()
            distinct, used1 = m.value_count, e.hbm_used()
            m.close()
            t2 = time.perf_counter()
            m = e.ordinal_map([seg], field)
            t3 = time.perf_counter()
            m.close()
            first, again = (t1 - t0) * 1e3, (t3 - t2) * 1e3
            emit(what="numeric_ordinals_first_use", field=field, docs=a.docs, rep=rep, distinct=distinct,
                 first_map_ms=round(first, 3), cached_map_ms=round(again, 3), product_ms=round(first - again, 3),
                 product_and_map_bytes=used1 - used0)
            seg.close()
    e.set_option("numeric_terms_max_distinct", default_cap)
    # steady state: the same kernel reads a 16-bit ordinal per doc either way
    seg = e.synthetic_segment(a.docs, fields=("status", "host"))
    plans = {"status": e.plan([AB.terms("t").field("status")]), "host": e.plan([AB.terms("t").field("host")])}
    for p in plans.values():  # first use: products, code objects
        p.collect(seg)
        p.build()
    times = {k: [] for k in plans}
    for _ in range(20):
        for k, p in plans.items():  # alternating
            p.reset()
            p.collect(seg)
            p.build()
            times[k].append(p.last_collect_stats()[0])
    for k in plans:
        t = np.array(times[k])
        emit(what="terms_steady_state", field=k, docs=a.docs, reps=len(t), kernel_ms_median=round(float(np.median(t)), 4),
             kernel_ms_min=round(float(t.min()), 4), kernel_ms_max=round(float(t.max()), 4))
    for p in plans.values():
        p.close()
    seg.close()
    e.close()


if __name__ == "__main__":
    main()
