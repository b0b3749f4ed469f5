"""One-time cost of the per-doc value-count product (a lone value_count leaf) for its three sources, on one
GPU.  Writes JSON lines to stdout and to --out.

    python tools/value_count_timing.py [--docs 100000000] [--out profiles/single_value_metrics/product_100m.jsonl]

date_histogram(1h){value_count(field)} is collected and built twice on a fresh segment whose timestamp copies an earlier
date_histogram request has already built.  The first request builds the product of the column (one launch, ending in a
stream synchronise) and collects it as 16-bit integer runs; the second finds it cached and only collects.  Their
difference is the product alone.  Host wall clock; both requests end in the build's synchronise.
Sources: a single-valued keyword column (32-bit ordinals; and its 16-bit copy, built beforehand by a terms request), a
long column with a present bitset, a multi-valued long column (CSR offsets).
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

# bytes per doc the product kernel reads and writes (it writes one u16 per doc)
TRAFFIC = {"ord32": (4, 2), "ord16": (2, 2), "present": (1.0 / 8, 2), "csr": (8, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
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
    rng = np.random.default_rng(3)

    def columns(docs):
        present = rng.random(docs) < 0.6
        pad = np.zeros((docs + 63) // 64 * 64, dtype=bool)
        pad[:docs] = present
        offs = np.zeros(docs + 1, dtype=np.uint64)
        np.cumsum(rng.integers(0, 4, size=docs), out=offs[1:])
        ts = np.sort(rng.integers(1441065600000, 1441065600000 + 30 * 86400000, size=docs)).astype(np.int64)
        return {"@timestamp": {"type": N.COL_I64, "values": ts},
                "sparse": {"type": N.COL_I64, "values": np.zeros(docs, dtype=np.int64),
                           "present": np.packbits(pad, bitorder="little").view(np.uint64)},
                "multi": {"type": N.COL_I64, "values": np.zeros(int(offs[-1]), dtype=np.int64), "offsets": offs}}

    def segment(source, docs, cols):
        if source in ("ord32", "ord16"):
            seg = e.synthetic_segment(docs, fields=("host", "@timestamp"))
            if source == "ord16":  # the 16-bit ordinals exist once a terms request has read the column
                warm(seg, [AB.terms("t").field("host")])
            f = "host"
        else:
            f = "sparse" if source == "present" else "multi"
            seg = e.upload_segment({f: cols[f], "@timestamp": cols["@timestamp"]}, docs)
        warm(seg, [hist()])  # the timestamp column's compact copies
        return seg, f

    def hist():
        return AB.dateHistogram("h").field("@timestamp").interval("1h")

    def warm(seg, aggs):
        p = e.plan(aggs)
        p.collect(seg)
        p.build()
        p.close()

    def request(seg, field):
        p = e.plan([hist().subAggregation(AB.count("c").field(field))])
        t0 = time.perf_counter()
        p.collect(seg)
        r = p.build()
        t1 = time.perf_counter()
        v = sum(b["c"]["value"] for b in r.to_dict()["h"]["buckets"])
        p.close()
        return (t1 - t0) * 1e3, v

    small = columns(1 << 20)
    for s in TRAFFIC:  # warm-up: every kernel once, at a small size
        seg, f = segment(s, 1 << 20, small)
        request(seg, f)
        seg.close()
    cols = columns(a.docs)
    for source, (rd, wr) in TRAFFIC.items():
        for rep in range(a.reps):
            seg, f = segment(source, a.docs, cols)
            used0 = e.hbm_used()
            first, v1 = request(seg, f)
            used1 = e.hbm_used()
            again, v2 = request(seg, f)
            assert v1 == v2
            product_ms = first - again
            moved = (rd + wr) * a.docs
            emit(what="value_count_product_first_use", source=source, docs=a.docs, rep=rep, value_count=v1,
                 first_request_ms=round(first, 3), cached_request_ms=round(again, 3), product_ms=round(product_ms, 3),
                 read_bytes_per_doc=rd, written_bytes_per_doc=wr, product_hbm_bytes=used1 - used0,
                 gb_per_s=round(moved / (product_ms / 1e3) / 1e9, 1) if product_ms > 0 else None)
            seg.close()
    e.close()


if __name__ == "__main__":
    main()
