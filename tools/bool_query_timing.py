"""HIP-event time of the bool query's doc-bitset kernel (esgpu_bool_bits.hip, DESIGN §5 "Bool queries") beside the
closest plain-form work, on one GPU.  Writes JSON lines to stdout and to --out.

    timeout 600 python tools/bool_query_timing.py [--docs 100000000] [--out profiles/bool_query/bits_100m.jsonl]

bool:  must(range response_time_ms) + must_not(term status) + should(range bytes, exists price): one kernel over the four
       leaf columns at their upload widths (8 bytes each) that writes one bit per doc.
fold:  a five-clause plain conjunction over the same columns (two range clauses on response_time_ms, one on status, bytes
       and price each): more than four clauses, so set_preds folds them into a doc bitset by two chained filter_bits
       passes, which read the long columns' compact copies (16- and 32-bit deltas) where they exist.
Both under a top-level stats aggregation; the times are the doc-bitset pass alone (Plan.last_doc_bitset_stats: HIP events
on the plan's stream), the bytes what the pass read and wrote.  One process, one segment, the first repetition discarded.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import elasticsearch_amd as ea  # noqa: E402
from elasticsearch_amd import AggregationBuilders as AB  # noqa: E402
from elasticsearch_amd import QueryBuilders as QB  # noqa: E402

RT = "response_time_ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    queries = {
        "bool": (QB.boolQuery().must(QB.rangeQuery(RT).gte(10).lt(900)).mustNot(QB.termQuery("status", 404))
                 .should(QB.rangeQuery("bytes").gte(1000)).should(QB.existsQuery("price"))),
        "fold": [QB.rangeQuery(RT).gte(10), QB.rangeQuery(RT).lt(900), QB.rangeQuery("status").lt(404),
                 QB.rangeQuery("bytes").gte(1000), QB.rangeQuery("price").gte(0.0)],
    }
    e = ea.Engine(0)
    seg = e.synthetic_segment(a.docs, fields=(RT, "status", "bytes", "price"))
    for what, q in queries.items():
        plan = e.plan([AB.stats("s").field("bytes")], filters=q)
        for rep in range(a.reps + 1):
            plan.collect(seg)
            ms, nbytes = plan.last_doc_bitset_stats()
            count = plan.build().to_dict()["s"]["count"]
            plan.reset()
            if rep == 0:
                continue  # builds the compact copies, loads the kernels
            emit(what="doc_bitset_" + what, docs=a.docs, rep=rep, matched=count, kernel_ms=round(ms, 4), bytes=nbytes,
                 bytes_per_doc=round(nbytes / a.docs, 3), gb_per_s=round(nbytes / (ms / 1e3) / 1e9, 1) if ms > 0 else None)
        plan.close()
    seg.close()
    e.close()


if __name__ == "__main__":
    main()
