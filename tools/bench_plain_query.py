#!/usr/bin/env python3
"""A plain query (DiagonalSender.encodeQuery: the sender knows the probe) beside the encrypted query against the SAME encrypted
database, in the same process and session, alternating.  The database is random residues (Context.db_fill_random, the form
hydia_auto_babies picks for its size): loop B's time does not depend on what the residues are.  One JSON line per (database size,
query kind, repeat): indexScenario per query over the timed calls, loop B per query (hydia_kernel_time: "hydia_pq" for the plain
query, "hydia_tensor" for the encrypted one), the key-switch inner products per query, and the loop-B entries of the byte ledger.
The yardstick of a plain line is the encrypted line of the same size and repeat next to it; the spread over the repeats is the margin.

--batch Q [Q ...]: plain queries only — single indexScenario calls beside indexScenarioPlainMulti batches of Q distinct probes at each
width of --widths (Context.set_pq_batch_width: queries per database pass), the variants alternating inside every repeat.  One JSON
line per (size, repeat, variant): indexScenario per QUERY, loop B per QUERY (hydia_kernel_time "hydia_pq" / "hydia_pq_multi"), the
sub-batches free HBM cut the batch into, the ledger's loop-B launches and bytes per query.  Only the rotation keys a plain query needs
are generated (powers of two, giant steps).  Single calls on ANOTHER build of the library (a parent commit) come from that build's own
copy of this tool, run alternately with this one in the same session (profiles/plain_query_batch/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_matching_amd as im  # noqa: E402


def measure(cc, sender, query, timer, warmup, queries):
    for _ in range(warmup):
        out = sender.indexScenario(query)
    cc.sync()
    cc.kernel_time_reset()
    im.byte_ledger(1)
    t0 = time.time()
    for _ in range(queries):
        out = sender.indexScenario(query)
    cc.sync()
    ms = (time.time() - t0) * 1e3 / queries
    led = im.byte_ledger(0)
    blocks = len(out)
    del out
    loop_b = {k: v[1] / queries for k, v in led.items() if k.startswith("k_hydia_") or k.startswith("op:loop_") or k == "k_automorph_batch"}
    ks_ms, ks_n = cc.kernel_time("ks_inner_product")
    n = cc.db_stats()[0]
    return {"db_kind": cc.db_kind(), "db_babies": cc.db_babies(), "db_group": cc.db_group(), "db_residue_bits": cc.db_residue_bits(),
            "blocks": blocks, "index_scenario_ms_per_query": round(ms, 3), "vectors_per_s": round(n * 1e3 / ms), "loop_b_timer": timer,
            "loop_b_ms_per_query": round(cc.kernel_time(timer)[0] / queries, 3), "ks_inner_product_ms_per_query": round(ks_ms / queries, 3),
            "ks_inner_product_launches_per_query": ks_n / queries, "ledger_bytes_per_query": loop_b}


def measure_batch(cc, sender, probes, width, warmup, calls):
    """`calls` timed indexScenarioPlainMulti calls of len(probes) probes at `width` queries per pass; figures per query"""
    Q = len(probes)
    cc.set_pq_batch_width(width)
    try:
        for _ in range(warmup):
            out = sender.indexScenarioPlainMulti(probes)
        cc.sync()
        cc.kernel_time_reset()
        im.byte_ledger(1)
        t0 = time.time()
        for _ in range(calls):
            out = sender.indexScenarioPlainMulti(probes)
        cc.sync()
        ms = (time.time() - t0) * 1e3 / (calls * Q)
        led = im.byte_ledger(0)
    finally:
        cc.set_pq_batch_width(0)
    blocks = len(out[0])
    del out
    per = calls * Q
    loop_b = {k: [v[0] / calls, v[1] / per] for k, v in led.items() if k.startswith("k_hydia_") or k.startswith("op:loop_") or k == "k_automorph_batch"}
    lb_ms, lb_n = cc.kernel_time("hydia_pq_multi")
    ks_ms, ks_n = cc.kernel_time("ks_inner_product")
    n = cc.db_stats()[0]
    return {"db_kind": cc.db_kind(), "db_babies": cc.db_babies(), "db_group": cc.db_group(), "db_residue_bits": cc.db_residue_bits(),
            "blocks": blocks, "index_scenario_ms_per_query": round(ms, 3), "vectors_per_s": round(n * 1e3 / ms), "loop_b_timer": "hydia_pq_multi",
            "loop_b_ms_per_query": round(lb_ms / per, 3), "sub_batches_per_call": lb_n / calls, "ks_inner_product_ms_per_query": round(ks_ms / per, 3),
            "ks_inner_product_launches_per_query": ks_n / per, "ledger_launches_per_call_and_bytes_per_query": loop_b}


def main_batch(args):
    cc = im.Context()
    slots = cc.N // 2
    cc.keygen_rotations(sorted({1 << k for k in range(slots.bit_length() - 1)} | set(range(64, cc.dim, 64))), 20250725)
    try:  # the commit the library was built at (image_matching_amd/VERSION, written by the build)
        library = open(os.path.join(os.path.dirname(im.lib_path()), "VERSION")).read().strip()
    except OSError:
        library = "unknown"
    rng = np.random.default_rng(8)
    vecs = rng.choice([-1.0, 1.0], size=(max(args.batch), cc.dim))
    for l2 in args.log2n:
        n = 1 << l2
        cc.db_fill_random(n, 1000 + l2)
        sender = im.DiagonalSender(cc, n)
        probes = sender.encodeQueries(vecs)
        for rep in range(args.reps):
            variants = [("single", 1, 0)] + [("batch", Q, w) for Q in args.batch for w in args.widths if w <= Q]
            for kind, Q, w in variants:
                row = {"log2n": l2, "n": n, "rep": rep, "query": "plain", "variant": kind, "batch": Q, "width": w, "library": library}
                try:
                    if kind == "single":
                        row.update(measure(cc, sender, probes[0], "hydia_pq", args.warmup, args.queries))
                    else:
                        row.update(measure_batch(cc, sender, probes[:Q], w, 1, max(2, args.queries // Q)))
                except im.HydiaError as e:
                    im.byte_ledger(0)
                    row.update({"error": str(e)})
                print(json.dumps(row), flush=True)
        del probes
    cc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[14, 17, 20])
    ap.add_argument("--reps", type=int, default=2, help="alternations encrypted / plain per size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=10, help="timed indexScenario calls per query kind and repeat")
    ap.add_argument("--batch", type=int, nargs="*", default=[], help="plain queries only: batches of these sizes beside single calls")
    ap.add_argument("--widths", type=int, nargs="*", default=[2, 4], help="--batch: queries per database pass to compare (1, 2, 4)")
    args = ap.parse_args()
    if args.batch:
        return main_batch(args)
    cc = im.Context()
    cc.keygen(20250725)  # the full key set: the encrypted query needs rotations 1 .. vector_dim-1, the plain one does not look at them
    receiver = im.DiagonalReceiver(cc, 1)
    enc = receiver.encryptQuery(np.ones(cc.dim), seed=5, nonce=1)
    for l2 in args.log2n:
        n = 1 << l2
        cc.db_fill_random(n, 1000 + l2)
        sender = im.DiagonalSender(cc, n)
        plain = sender.encodeQuery(np.ones(cc.dim))
        for rep in range(args.reps):
            for kind, query, timer in (("encrypted", enc, "hydia_tensor"), ("plain", plain, "hydia_pq")):
                row = {"log2n": l2, "n": n, "rep": rep, "query": kind}
                try:
                    row.update(measure(cc, sender, query, timer, args.warmup, args.queries))
                except im.HydiaError as e:
                    im.byte_ledger(0)
                    row.update({"error": str(e)})
                print(json.dumps(row), flush=True)
        del plain
    del enc
    cc.close()


if __name__ == "__main__":
    main()
