#!/usr/bin/env python3
"""A plain gallery (PlainEnroller: unencrypted templates, database kinds 7 / 8) beside the encrypted database of the same rows
(DiagonalEnroller), in the same process and session, alternating.  One JSON line per (database size, kind, repeat): enrolment time,
indexScenario per query, loop B per query (hydia_kernel_time: "hydia_plain" for the gallery, "hydia_tensor" for the encrypted
database), resident bytes, the loop-B entries of the byte ledger, and the decrypted index list against the rows planted in the gallery.
The yardstick of a plain line is the encrypted line of the same size and repeat next to it; the spread over the repeats is the margin.
--plain-only sizes (2^21 by default) are run for the gallery alone: the encrypted database of that size does not fit one GPU.

--batch Q [Q ...]: the gallery only — single indexScenario calls beside indexScenarioGalleryMulti batches of Q distinct encrypted queries
at each width of --widths (Context.set_gallery_batch_width: queries per pass over the gallery), the variants alternating inside every
repeat.  One JSON line per (size, repeat, variant): indexScenario per QUERY, loop B per QUERY (hydia_kernel_time "hydia_plain" /
"hydia_plain_multi"), the sub-batches free HBM cut the batch into, the ledger's loop-B launches and bytes per query.  The gallery is
allocated in the form hydia_auto_babies picks for its size and left at the zero polynomials (plain_db_alloc: loop B's time does not
depend on what the residues are; nothing is decrypted).  Single calls on ANOTHER build of the library (a parent commit) come from a
driver that makes the same single calls on that build, run alternately with this one in the same session
(profiles/plain_gallery_batch/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_matching_amd as im  # noqa: E402


def rows_for(n, dim, seed):
    """n random templates (float64, the enrollers normalise them in place) with a few planted matches of the all-ones query"""
    rng = np.random.default_rng(seed)
    db = np.empty((n, dim), dtype=np.float64)
    step = 1 << 16
    for lo in range(0, n, step):  # in pieces: the generator's temporaries stay small
        db[lo:lo + step] = rng.integers(-99, 100, size=(min(step, n - lo), dim))
    planted = sorted({0, n // 3, n - 1})
    for i in planted:
        db[i] = rng.integers(1, 4, size=dim)
    return db, planted


def measure(cc, kind, rows, planted, queries, timer):
    n = rows.shape[0]
    work = rows.copy()
    cc.sync()
    t0 = time.time()
    if kind == "plain":
        im.PlainEnroller(cc, n).serializeDB(work)
    else:
        im.DiagonalEnroller(cc, n).serializeDB(work, seed=41)
    cc.sync()
    enrol_ms = (time.time() - t0) * 1e3
    del work
    r, s = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
    q = r.encryptQuery(np.ones(cc.dim), seed=5, nonce=1)
    hits = r.decryptIndex(s.indexScenario(q))  # warm-up, and the answer
    cc.sync()
    cc.kernel_time_reset()
    im.byte_ledger(1)
    t0 = time.time()
    for _ in range(queries):
        out = s.indexScenario(q)
    cc.sync()
    ms = (time.time() - t0) * 1e3 / queries
    led = im.byte_ledger(0)
    del out
    loop_b = {k: v[1] / queries for k, v in led.items() if "k_hydia_plain" in k or "k_hydia_tensor" in k or k.startswith("op:loop_b")}
    stats = cc.db_stats()
    return {"kind": kind, "db_kind": cc.db_kind(), "db_babies": cc.db_babies(), "db_group": cc.db_group(), "db_residue_bits": cc.db_residue_bits(),
            "entries": stats[1], "resident_bytes": stats[2], "enrol_ms": round(enrol_ms, 1), "index_scenario_ms_per_query": round(ms, 3),
            "vectors_per_s": round(n * 1e3 / ms), "loop_b_timer": timer, "loop_b_ms_per_query": round(cc.kernel_time(timer)[0] / queries, 3),
            "ledger_bytes_per_query": loop_b, "planted_found": set(planted) <= set(hits), "hits": len(hits)}


def measure_single(cc, sender, query, warmup, queries):
    """`queries` timed single indexScenario calls; the figures of measure_batch"""
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
    loop_b = {k: [v[0] / queries, v[1] / queries] for k, v in led.items() if k.startswith("k_hydia_") or k.startswith("op:loop_")}
    lb_ms, lb_n = cc.kernel_time("hydia_plain")
    return {"blocks": blocks, "index_scenario_ms_per_query": round(ms, 3), "loop_b_timer": "hydia_plain",
            "loop_b_ms_per_query": round(lb_ms / queries, 3), "sub_batches_per_call": lb_n / queries,
            "ledger_launches_per_call_and_bytes_per_query": loop_b}


def measure_batch(cc, sender, qs, width, warmup, calls):
    """`calls` timed indexScenarioGalleryMulti calls of len(qs) queries at `width` queries per pass; figures per query"""
    Q = len(qs)
    cc.set_gallery_batch_width(width)
    try:
        for _ in range(warmup):
            out = sender.indexScenarioGalleryMulti(qs)
        cc.sync()
        cc.kernel_time_reset()
        im.byte_ledger(1)
        t0 = time.time()
        for _ in range(calls):
            out = sender.indexScenarioGalleryMulti(qs)
        cc.sync()
        ms = (time.time() - t0) * 1e3 / (calls * Q)
        led = im.byte_ledger(0)
    finally:
        cc.set_gallery_batch_width(0)
    blocks = len(out[0])
    del out
    per = calls * Q
    loop_b = {k: [v[0] / calls, v[1] / per] for k, v in led.items() if k.startswith("k_hydia_") or k.startswith("op:loop_")}
    lb_ms, lb_n = cc.kernel_time("hydia_plain_multi")
    return {"blocks": blocks, "index_scenario_ms_per_query": round(ms, 3), "loop_b_timer": "hydia_plain_multi",
            "loop_b_ms_per_query": round(lb_ms / per, 3), "sub_batches_per_call": lb_n / calls,
            "ledger_launches_per_call_and_bytes_per_query": loop_b}


def main_batch(args):
    cc = im.Context()
    cc.keygen(20250725)  # loop A of an encrypted query needs the rotation keys 1 .. vector_dim-1
    try:  # the commit the library was built at (image_matching_amd/VERSION, written by the build)
        library = open(os.path.join(os.path.dirname(im.lib_path()), "VERSION")).read().strip()
    except OSError:
        library = "unknown"
    rng = np.random.default_rng(8)
    vecs = rng.choice([-1.0, 1.0], size=(max(args.batch), cc.dim))
    slots = cc.N // 2
    for l2 in args.log2n:
        n = 1 << l2
        cc.plain_db_alloc(n, cc.auto_babies(-(-n // slots)))
        sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
        qs = [receiver.encryptQuery(v, seed=5 + k, nonce=1) for k, v in enumerate(vecs)]
        for rep in range(args.reps):
            variants = [("single", 1, 0)] + [("batch", Q, w) for Q in args.batch for w in sorted({min(w, Q) for w in args.widths})]  # (a batch of one: width 1)
            for kind, Q, w in variants:
                row = {"log2n": l2, "n": n, "rep": rep, "variant": kind, "batch": Q, "width": w, "library": library, "db_kind": cc.db_kind(),
                       "db_babies": cc.db_babies(), "db_group": cc.db_group(), "db_residue_bits": cc.db_residue_bits()}
                try:
                    if kind == "single":
                        row.update(measure_single(cc, sender, qs[0], args.warmup, args.queries))
                    else:
                        row.update(measure_batch(cc, sender, qs[:Q], w, 1, max(2, args.queries // Q)))
                except im.HydiaError as e:
                    im.byte_ledger(0)
                    row.update({"error": str(e)})
                print(json.dumps(row), flush=True)
        del qs
    cc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[14, 17, 20])
    ap.add_argument("--plain-only", type=int, nargs="*", default=[21], help="sizes run for the plain gallery alone")
    ap.add_argument("--reps", type=int, default=3, help="alternations plain / encrypted per size")
    ap.add_argument("--queries", type=int, default=5, help="timed indexScenario calls per enrolment")
    ap.add_argument("--warmup", type=int, default=2, help="--batch: untimed single calls before the timed ones")
    ap.add_argument("--batch", type=int, nargs="*", default=[], help="the gallery only: batches of these sizes beside single calls")
    ap.add_argument("--widths", type=int, nargs="*", default=[2, 4], help="--batch: queries per pass over the gallery to compare (1, 2, 4)")
    args = ap.parse_args()
    if args.batch:
        return main_batch(args)
    cc = im.Context()
    cc.keygen(20250725)
    for l2, kinds in [(l, ("plain", "encrypted")) for l in args.log2n] + [(l, ("plain",)) for l in args.plain_only]:
        rows, planted = rows_for(1 << l2, cc.dim, l2)
        for rep in range(args.reps):
            for kind in kinds:
                row = {"log2n": l2, "n": 1 << l2, "rep": rep}
                try:
                    row.update(measure(cc, kind, rows, planted, args.queries, "hydia_plain" if kind == "plain" else "hydia_tensor"))
                except im.HydiaError as e:
                    im.byte_ledger(0)
                    row.update({"kind": kind, "error": str(e)})
                print(json.dumps(row), flush=True)
        del rows
    cc.close()


if __name__ == "__main__":
    main()
