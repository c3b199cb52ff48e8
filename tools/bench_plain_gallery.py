#!/usr/bin/env python3
"""A plain gallery (PlainEnroller: unencrypted templates, database kinds 7 / 8) beside the encrypted database of the same rows
(DiagonalEnroller), in the same process and session, alternating.  One JSON line per (database size, kind, repeat): enrolment time,
indexScenario per query, loop B per query (hydia_kernel_time: "hydia_plain" for the gallery, "hydia_tensor" for the encrypted
database), resident bytes, the loop-B entries of the byte ledger, and the decrypted index list against the rows planted in the gallery.
The yardstick of a plain line is the encrypted line of the same size and repeat next to it; the spread over the repeats is the margin.
--plain-only sizes (2^21 by default) are run for the gallery alone: the encrypted database of that size does not fit one GPU."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[14, 17, 20])
    ap.add_argument("--plain-only", type=int, nargs="*", default=[21], help="sizes run for the plain gallery alone")
    ap.add_argument("--reps", type=int, default=3, help="alternations plain / encrypted per size")
    ap.add_argument("--queries", type=int, default=5, help="timed indexScenario calls per enrolment")
    args = ap.parse_args()
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
