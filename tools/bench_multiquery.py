#!/usr/bin/env python3
"""A batch of Q queries in one pass over the encrypted database (DiagonalSender.indexScenarioMulti) against Q sequential
indexScenario calls.  One JSON line per (database size, Q): ms per query both ways, database vectors x queries per second, the
loop-B kernel time per query (hydia_kernel_time: "hydia_tensor" for the sequential calls, "hydia_tensor_multi" for the batch),
the byte ledger of the batch's loop B, and whether the decrypted index lists agree.  The database is random residues
(hydia_db_fill_random) at every size: the index lists are compared, not their contents.  A Q that does not fit prints its error."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_matching_amd as im  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[14, 17, 20])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=1)
    args = ap.parse_args()
    cc = im.Context()
    cc.keygen(20250725)
    for l2 in args.log2n:
        n = 1 << l2
        cc.db_fill_random(n, seed=l2)
        cc.sync()
        r, s = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
        rng = np.random.default_rng(l2)
        for Q in args.queries:
            row = {"log2n": l2, "n": n, "queries": Q, "db_kind": cc.db_kind(), "db_group": cc.db_group()}
            try:
                qs = [r.encryptQuery(rng.standard_normal(cc.dim), seed=5, nonce=1 + i) for i in range(Q)]
                # sequential single-query calls (after a warm-up)
                s.indexScenario(qs[0])
                cc.sync()
                cc.kernel_time_reset()
                t0 = time.time()
                for _ in range(args.reps):
                    seq = [s.indexScenario(q) for q in qs]
                cc.sync()
                ms_seq = (time.time() - t0) * 1e3 / (args.reps * Q)
                kt_seq = cc.kernel_time("hydia_tensor")[0] / (args.reps * Q)
                # one batch (after a warm-up)
                s.indexScenarioMulti(qs)
                cc.sync()
                cc.kernel_time_reset()
                im.byte_ledger(1)
                t0 = time.time()
                for _ in range(args.reps):
                    multi = s.indexScenarioMulti(qs)
                cc.sync()
                ms_multi = (time.time() - t0) * 1e3 / (args.reps * Q)
                led = im.byte_ledger(0)
                kt_multi = cc.kernel_time("hydia_tensor_multi")[0] / (args.reps * Q)
                loop_b = {k: v for k, v in led.items() if "hydia_tensor" in k or k == "op:loop_b_multi"}
                agree = all(r.decryptIndex(a) == r.decryptIndex(b) for a, b in zip(seq, multi))
                bitexact = all(np.array_equal(a.export(), b.export()) for a, b in zip(seq, multi))
                row.update({"seq_ms_per_query": round(ms_seq, 3), "multi_ms_per_query": round(ms_multi, 3),
                            "seq_vectors_queries_per_s": round(n * 1e3 / ms_seq), "multi_vectors_queries_per_s": round(n * 1e3 / ms_multi),
                            "loop_b_seq_ms_per_query": round(kt_seq, 3), "loop_b_multi_ms_per_query": round(kt_multi, 3),
                            "loop_b_ratio": round(kt_multi / kt_seq, 3) if kt_seq else None,
                            "ledger_bytes_per_batch": {k: v[1] / args.reps for k, v in loop_b.items()},
                            "index_lists_agree": bool(agree), "bit_exact": bool(bitexact)})
                del seq, multi, qs
            except im.HydiaError as e:
                im.byte_ledger(0)
                row["error"] = str(e)
            print(json.dumps(row), flush=True)
    cc.close()


if __name__ == "__main__":
    main()
