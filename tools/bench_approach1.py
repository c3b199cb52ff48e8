#!/usr/bin/env python3
"""Approach 1 (the literature baseline) on the GPU stack: enrol a random row-packed database of 2^k vectors at the approach-1 ring
(hydia_params_for_approach(1): N = 2^16, 14 + 5 limbs), time indexScenario with warm-up and print ONE JSON line: ms per query (mean,
min, max, standard deviation over the timed steps), vectors/s, the split into similarity / merge / comparator by HIP events on the
library's stream, and the byte ledger's inherent bytes (op:*) of one query.  The fused paths are switched by the environment
(HYDIA_BASE_NO_ROTADD, HYDIA_BASE_NO_BCAST, HYDIA_BASE_CHUNK); the line records what was set.  Results are checked: the index is
the planted matches.

--approach 2 runs GROTE group testing (GroteSender / GroteReceiver) on its own chain (hydia_params_for_approach(2): 19 + 6 limbs) over
the same kind of database: the line then also splits the alpha norm (grote_alpha / grote_rows / grote_cols / grote_compare) and records
HYDIA_GROTE_NO_SQ.  One match is planted there: group testing answers several matches of one matrix with all their crossings.

--approach 3 runs the Blind-Match method (BlindEnroller / BlindReceiver / BlindSender) on its own chain (hydia_params_for_approach(3): 13
+ 5 limbs) over a chunk-packed database (chunk_len 128): the split is blind_similarity / blind_compress / blind_compare, and the line
records HYDIA_BLIND_NO_DOT and HYDIA_BLIND_PASS.  The planted matches come back in the order decryptIndex walks the compressed slots."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_matching_amd as im  # noqa: E402

PHASES = {1: ("base_similarity", "base_merge", "base_compare"),
          2: ("base_similarity", "base_merge", "grote_alpha", "grote_rows", "grote_cols", "grote_compare"),
          3: ("blind_similarity", "blind_compress", "blind_compare")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--approach", type=int, default=1, choices=(1, 2, 3))
    ap.add_argument("--log2n", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log-n", type=int, default=0, help="ring override for a quick look (0 = the approach's own ring)")
    ap.add_argument("--dim", type=int, default=512)
    args = ap.parse_args()
    p = im.params_for_approach(args.approach)
    if args.log_n:
        p.log_n = args.log_n
    p.vector_dim = args.dim
    cc = im.Context(p, 0)
    cc.keygen_rotations(cc.base_rotations(), seed=20250725)
    n = 1 << args.log2n
    rng = np.random.default_rng(args.log2n)
    db = rng.integers(-99, 100, size=(n, args.dim), dtype=np.int8).astype(np.float64)
    planted = [n // 2 + 1] if args.approach == 2 else sorted(set([0, n // 2, n - 1]))
    for i in planted:
        db[i] = rng.integers(1, 4, size=args.dim)
    query = np.ones(args.dim)
    t0 = time.time()
    (im.BlindEnroller if args.approach == 3 else im.BaseEnroller)(cc, n).serializeDB(db, seed=3)
    cc.sync()
    enroll_s = time.time() - t0
    receiver, sender = {1: (im.BaseReceiver, im.BaseSender), 2: (im.GroteReceiver, im.GroteSender), 3: (im.BlindReceiver, im.BlindSender)}[args.approach]
    receiver, sender = receiver(cc, n), sender(cc, n)
    q = receiver.encryptQuery(query, seed=5)
    for _ in range(args.warmup):
        idx = sender.indexScenario(q)
    cc.sync()
    cc.kernel_time_reset()
    ms = []
    for _ in range(args.steps):
        t0 = time.time()
        idx = sender.indexScenario(q)
        cc.sync()
        ms.append((time.time() - t0) * 1e3)
    split = {k: round(cc.kernel_time(k)[0] / args.steps, 3) for k in PHASES[args.approach]}
    ok = sorted(receiver.decryptIndex(idx)) == planted
    im.byte_ledger(1)
    idx = sender.indexScenario(q)
    cc.sync()
    led = im.byte_ledger(0)
    ops = {k: b for k, (_, b) in led.items() if k.startswith("op:")}
    launches = sum(c for k, (c, _) in led.items() if not k.startswith("op:"))
    mean = float(np.mean(ms))
    env = {k: os.environ[k] for k in ("HYDIA_BASE_NO_ROTADD", "HYDIA_BASE_NO_BCAST", "HYDIA_BASE_CHUNK", "HYDIA_GROTE_NO_SQ", "HYDIA_BLIND_NO_DOT",
                                          "HYDIA_BLIND_PASS") if k in os.environ}
    print(json.dumps({
        "metric": "approach%d_index_scenario" % args.approach, "log2n": args.log2n, "n": n, "ring_log_n": int(p.log_n), "vector_dim": args.dim,
        "db_cts": cc.db_stats()[1], "db_bytes": cc.db_stats()[2], "env": env, "steps": args.steps, "warmup": args.warmup,
        "ms_per_query": round(mean, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "ms_std": round(float(np.std(ms)), 3),
        "vectors_per_s": round(n / mean * 1e3, 1), "split_ms": split, "enroll_s": round(enroll_s, 2), "correct": bool(ok),
        "ledger_op_bytes": round(sum(ops.values())), "ledger_ops": {k: round(v) for k, v in sorted(ops.items())},
        "kernel_launches": launches, "version": im.load_library().hydia_version().decode()}), flush=True)
    cc.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
