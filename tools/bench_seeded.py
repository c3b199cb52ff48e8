#!/usr/bin/env python3
"""What seeded keys and queries cost and save, measured and not gated.  Full ring (N = 2^15, 512-dim vectors) unless told otherwise, one
process, one session; the two sides of every comparison alternate --reps times.  Host clock around calls that are synchronous on
return; the spread is min / median / max.
  1. --probes probes (1 and 64 by default) made into queries: hydia_encrypt_query per probe (public key) against ONE
     hydia_encrypt_queries_seeded (secret key, k_enc_sym), per probe
  2. one query into a sender's handle: hydia_ct_import of the full ciphertext against hydia_ct_expand_seeded of its c0
  3. --keys rotation keys from host memory to resident: hydia_import_eval_key of the full keys against hydia_import_eval_key_seeded of
     the halves
and the wire bytes of each.  One JSON line per comparison."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3), "n": len(xs)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def alternate(reps, a, b):
    """a(), b(), a(), b() ... after one untimed call of each; (spread of a, spread of b) in ms"""
    a(), b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a)[0])
        tb.append(timed(b)[0])
    return spread(ta), spread(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=15)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--probes", default="1,64")
    ap.add_argument("--keys", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import image_matching_amd as im
    params = im.default_params(log_n=args.log_n, vector_dim=args.dim)
    R, S = im.Context(params, 0), im.Context(params, 0)
    rots = list(range(1, args.keys + 1))
    R.keygen_rotations_seeded(rots, seed=20250725, a_seed=20250726)
    receiver, sender = im.DiagonalReceiver(R, 1), im.DiagonalSender(S, 1)
    rng = np.random.default_rng(3)
    seeds = iter(range(1000, 1000000))
    ct_bytes, half_bytes = 2 * R.nQ * R.N * 8, R.nQ * R.N * 8

    for k in [int(x) for x in args.probes.split(",")]:
        probes = rng.standard_normal((k, args.dim))

        def public():
            s = next(seeds)
            return [receiver.encryptQuery(row, seed=s, nonce=1 + i) for i, row in enumerate(probes)]

        def seeded():
            return receiver.encryptQueriesSeeded(probes, seed=next(seeds), a_seed=next(seeds), nonce0=1)
        tp, ts = alternate(args.reps, public, seeded)
        print(json.dumps({"what": "encrypt", "probes": k, "public_key_ms": tp, "seeded_ms": ts,
                          "public_key_ms_per_probe": round(tp["median"] / k, 4), "seeded_ms_per_probe": round(ts["median"] / k, 4),
                          "note": "public: the ciphertext stays in device memory; seeded: c0 is copied to host memory",
                          "wire_bytes_per_probe": {"public_key": ct_bytes, "seeded": half_bytes + 40}}), flush=True)

    probe = rng.standard_normal(args.dim)
    full = receiver.encryptQuery(probe, seed=next(seeds), nonce=1).export()
    sq = receiver.encryptQuerySeeded(probe, seed=next(seeds), a_seed=next(seeds), nonce=1)
    ti, te = alternate(args.reps, lambda: S.import_ct(full, S.delta), lambda: sender.expandQuery(sq))
    print(json.dumps({"what": "query into a handle", "ct_import_ms": ti, "ct_expand_seeded_ms": te,
                      "wire_bytes": {"ct_import": int(full.nbytes), "ct_expand_seeded": sq.nbytes}}), flush=True)

    whole = {r: R.export_eval_key(r) for r in rots}
    halves = {r: R.export_eval_key_seeded(r) for r in rots}
    a_seed = R.key_seed()

    def import_whole():
        for r in rots:
            S.import_eval_key(r, whole[r])

    def import_halves():
        for r in rots:
            S.import_eval_key_seeded(r, halves[r], a_seed)
    tw, th = alternate(args.reps, import_whole, import_halves)
    assert np.array_equal(S.export_eval_key(rots[-1]), whole[rots[-1]])
    print(json.dumps({"what": "rotation keys, host to resident", "keys": len(rots), "import_eval_key_ms": tw, "import_eval_key_seeded_ms": th,
                      "wire_bytes": {"import_eval_key": sum(int(v.nbytes) for v in whole.values()),
                                     "import_eval_key_seeded": sum(int(v.nbytes) for v in halves.values()) + 32}}), flush=True)
    R.close()
    S.close()


if __name__ == "__main__":
    main()
