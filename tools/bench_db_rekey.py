#!/usr/bin/env python3
"""Re-keying a resident database (hydia_db_rekey) beside what it replaces, hydia_db_enroll of the same rows, in one process and
session.  Full ring (N = 2^15, 512-dim vectors, 16384 vectors and 512 ciphertexts per block) unless told otherwise.  Per database size
(--blocks): the enrolment (host clock around the call, which ends in a device synchronise; --reps repeats after one warm-up), then
--warmup untimed and --reps timed re-keys with one switching key — host clock around the call, and the three phases of
hydia_kernel_time ("db_rekey_gather", "db_rekey_switch", "db_rekey_store": device events around each chunk's launches) with the bytes
the gather and store kernels must move as GB/s.  One JSON line per size; the spread is min / median / max.
--ab: the fused store against db_unpack + add + db_pack (tools/ab_rekey_store.cpp, built with --build: the unfused form lives in that
tool only), in a child process of its own BEFORE this process opens the GPU; its JSON line comes first."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AB = os.path.join(ROOT, "tools", "ab_rekey_store")


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3), "n": len(xs)}


def timed(cc, fn):
    cc.sync()
    t0 = time.perf_counter()
    fn()
    cc.sync()
    return (time.perf_counter() - t0) * 1e3


def build_ab():
    csrc = os.path.join(ROOT, "image_matching_amd", "csrc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                           AB + ".cpp", "-L", os.path.join(ROOT, "image_matching_amd"), "-lhydia", "-lpthread",
                           "-Wl,-rpath,$ORIGIN/../image_matching_amd", "-o", AB])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=15)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--blocks", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build", action="store_true", help="compile tools/ab_rekey_store and exit")
    ap.add_argument("--ab", type=int, default=0, metavar="BLOCKS", help="run the store A/B on a database of BLOCKS blocks first")
    args = ap.parse_args()
    if args.build:
        build_ab()
        return
    if args.ab:
        out = subprocess.run([AB, str(args.ab), str(args.dim), "256", str(args.reps)], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            print(json.dumps({"ab": "rekey_store", "error": (out.stderr or out.stdout).strip()[-300:]}), flush=True)
        else:
            row = json.loads(out.stdout.strip().splitlines()[-1])
            f, u = spread(row.pop("fused_ms")), spread(row.pop("unfused_ms"))
            row.update({"fused_ms": f, "unfused_ms": u, "unfused_over_fused": round(u["median"] / f["median"], 3)})
            print(json.dumps(row), flush=True)
    import image_matching_amd as im
    cc_old = im.Context(im.default_params(log_n=args.log_n, vector_dim=args.dim), 0)
    cc_old.keygen(20250725)
    cc_new = im.Context(im.default_params(log_n=args.log_n, vector_dim=args.dim), 0)
    cc_new.keygen_rotations([1], 20250726)  # the new receiver: only its secret matters here
    key = cc_new.keygen_switch(cc_old.export_secret_key(), 20250727)
    cc_new.close()
    S, dim = cc_old.N // 2, args.dim
    rng = np.random.default_rng(1)
    for G in args.blocks:
        db = rng.integers(-99, 100, size=(G * S, dim), dtype=np.int8).astype(np.float64)
        db /= np.linalg.norm(db, axis=1, keepdims=True)  # normalised once: every enrolment normalises again, which changes nothing
        enr = im.DiagonalEnroller(cc_old, G * S)
        seeds = iter(range(1000 * G, 1000 * G + 100))
        row = {"log_n": args.log_n, "dim": dim, "blocks": G, "vectors": G * S}
        try:
            enr.serializeDB(db, seed=next(seeds))  # warm-up
            t_enroll = [timed(cc_old, lambda: enr.serializeDB(db, seed=next(seeds))) for _ in range(args.reps)]
            n_vec, n_cts, db_bytes = cc_old.db_stats()
            row.update({"kind": cc_old.db_kind(), "babies": cc_old.db_babies(), "group": cc_old.db_group(), "residue_bits": cc_old.db_residue_bits(),
                        "cts": n_cts, "resident_bytes": db_bytes})
            for _ in range(args.warmup):
                cc_old.db_rekey(key)
            t_rekey, phases = [], {"db_rekey_gather": [], "db_rekey_switch": [], "db_rekey_store": []}
            chunks = 0
            for _ in range(args.reps):
                cc_old.kernel_time_reset()
                t_rekey.append(timed(cc_old, lambda: cc_old.db_rekey(key)))
                for name in phases:
                    ms, chunks = cc_old.kernel_time(name)
                    phases[name].append(ms)
            ct_bytes, plain = db_bytes / n_cts, cc_old.nQ * cc_old.N * 8
            moved = {"db_rekey_gather": n_cts * (0.5 * ct_bytes + plain), "db_rekey_store": n_cts * (1.5 * ct_bytes + 2.0 * plain)}
            row.update({"enroll_ms": spread(t_enroll), "rekey_ms": spread(t_rekey), "chunks_per_rekey": int(chunks),
                        "enroll_over_rekey": round(spread(t_enroll)["median"] / spread(t_rekey)["median"], 3),
                        "rekey_us_per_ct": round(spread(t_rekey)["median"] * 1e3 / n_cts, 2)})
            for name, xs in phases.items():
                row[name + "_ms"] = spread(xs)
                if name in moved:
                    row[name + "_gb_per_s"] = spread([moved[name] / (ms * 1e-3) / 1e9 for ms in xs])
        except im.HydiaError as e:
            row["error"] = str(e)
        print(json.dumps(row), flush=True)
        del db
    cc_old.close()


if __name__ == "__main__":
    main()
