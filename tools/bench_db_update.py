#!/usr/bin/env python3
"""In-place database update (hydia_db_update) against the only thing there was before it, a whole re-enrolment.  Full ring
(N = 2^15, 512-dim vectors, 16384 vectors per block) unless told otherwise.  Times, each over --reps repeats after a warm-up of every
shape, host clock around calls that end in a device synchronise:
  (a) an update of one full block inside a resident database of --blocks blocks
  (b) an append of one block that grows the database from --blocks to --blocks + 1 (second buffer, old ciphertexts moved)
  (c) hydia_db_enroll of all --blocks and of all --blocks + 1 blocks
and the accumulate kernels' own time (hydia_kernel_time "db_accumulate": device events around k_db_accumulate + k_db_accumulate46)
beside the bytes they must move — resident bytes read and written plus the fresh ciphertexts read — as GB/s, next to what
tools/ubench/stream_rate measures in the same session when that binary is built (hipcc --offload-arch=gfx950 -O3 -o
tools/ubench/stream_rate tools/ubench/stream_rate.hip).  One JSON line at the end; the spread is min / median / max."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import image_matching_amd as im  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3), "n": len(xs)}


def timed(cc, fn):
    cc.sync()
    t0 = time.perf_counter()
    fn()
    cc.sync()
    return (time.perf_counter() - t0) * 1e3


def stream_rate_lines():
    exe = os.path.join(ROOT, "tools", "ubench", "stream_rate")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)  # a child of its own, before this process opens the GPU
    if out.returncode != 0:
        return ["stream_rate failed: " + out.stderr.strip()[-200:]]
    keep = [ln.strip() for ln in out.stdout.splitlines() if ln.startswith("seq ") or "workgroup-sequential layout:" in ln or "46-bit residues" in ln]
    return [ln for ln in keep if not ln.startswith("[")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=15)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-stream-rate", action="store_true")
    args = ap.parse_args()
    stream = None if args.no_stream_rate else stream_rate_lines()
    cc = im.Context(im.default_params(log_n=args.log_n, vector_dim=args.dim), 0)
    cc.keygen(20250725)
    S, dim, G = cc.N // 2, args.dim, args.blocks
    rng = np.random.default_rng(1)
    db = rng.integers(-99, 100, size=((G + 1) * S, dim), dtype=np.int8).astype(np.float64)
    db /= np.linalg.norm(db, axis=1, keepdims=True)  # normalised once: every timed call normalises again, which changes nothing
    seeds = iter(range(1000, 100000))  # a fresh seed per call, as a user must
    enr = im.DiagonalEnroller(cc, G * S)

    def enroll(blocks):
        enr.numVectors = blocks * S
        enr.serializeDB(db[:blocks * S], seed=next(seeds))

    def update_block(g):
        enr.updateRows(g * S, db[g * S:(g + 1) * S], True, seed=next(seeds))

    def append_block():
        enr.appendDB(db[G * S:(G + 1) * S], seed=next(seeds))

    # warm-up of every shape
    enroll(G)
    update_block(G // 2)
    append_block()
    enroll(G + 1)
    t_enroll, t_enroll1, t_update, t_append = [], [], [], []
    acc_ms, acc_launches = [], 0
    for _ in range(args.reps):
        t_enroll.append(timed(cc, lambda: enroll(G)))
        info = {"kind": cc.db_kind(), "babies": cc.db_babies(), "group": cc.db_group(), "residue_bits": cc.db_residue_bits()}
        n_vec, n_cts, db_bytes = cc.db_stats()
        cc.kernel_time_reset()
        t_update.append(timed(cc, lambda: update_block(G // 2)))
        ms, launches = cc.kernel_time("db_accumulate")
        acc_ms.append(ms)
        acc_launches = launches
        t_append.append(timed(cc, append_block))
        info_grown = {"group": cc.db_group(), "residue_bits": cc.db_residue_bits(), "n_cts": cc.db_stats()[1]}
    for _ in range(args.reps):
        t_enroll1.append(timed(cc, lambda: enroll(G + 1)))
    ct_bytes = db_bytes / n_cts
    moved = dim * (2.0 * ct_bytes + 2.0 * cc.nQ * cc.N * 8)  # one block: resident bytes read + written, fresh ciphertexts read
    rates = [moved / (ms * 1e-3) / 1e9 for ms in acc_ms]
    out = {
        "log_n": args.log_n, "dim": dim, "blocks": G, "resident": info, "after_append": info_grown,
        "update_one_block_ms": spread(t_update), "append_one_block_ms": spread(t_append),
        "enroll_%d_blocks_ms" % G: spread(t_enroll), "enroll_%d_blocks_ms" % (G + 1): spread(t_enroll1),
        "enroll_over_update": round(spread(t_enroll)["median"] / spread(t_update)["median"], 2),
        "enroll_over_append": round(spread(t_enroll1)["median"] / spread(t_append)["median"], 2),
        "accumulate_kernels_ms": spread(acc_ms), "accumulate_calls_per_update": int(acc_launches),
        "accumulate_bytes_moved": int(moved), "accumulate_gb_per_s": spread(rates),
        "accumulate_share_of_update": round(spread(acc_ms)["median"] / spread(t_update)["median"], 4),
        "stream_rate": stream,
    }
    print(json.dumps(out), flush=True)
    cc.close()


if __name__ == "__main__":
    main()
