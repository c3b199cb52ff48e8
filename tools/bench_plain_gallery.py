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
(profiles/plain_gallery_batch/README.md).

--update: the gallery only — the in-place update (hydia_plain_db_update) against the only thing there was before it, a whole
re-enrolment, mirroring tools/bench_db_update.py.  Full ring, --blocks blocks (16), --reps repeats (5) after a warm-up of every shape,
host clock around calls that end in a device synchronise:
  (a) an update of one full block inside the resident gallery
  (b) an append of one block that grows the gallery from --blocks to --blocks + 1 (second buffer, old plaintexts moved)
  (c) hydia_plain_db_enroll of all --blocks and of all --blocks + 1 blocks
the accumulate kernels' own time (hydia_kernel_time "db_accumulate": k_plain_db_accumulate + k_plain_db_accumulate46) beside the bytes
they must move — one polynomial read and written plus n_q N 8 fresh bytes read per entry — as GB/s, next to what tools/ubench/stream_rate
measures in the same session when that binary is built, and the wall time of hydia_plain_db_save / hydia_plain_db_load of the --blocks
blocks in --file-dir (the file system is named).  One JSON line at the end; the spread is min / median / max."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def file_system_of(path):
    """the mount point, type and device the path lies on (the longest mount point that is a prefix of it)"""
    path, best = os.path.realpath(path), None
    try:
        for ln in open("/proc/mounts"):
            dev, mnt, typ = ln.split()[:3]
            if (path == mnt or path.startswith(mnt.rstrip("/") + "/")) and (best is None or len(mnt) > len(best[1])):
                best = (dev, mnt, typ)
    except OSError:
        pass
    return None if best is None else {"device": best[0], "mount": best[1], "type": best[2]}


def main_update(args):
    stream = None if args.no_stream_rate else stream_rate_lines()
    cc = im.Context()  # nothing is encrypted and no query is served: no key is needed
    S, dim, G = cc.N // 2, cc.dim, args.blocks
    rng = np.random.default_rng(1)
    db = rng.integers(-99, 100, size=((G + 1) * S, dim), dtype=np.int8).astype(np.float64)
    db /= np.linalg.norm(db, axis=1, keepdims=True)  # normalised once: every timed call normalises again, which changes nothing
    enr = im.PlainEnroller(cc, G * S)

    def enroll(blocks):
        enr.numVectors = blocks * S
        enr.serializeDB(db[:blocks * S])

    def update_block(g):
        enr.updateRows(g * S, db[g * S:(g + 1) * S], True)

    def append_block():
        enr.appendDB(db[G * S:(G + 1) * S])

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
        n_vec, n_pts, db_bytes = cc.db_stats()
        cc.kernel_time_reset()
        t_update.append(timed(cc, lambda: update_block(G // 2)))
        ms, launches = cc.kernel_time("db_accumulate")
        acc_ms.append(ms)
        acc_launches = launches
        t_append.append(timed(cc, append_block))
        info_grown = {"group": cc.db_group(), "residue_bits": cc.db_residue_bits(), "n_pts": cc.db_stats()[1]}
    for _ in range(args.reps):
        t_enroll1.append(timed(cc, lambda: enroll(G + 1)))
    pt_bytes = db_bytes / n_pts
    moved = dim * (2.0 * pt_bytes + 1.0 * cc.nQ * cc.N * 8)  # one block: one polynomial read + written, the fresh residues read
    rates = [moved / (ms * 1e-3) / 1e9 for ms in acc_ms]
    out = {
        "log_n": 15, "dim": dim, "blocks": G, "resident": info, "after_append": info_grown,
        "update_one_block_ms": spread(t_update), "append_one_block_ms": spread(t_append),
        "enroll_%d_blocks_ms" % G: spread(t_enroll), "enroll_%d_blocks_ms" % (G + 1): spread(t_enroll1),
        "enroll_over_update": round(spread(t_enroll)["median"] / spread(t_update)["median"], 2),
        "enroll_over_append": round(spread(t_enroll1)["median"] / spread(t_append)["median"], 2),
        "accumulate_kernels_ms": spread(acc_ms), "accumulate_calls_per_update": int(acc_launches),
        "accumulate_bytes_moved": int(moved), "accumulate_gb_per_s": spread(rates),
        "accumulate_share_of_update": round(spread(acc_ms)["median"] / spread(t_update)["median"], 4),
        "stream_rate": stream,
    }
    # the file: hydia_plain_db_save / hydia_plain_db_load of the G blocks, wall time
    enroll(G)
    file_bytes = 312 + n_pts * (cc.N * 8 + (cc.nQ - 1) * cc.N * 6)
    d = tempfile.mkdtemp(prefix="plain_gallery_", dir=args.file_dir)
    path = os.path.join(d, "gallery.db")
    out["file"] = {"bytes": file_bytes, "file_system": file_system_of(d)}
    try:
        free = os.statvfs(d)
        if free.f_bavail * free.f_frsize < 1.25 * file_bytes:
            out["file"]["unmeasured"] = "not enough room in " + d
        else:
            t_save, t_load = [], []
            for _ in range(args.file_reps):
                t_save.append(timed(cc, lambda: cc.plain_db_save(path)))
                t_load.append(timed(cc, lambda: cc.plain_db_load(path)))
            out["file"].update({"save_ms": spread(t_save), "load_ms": spread(t_load), "size_on_disk": os.path.getsize(path)})
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(d)
    print(json.dumps(out), flush=True)
    cc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--update", action="store_true", help="the gallery only: in-place update and append against re-enrolment, and the file")
    ap.add_argument("--blocks", type=int, default=16, help="--update: blocks resident")
    ap.add_argument("--file-dir", default=None, help="--update: where the gallery file is written (default: the system's temporary directory)")
    ap.add_argument("--file-reps", type=int, default=2, help="--update: save / load repeats")
    ap.add_argument("--no-stream-rate", action="store_true", help="--update: do not run tools/ubench/stream_rate first")
    ap.add_argument("--log2n", type=int, nargs="*", default=[14, 17, 20])
    ap.add_argument("--plain-only", type=int, nargs="*", default=[21], help="sizes run for the plain gallery alone")
    ap.add_argument("--reps", type=int, default=None, help="alternations plain / encrypted per size (3); --update: repeats (5)")
    ap.add_argument("--queries", type=int, default=5, help="timed indexScenario calls per enrolment")
    ap.add_argument("--warmup", type=int, default=2, help="--batch: untimed single calls before the timed ones")
    ap.add_argument("--batch", type=int, nargs="*", default=[], help="the gallery only: batches of these sizes beside single calls")
    ap.add_argument("--widths", type=int, nargs="*", default=[2, 4], help="--batch: queries per pass over the gallery to compare (1, 2, 4)")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 5 if args.update else 3
    if args.update:
        return main_update(args)
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
