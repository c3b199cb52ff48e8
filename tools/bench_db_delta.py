#!/usr/bin/env python3
"""What a database delta costs (include/hydia.h "database deltas"), measured and not gated.  Default parameters (N = 2^15, 512-dim
vectors: blocks of 16384 vectors, 512 ciphertexts each), --blocks resident hoisted blocks of random residues, ONE block of 16384 rows
updated inside them.  Times are per call on the host clock, through the C entry points into buffers allocated once (pageable host
memory, as a caller's); every call ends in a device synchronise.  Spread: min / median / max.
  delta    hydia_db_delta_make and hydia_db_delta_apply of the block, and beside them hydia_db_update of the same rows in the same session
  update   hydia_db_update of the same rows on this tree's library and on the built checkout --parent-root names (the parent commit),
           alternating over --repeats child processes each
  kernels  hydia_kernel_time and the byte ledger of k_wire_check, k_db_accumulate_wire and k_db_store_wire (a delta that appends a block)
           beside a device-to-device copy of as many bytes
  --seeded the seeded delta (include/hydia.h "seeded database deltas") beside the whole one, on this tree's library alone:
           seeded   hydia_db_delta_make_seeded / _apply_seeded and hydia_db_delta_make / _apply of the same block, alternating in ONE
                    process over --repeats repeats (medians of --calls calls each), and the bytes of both messages
           kernels_seeded   hydia_kernel_time and the byte ledger of k_wire_check, k_db_accumulate_seeded and k_db_store_seeded (a seeded
                    delta that adds to the last block and creates the next one), beside the whole delta's kernels in the same process and
                    a device-to-device copy of as many bytes
The seeds repeat from call to call: a measurement, never a deployment (include/hydia.h, SEED).  Every leg is a child process of its own
(one library per process).  One JSON line per child."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_wire_check", "k_db_accumulate_wire", "k_db_store_wire"]


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3), "n": len(xs)}


def timed(fn, calls):
    fn()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def setup(args):
    """a context with the receiver's public key, --blocks hoisted blocks of random residues resident, and one block of rows"""
    import image_matching_amd as im
    cc = im.Context(im.default_params(log_n=args.log_n, vector_dim=args.dim), 0)
    cc.keygen_rotations([], 7)
    cc.set_matvec("hoisted")
    cc.db_fill_random(args.blocks * cc.slots, 5)
    rows = np.random.default_rng(1).integers(-99, 100, size=(cc.slots, cc.dim)).astype(np.float64)
    seed = np.frombuffer((9).to_bytes(32, "little"), dtype=np.uint8).copy()
    return im, cc, rows, seed


def leg_update(args):
    im, cc, rows, seed = setup(args)
    first = (args.blocks // 2) * cc.slots

    def update():
        assert cc.L.hydia_db_update(cc.h, first, p(rows), rows.shape[0], 1, p(seed)) == 0
    out = {"leg": "update", "blocks": args.blocks, "rows": rows.shape[0], "db_update_ms": timed(update, args.calls),
           "group": cc.db_group(), "residue_bits": cc.db_residue_bits()}
    cc.close()
    return out


def leg_delta(args):
    im, cc, rows, seed = setup(args)
    first = (args.blocks // 2) * cc.slots
    need = cc.db_delta_bytes(first, rows.shape[0])
    buf, ln = np.empty(need, dtype=np.uint8), C.c_size_t()

    def make():
        assert cc.L.hydia_db_delta_make(cc.h, first, p(rows), rows.shape[0], 1, p(seed), cc.dim, 0, p(buf), buf.size, C.byref(ln)) == 0

    def apply():
        assert cc.L.hydia_db_delta_apply(cc.h, p(buf), ln.value) == 0

    def update():
        assert cc.L.hydia_db_update(cc.h, first, p(rows), rows.shape[0], 1, p(seed)) == 0
    out = {"leg": "delta", "blocks": args.blocks, "rows": rows.shape[0], "delta_bytes": need, "group": cc.db_group(), "residue_bits": cc.db_residue_bits()}
    out["db_delta_make_ms"] = timed(make, args.calls)
    out["db_delta_apply_ms"] = timed(apply, args.calls)
    out["db_update_ms"] = timed(update, args.calls)
    cc.close()
    return out


def leg_kernels(args):
    import torch  # (before the context: torch finds no device once the library has opened it)
    torch.zeros(1, device="cuda")
    im, cc, rows, seed = setup(args)
    first = args.blocks * cc.slots - 100  # the last 100 slots of the last block and a new block: one accumulate, one store per delta
    need = cc.db_delta_bytes(first, rows.shape[0])
    buf, ln = np.empty(need, dtype=np.uint8), C.c_size_t()
    out = {"leg": "kernels", "blocks": args.blocks}
    im.byte_ledger(1)
    cc.kernel_time_reset()
    for k in range(args.calls):
        fv = first + k * cc.slots
        assert cc.L.hydia_db_delta_make(cc.h, fv, p(rows), rows.shape[0], 1, p(seed), cc.dim, 0, p(buf), buf.size, C.byref(ln)) == 0
        assert cc.L.hydia_db_delta_apply(cc.h, p(buf), ln.value) == 0
    ledger = im.byte_ledger(0)
    for name in KERNELS + ["k_wire_pack"]:
        ms, launches = cc.kernel_time(name)
        n, nbytes = ledger.get(name, (0, 0.0))
        per = ms / max(launches, 1)
        out[name] = {"ms_per_launch": round(per, 4), "launches": launches, "ledger_bytes_per_launch": int(nbytes / max(n, 1)),
                     "tb_per_s": round(nbytes / max(n, 1) / (per * 1e-3) / 1e12, 3) if per > 0 else None}
    stats = cc.db_stats()
    out["blocks_after"], out["group_after"] = stats[1] // cc.dim, cc.db_group()
    cc.close()
    # a device copy that reads and writes what the fused apply kernel reads and writes of one block, and one of what the check reads
    for name in ("k_db_accumulate_wire", "k_wire_check"):
        nbytes = out[name]["ledger_bytes_per_launch"]
        half = max(nbytes // 2, 8)
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        copies = []
        for _ in range(args.calls + 1):
            a.record()
            dst.copy_(src)
            b.record()
            b.synchronize()
            copies.append(a.elapsed_time(b))
        ms = spread(copies[1:])
        out["device_copy_of_%s_bytes" % name] = {"bytes_moved": 2 * half, "ms": ms, "tb_per_s": round(2 * half / (ms["median"] * 1e-3) / 1e12, 3)}
        del src, dst
    return out


def leg_seeded(args):
    im, cc, rows, seed = setup(args)  # (keygen_rotations: the secret key is on the context)
    a_seed = np.frombuffer((10).to_bytes(32, "little"), dtype=np.uint8).copy()
    first = (args.blocks // 2) * cc.slots
    need_w, need_s = cc.db_delta_bytes(first, rows.shape[0]), cc.db_delta_seeded_bytes(first, rows.shape[0])
    buf_w, buf_s, ln_w, ln_s = np.empty(need_w, dtype=np.uint8), np.empty(need_s, dtype=np.uint8), C.c_size_t(), C.c_size_t()

    def make_s():
        assert cc.L.hydia_db_delta_make_seeded(cc.h, first, p(rows), rows.shape[0], 1, p(seed), p(a_seed), cc.dim, 0, p(buf_s), buf_s.size, C.byref(ln_s)) == 0

    def apply_s():
        assert cc.L.hydia_db_delta_apply_seeded(cc.h, p(buf_s), ln_s.value) == 0

    def make_w():
        assert cc.L.hydia_db_delta_make(cc.h, first, p(rows), rows.shape[0], 1, p(seed), cc.dim, 0, p(buf_w), buf_w.size, C.byref(ln_w)) == 0

    def apply_w():
        assert cc.L.hydia_db_delta_apply(cc.h, p(buf_w), ln_w.value) == 0
    out = {"leg": "seeded", "blocks": args.blocks, "rows": rows.shape[0], "delta_bytes": need_w, "seeded_delta_bytes": need_s,
           "ratio": round(need_s / need_w, 4), "group": cc.db_group(), "residue_bits": cc.db_residue_bits(), "repeats": []}
    for _ in range(args.repeats):  # seeded and whole alternate inside every repeat
        out["repeats"].append({"make_seeded_ms": timed(make_s, args.calls), "make_ms": timed(make_w, args.calls),
                               "apply_seeded_ms": timed(apply_s, args.calls), "apply_ms": timed(apply_w, args.calls)})
    for k in ("make_seeded_ms", "make_ms", "apply_seeded_ms", "apply_ms"):
        out[k + "_medians"] = [r[k]["median"] for r in out["repeats"]]
    cc.close()
    return out


def leg_kernels_seeded(args):
    import torch  # (before the context: torch finds no device once the library has opened it)
    torch.zeros(1, device="cuda")
    im, cc, rows, seed = setup(args)
    a_seed = np.frombuffer((10).to_bytes(32, "little"), dtype=np.uint8).copy()
    first = args.blocks * cc.slots - 100  # the last 100 slots of the last block and a new block: one accumulate, one store per delta
    need_w, need_s = cc.db_delta_bytes(first, rows.shape[0]), cc.db_delta_seeded_bytes(first, rows.shape[0])
    buf, ln = np.empty(need_w, dtype=np.uint8), C.c_size_t()
    out = {"leg": "kernels_seeded", "blocks": args.blocks}
    names = {"seeded": ["k_wire_check", "k_db_accumulate_seeded", "k_db_store_seeded", "k_wire_pack"],
             "whole": ["k_wire_check", "k_db_accumulate_wire", "k_db_store_wire", "k_wire_pack"]}
    for kind in ("seeded", "whole"):
        im.byte_ledger(1)
        cc.kernel_time_reset()
        for k in range(args.calls):
            fv = first + (k + (args.calls if kind == "whole" else 0)) * cc.slots
            if kind == "seeded":
                assert cc.L.hydia_db_delta_make_seeded(cc.h, fv, p(rows), rows.shape[0], 1, p(seed), p(a_seed), cc.dim, 0, p(buf), buf.size, C.byref(ln)) == 0
                assert cc.L.hydia_db_delta_apply_seeded(cc.h, p(buf), ln.value) == 0
            else:
                assert cc.L.hydia_db_delta_make(cc.h, fv, p(rows), rows.shape[0], 1, p(seed), cc.dim, 0, p(buf), buf.size, C.byref(ln)) == 0
                assert cc.L.hydia_db_delta_apply(cc.h, p(buf), ln.value) == 0
        ledger = im.byte_ledger(0)
        out[kind] = {}
        for name in names[kind]:
            ms, launches = cc.kernel_time(name)
            n, nbytes = ledger.get(name, (0, 0.0))
            per = ms / max(launches, 1)
            out[kind][name] = {"ms_per_launch": round(per, 4), "launches": launches, "ledger_bytes_per_launch": int(nbytes / max(n, 1)),
                               "tb_per_s": round(nbytes / max(n, 1) / (per * 1e-3) / 1e12, 3) if per > 0 and n else None}
    stats = cc.db_stats()
    out["blocks_after"], out["group_after"], out["seeded_delta_bytes"], out["delta_bytes"] = stats[1] // cc.dim, cc.db_group(), need_s, need_w
    cc.close()
    # a device copy that reads and writes what each seeded apply kernel reads and writes of one block, and one of what the check reads
    for name in ("k_db_accumulate_seeded", "k_db_store_seeded", "k_wire_check"):
        nbytes = out["seeded"][name]["ledger_bytes_per_launch"]
        half = max(nbytes // 2, 8)
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        copies = []
        for _ in range(args.calls + 1):
            a.record()
            dst.copy_(src)
            b.record()
            b.synchronize()
            copies.append(a.elapsed_time(b))
        ms = spread(copies[1:])
        out["device_copy_of_%s_bytes" % name] = {"bytes_moved": 2 * half, "ms": ms, "tb_per_s": round(2 * half / (ms["median"] * 1e-3) / 1e12, 3)}
        del src, dst
    return out


LEGS = {"update": leg_update, "delta": leg_delta, "kernels": leg_kernels, "seeded": leg_seeded, "kernels_seeded": leg_kernels_seeded}


def child(args, leg, root):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--log-n", str(args.log_n), "--dim", str(args.dim), "--blocks", str(args.blocks),
           "--calls", str(args.calls), "--repeats", str(args.repeats)] + (["--root", root] if root else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
    if r.returncode != 0:
        raise SystemExit("leg %s failed (%d): %s" % (leg, r.returncode, r.stderr[-2000:]))
    line = json.loads(r.stdout.strip().splitlines()[-1])
    line["library"] = "parent" if root else "tree"
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=15)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--calls", type=int, default=3, help="timed calls per figure and child")
    ap.add_argument("--repeats", type=int, default=5, help="alternations of the tree and parent children of the update leg")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit for the update leg")
    ap.add_argument("--root", default=None, help="(a child's) checkout to import image_matching_amd from")
    ap.add_argument("--leg", choices=sorted(LEGS), default=None)
    ap.add_argument("--only", default="delta,update,kernels")
    ap.add_argument("--seeded", action="store_true", help="the seeded delta beside the whole one (legs seeded and kernels_seeded) instead")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    if args.leg:
        print(json.dumps(LEGS[args.leg](args)), flush=True)
        return
    if args.seeded:
        child(args, "seeded", None)
        child(args, "kernels_seeded", None)
        return
    only = args.only.split(",")
    if "delta" in only:
        child(args, "delta", None)
    if "update" in only:
        lines = []
        for _ in range(args.repeats):
            lines.append(child(args, "update", None))
            if args.parent_root:
                lines.append(child(args, "update", args.parent_root))
        summary = {"summary": "update", "parent_measured": bool(args.parent_root)}
        for lib in ("tree", "parent"):
            med = [ln["db_update_ms"]["median"] for ln in lines if ln["library"] == lib]
            if med:
                summary["db_update_%s_medians_ms" % lib] = med
        print(json.dumps(summary), flush=True)
    if "kernels" in only:
        child(args, "kernels", None)


if __name__ == "__main__":
    main()
