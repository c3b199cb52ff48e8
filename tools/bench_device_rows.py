#!/usr/bin/env python3
"""What templates in device memory (hydia_dev_rows) buy, measured and not gated.  Full ring (N = 2^15, 512-dim vectors, 16384 vectors
per block) unless told otherwise.  Host clock around calls that end in a device synchronise; the spread is min / median / max.
  1. hydia_rows_widen_device at --rows x dim for each element type, with and without normalisation, beside a device-to-device copy
     of the same bytes (read n dim sizeof(T) + write n dim 8) in the same process
  2. enrolment of --rows rows from an f32 tensor (hydia_db_enroll_device) against hydia_db_enroll from host doubles, and the same for
     the plain gallery
  3. --probes probes at one block: hydia_encode_queries_device + indexScenarioPlainMulti against --probes hydia_encode_query + the
     same batch; the same for encrypted probes against a plain gallery (hydia_encrypt_queries_device + indexScenarioGalleryMulti)
The host legs of 2 and 3 run on the built checkout --parent-root names (the parent commit's package and library) when given, else on
this tree's.  Every leg is a child process of its own (one library per process), and the legs alternate: tree, parent, tree,
parent ... --rounds times, all in one session.  One JSON line per child and one summary line at the end."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3), "n": len(xs)}


def timed(cc, fn):
    import torch
    torch.cuda.synchronize()
    cc.sync()
    t0 = time.perf_counter()
    fn()
    cc.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def leg_widen(args):
    import torch
    import image_matching_amd as im
    cc = im.Context(im.default_params(log_n=args.log_n, vector_dim=args.dim), 0)
    n, dim = args.rows, args.dim
    out = {"leg": "widen", "rows": n, "dim": dim}
    src64 = torch.randn((n, dim), dtype=torch.float64, device="cuda")
    for name, tt in (("f64", torch.float64), ("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        t = src64.to(tt)
        moved = n * dim * (t.element_size() + 8)
        # the copy of the same bytes: the source onto itself-sized scratch plus a double buffer onto another
        a, b = torch.empty_like(t), torch.empty((n, dim), dtype=torch.float64, device="cuda")
        c = torch.empty_like(b)

        def copy():
            a.copy_(t)        # reads and writes n dim sizeof(T)
            c.copy_(b)        # reads and writes n dim 8
        # (the copy moves 2 n dim (sizeof(T) + 8) bytes: twice the kernel's, so its rate is computed over twice the bytes)
        for fn in (copy, lambda: cc.rows_widen_device(t, True), lambda: cc.rows_widen_device(t, False)):
            fn()
        t_copy, t_norm, t_plain = [], [], []
        for _ in range(args.reps):
            t_copy.append(timed(cc, copy))
            t_norm.append(timed(cc, lambda: cc.rows_widen_device(t, True)))
            t_plain.append(timed(cc, lambda: cc.rows_widen_device(t, False)))
        gbs = lambda ms, bytes_: round(bytes_ / (ms * 1e-3) / 1e9, 1)  # noqa: E731
        out[name] = {"bytes_moved": moved, "normalise_ms": spread(t_norm), "widen_only_ms": spread(t_plain), "copy_ms": spread(t_copy),
                     "normalise_gb_per_s": gbs(spread(t_norm)["median"], moved), "widen_only_gb_per_s": gbs(spread(t_plain)["median"], moved),
                     "copy_gb_per_s": gbs(spread(t_copy)["median"], 2 * moved)}
    # (both widen timings include the allocation of the output tensor by the caching allocator and one host synchronise)
    cc.close()
    return out


def leg_enroll(args):
    import torch
    import image_matching_amd as im
    cc = im.Context(im.default_params(log_n=args.log_n, vector_dim=args.dim), 0)
    cc.keygen(20250725)
    n, dim = args.rows, args.dim
    rng = np.random.default_rng(1)
    db32 = rng.standard_normal((n, dim)).astype(np.float32)
    seeds = iter(range(1000, 100000))
    enr, penr = im.DiagonalEnroller(cc, n), im.PlainEnroller(cc, n)
    out = {"leg": "enroll", "source": args.source, "rows": n, "dim": dim}
    if args.source == "device":
        t = torch.from_numpy(db32).cuda()
        runs = {"enroll_ms": lambda: enr.serializeDB(t, seed=next(seeds)), "plain_enroll_ms": lambda: penr.serializeDB(t)}
    else:
        # what a caller with an f32 tensor on the GPU does without this feature: copy to the host, widen, enrol (which normalises)
        t = torch.from_numpy(db32).cuda()

        def host_enroll(e, **kw):
            e.serializeDB(t.cpu().numpy().astype(np.float64), **kw)
        runs = {"enroll_ms": lambda: host_enroll(enr, seed=next(seeds)), "plain_enroll_ms": lambda: host_enroll(penr)}
    for k, fn in runs.items():
        fn()
        out[k] = spread([timed(cc, fn) for _ in range(args.reps)])
    out["kind"] = cc.db_kind()
    cc.close()
    return out


def leg_queries(args):
    import torch
    import image_matching_amd as im
    cc = im.Context(im.default_params(log_n=args.log_n, vector_dim=args.dim), 0)
    cc.keygen(20250725)
    n, dim, Q = cc.N // 2, args.dim, args.probes
    rng = np.random.default_rng(2)
    db = rng.standard_normal((n, dim))
    probes16 = torch.from_numpy(rng.standard_normal((Q, dim))).cuda().to(torch.float16)
    receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
    out = {"leg": "queries", "source": args.source, "probes": Q, "vectors": n, "dim": dim}
    seeds = iter(range(1000, 100000))

    def encode():
        if args.source == "device":
            return sender.encodeQueries(probes16)
        host = probes16.cpu().numpy().astype(np.float64)
        return [sender.encodeQuery(row) for row in host]

    def encrypt():
        if args.source == "device":
            return receiver.encryptQueries(probes16, seed=next(seeds), nonce0=1)
        host = probes16.cpu().numpy().astype(np.float64)
        s = next(seeds)
        return [receiver.encryptQuery(row, seed=s, nonce=1 + i) for i, row in enumerate(host)]

    for name, make, enrol, serve in (("plain_query", encode, lambda: im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=9), sender.indexScenarioPlainMulti),
                                     ("plain_gallery", encrypt, lambda: im.PlainEnroller(cc, n).serializeDB(db.copy()), sender.indexScenarioGalleryMulti)):
        enrol()
        serve(make())
        t_make, t_all = [], []
        for _ in range(args.reps):
            t_make.append(timed(cc, make))
            t_all.append(timed(cc, lambda: serve(make())))
        out[name] = {"make_queries_ms": spread(t_make), "make_and_serve_ms": spread(t_all),
                     "make_share": round(spread(t_make)["median"] / spread(t_all)["median"], 4)}
    cc.close()
    return out


LEGS = {"widen": leg_widen, "enroll": leg_enroll, "queries": leg_queries}


def child(args, leg, source, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--source", source, "--log-n", str(args.log_n), "--dim", str(args.dim),
           "--rows", str(args.rows), "--probes", str(args.probes), "--reps", str(args.reps)] + (["--root", lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("leg %s/%s failed (%d): %s" % (leg, source, r.returncode, r.stderr[-2000:]))
    line = json.loads(r.stdout.strip().splitlines()[-1])
    line["library"] = "parent" if lib else "tree"
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=15)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--rows", type=int, default=1 << 17)
    ap.add_argument("--probes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the tree and parent legs")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit for the host legs")
    ap.add_argument("--root", default=None, help="(a child's) checkout to import image_matching_amd from")
    ap.add_argument("--leg", choices=sorted(LEGS), default=None)
    ap.add_argument("--source", choices=["device", "host"], default="device")
    ap.add_argument("--only", default="widen,enroll,queries")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    if args.leg:
        print(json.dumps(LEGS[args.leg](args)), flush=True)
        return
    only = args.only.split(",")
    lines = []
    if "widen" in only:
        lines.append(child(args, "widen", "device", None))
    for leg in ("enroll", "queries"):
        if leg not in only:
            continue
        for _ in range(args.rounds):
            lines.append(child(args, leg, "device", None))
            lines.append(child(args, leg, "host", args.parent_root))
    summary = {"summary": True, "host_legs_on_parent": bool(args.parent_root)}
    for leg, keys in (("enroll", ("enroll_ms", "plain_enroll_ms")), ("queries", ("plain_query", "plain_gallery"))):
        for k in keys:
            med = {}
            for src in ("device", "host"):
                xs = [ln[k] for ln in lines if ln.get("leg") == leg and ln.get("source") == src]
                if xs:
                    med[src] = [x["median"] if "median" in x else x["make_queries_ms"]["median"] for x in xs]
            if len(med) == 2:
                summary[k] = {"device_medians_ms": med["device"], "host_medians_ms": med["host"],
                              "host_over_device": round(float(np.median(med["host"]) / np.median(med["device"])), 2)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
