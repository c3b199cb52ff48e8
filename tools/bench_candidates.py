#!/usr/bin/env python3
"""What the selection stage behind the decoder costs and buys (include/hydia.h "candidate lists and matches"), measured and not gated.
Full ring (N = 2^15, 16384 slots), --cts one-limb ciphertexts (64: the shape of a 2^20-vector result).  Times are per call on the host
clock, through the C entry points into buffers allocated once; every call ends in a device synchronise.  Spread: min / median / max.
  index    hydia_decrypt_index at 0, 10 and 10 000 matches — on this tree's library and on the built checkout --parent-root names (the
           parent commit, where the scan runs on the host), alternating over --repeats child processes each
  topk     hydia_decrypt + np.argpartition against hydia_decrypt_topk at k = 10 and 1000
  multi    hydia_decrypt_topk_multi of 8 results against 8 hydia_decrypt_topk calls (k = 10)
  kernels  hydia_kernel_time per launch of each new kernel beside a device-to-device copy of the same bytes (the n doubles read once)
Every leg is a child process of its own (one library per process).  One JSON line per child."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_select_count", "k_select_scan", "k_select_scatter", "k_topk_hist", "k_topk_pick"]


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 4), "median": round(xs[len(xs) // 2], 4), "max": round(xs[-1], 4), "n": len(xs)}


def timed(fn, calls):
    fn()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def setup(args, matches, seed=1):
    """a context with the receiver's keys and a one-limb result of --cts ciphertexts: uniform scores in (-0.5, 0.5) with `matches` slots
    at 2.0"""
    import image_matching_amd as im
    cc = im.Context(im.default_params(log_n=args.log_n, vector_dim=args.dim), 0)
    cc.keygen_rotations([], 7)
    rng = np.random.default_rng(seed)
    slots = rng.uniform(-0.5, 0.5, (args.cts, cc.slots))
    if matches:
        slots.reshape(-1)[rng.choice(slots.size, matches, replace=False)] = 2.0
    ct = cc.encrypt(slots, seed=seed, nonce0=1)
    cc.level_reduce(ct, 1)
    return im, cc, ct


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def leg_index(args):
    out = {"leg": "index", "cts": args.cts}
    for m in (0, 10, 10000):
        im, cc, ct = setup(args, m)
        idx, n = np.zeros(args.cts * cc.slots, dtype=np.uint64), C.c_size_t()

        def call():
            assert cc.L.hydia_decrypt_index(cc.h, ct.h, p(idx), idx.size, C.byref(n)) == 0
        out["matches_%d_ms" % m] = timed(call, args.calls)
        assert n.value == m, (n.value, m)
        del ct
        cc.close()
    return out


def leg_topk(args):
    im, cc, ct = setup(args, 10)
    out = {"leg": "topk", "cts": args.cts}
    n_all = args.cts * cc.slots
    vals = np.zeros((args.cts, cc.slots))
    for k in (10, 1000):
        idx, val, got = np.zeros(k, dtype=np.uint64), np.zeros(k), C.c_size_t()

        def host():
            assert cc.L.hydia_decrypt(cc.h, ct.h, p(vals)) == 0
            flat = vals.reshape(-1)
            part = np.argpartition(-flat, k)[:k]
            return part[np.lexsort((part, -flat[part]))]

        def device():
            assert cc.L.hydia_decrypt_topk(cc.h, ct.h, 0, k, p(idx), p(val), C.byref(got)) == 0
        out["k_%d" % k] = {"decrypt_argpartition_ms": timed(host, args.calls), "decrypt_topk_ms": timed(device, args.calls)}
        assert got.value == k and np.array_equal(np.sort(idx.astype(np.int64)), np.sort(host())), "the two paths disagree"
    out["decrypt_alone_ms"] = timed(lambda: cc.L.hydia_decrypt(cc.h, ct.h, p(vals)), args.calls)
    out["slots"] = n_all
    del ct
    cc.close()
    return out


def leg_multi(args):
    im, cc, ct = setup(args, 10)
    results = [ct] + [setup_more(cc, args, s) for s in range(2, 9)]
    k, R = 10, 8
    hs = (C.c_void_p * R)(*[r.h for r in results])
    idx, val, got = np.zeros((R, k), dtype=np.uint64), np.zeros((R, k)), np.zeros(R, dtype=np.uint64)
    one_i, one_v, one_n = np.zeros((R, k), dtype=np.uint64), np.zeros((R, k)), C.c_size_t()

    def multi():
        assert cc.L.hydia_decrypt_topk_multi(cc.h, hs, R, 0, k, p(idx), p(val), p(got)) == 0

    def singles():
        for r in range(R):
            assert cc.L.hydia_decrypt_topk(cc.h, results[r].h, 0, k, p(one_i[r]), p(one_v[r]), C.byref(one_n)) == 0
    out = {"leg": "multi", "results": R, "k": k, "multi_ms": timed(multi, args.calls), "singles_ms": timed(singles, args.calls)}
    assert np.array_equal(idx, one_i) and np.array_equal(val.view(np.uint64), one_v.view(np.uint64))
    del results, ct
    cc.close()
    return out


def setup_more(cc, args, seed):
    rng = np.random.default_rng(seed)
    ct = cc.encrypt(rng.uniform(-0.5, 0.5, (args.cts, cc.slots)), seed=seed, nonce0=1)
    cc.level_reduce(ct, 1)
    return ct


def leg_kernels(args):
    import torch  # (before the context: torch finds no device once the library has opened it)
    torch.zeros(1, device="cuda")
    im, cc, ct = setup(args, 10000)
    dev = cc.decrypt_device(ct).reshape(-1)
    n = dev.numel()
    out = {"leg": "kernels", "n": n, "bytes_read": n * 8}
    other = torch.empty_like(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copies = []
    for _ in range(args.calls + 1):
        a.record()
        other.copy_(dev)
        b.record()
        b.synchronize()
        copies.append(a.elapsed_time(b))
    out["device_copy_ms"] = spread(copies[1:])  # reads and writes n * 8 bytes: twice what a selection kernel reads
    cc.slots_topk(dev, 10)
    cc.slots_select(dev, 1.0)
    cc.kernel_time_reset()
    for _ in range(args.calls):
        cc.slots_topk(dev, 10)
        cc.slots_select(dev, 1.0)
    for name in KERNELS:
        ms, launches = cc.kernel_time(name)
        out[name] = {"ms_per_launch": round(ms / max(launches, 1), 5), "launches": launches}
    del ct
    cc.close()
    return out


LEGS = {"index": leg_index, "topk": leg_topk, "multi": leg_multi, "kernels": leg_kernels}


def child(args, leg, root):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--log-n", str(args.log_n), "--dim", str(args.dim), "--cts", str(args.cts),
           "--calls", str(args.calls)] + (["--root", root] if root else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
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
    ap.add_argument("--cts", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20, help="timed calls per figure and child")
    ap.add_argument("--repeats", type=int, default=5, help="alternations of the tree and parent children of the index leg")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit for the index leg")
    ap.add_argument("--root", default=None, help="(a child's) checkout to import image_matching_amd from")
    ap.add_argument("--leg", choices=sorted(LEGS), default=None)
    ap.add_argument("--only", default="index,topk,multi,kernels")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    if args.leg:
        print(json.dumps(LEGS[args.leg](args)), flush=True)
        return
    only = args.only.split(",")
    lines = []
    if "index" in only:
        for _ in range(args.repeats):
            lines.append(child(args, "index", None))
            if args.parent_root:
                lines.append(child(args, "index", args.parent_root))
        summary = {"summary": "index", "parent_measured": bool(args.parent_root)}
        for m in (0, 10, 10000):
            for lib in ("tree", "parent"):
                med = [ln["matches_%d_ms" % m]["median"] for ln in lines if ln["library"] == lib]
                if med:
                    summary["matches_%d_%s_medians_ms" % (m, lib)] = med
        print(json.dumps(summary), flush=True)
    for leg in ("topk", "multi", "kernels"):
        if leg in only:
            child(args, leg, None)


if __name__ == "__main__":
    main()
