#!/usr/bin/env python3
"""What wire messages cost and save, measured and not gated.  Full ring (N = 2^15, 512-dim vectors) unless told otherwise, one process,
one session; the two sides of every comparison alternate --reps times after one untimed call of each.  Host clock around calls that are
synchronous on return; the spread is min / median / max.
  1. --keys rotation keys from host memory to resident: hydia_key_from_wire of seeded messages against hydia_import_eval_key_seeded of
     the raw halves
  2. --probes probes encrypted: hydia_encrypt_queries_seeded_wire (one message) against hydia_encrypt_queries_seeded (raw c0)
  3. --results ciphertexts out and back: hydia_ct_to_wire + hydia_ct_from_wire against hydia_ct_export + hydia_ct_import, on 1 and n_q limbs
  4. k_wire_pack / k_wire_unpack_check: HIP-event time (hydia_kernel_time) over the byte ledger's bytes, beside a device-to-device copy
     moving the same bytes in the same run (torch, when installed)
One JSON line per comparison."""
import argparse
import ctypes as C
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
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--keys", type=int, default=32)
    ap.add_argument("--results", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    try:
        import torch
    except ImportError:
        torch = None
    import image_matching_amd as im
    params = im.default_params(log_n=args.log_n, vector_dim=args.dim)
    R, S = im.Context(params, 0), im.Context(params, 0)
    rots = list(range(1, args.keys + 1))
    R.keygen_rotations_seeded(rots, seed=20250725, a_seed=20250726)
    receiver = im.DiagonalReceiver(R, 1)
    rng = np.random.default_rng(3)
    seeds = iter(range(1000, 1000000))

    # 1. keys
    halves = {r: R.export_eval_key_seeded(r) for r in rots}
    messages = {r: R.key_to_wire(r, seeded=True) for r in rots}
    a_seed = R.key_seed()

    def from_wire():
        for r in rots:
            S.key_from_wire(messages[r])

    def from_halves():
        for r in rots:
            S.import_eval_key_seeded(r, halves[r], a_seed)
    tw, th = alternate(args.reps, from_wire, from_halves)
    from_wire()
    assert np.array_equal(S.export_eval_key(rots[-1]), R.export_eval_key(rots[-1]))
    print(json.dumps({"what": "rotation keys, host to resident", "keys": len(rots), "key_from_wire_ms": tw, "import_eval_key_seeded_ms": th,
                      "bytes": {"wire": sum(len(m) for m in messages.values()), "raw_halves": sum(int(v.nbytes) for v in halves.values()) + 32}}), flush=True)

    # 2. probes.  Both sides through the C entry points into buffers allocated once, so that no allocation or Python copy is timed
    L, vp = R.L, lambda x: x.ctypes.data_as(C.c_void_p)
    probes = np.ascontiguousarray(rng.standard_normal((args.probes, args.dim)))
    wire_buf = np.zeros(R.wire_ct_bytes(args.probes, 1, R.nQ, True), dtype=np.uint8)
    raw_buf = np.zeros((args.probes, R.nQ, R.N), dtype=np.uint64)
    written = C.c_size_t()

    def key():
        return vp(np.frombuffer(int(next(seeds)).to_bytes(32, "little"), dtype=np.uint8).copy())

    def enc_wire():
        assert L.hydia_encrypt_queries_seeded_wire(R.h, vp(probes), args.probes, key(), key(), 1, vp(wire_buf), wire_buf.size, C.byref(written)) == 0

    def enc_raw():
        assert L.hydia_encrypt_queries_seeded(R.h, vp(probes), args.probes, key(), key(), 1, vp(raw_buf)) == 0
    tq, tr = alternate(args.reps, enc_wire, enc_raw)
    print(json.dumps({"what": "probes encrypted", "probes": args.probes, "seeded_wire_ms": tq, "seeded_raw_ms": tr,
                      "bytes": {"wire": int(wire_buf.size), "raw": int(raw_buf.nbytes) + 40}}), flush=True)

    # 3. results out and back, the same way: one buffer per side, a fresh handle per repeat
    for nl in (1, R.nQ):
        data = np.stack([rng.integers(0, int(R.moduli[j]), size=(args.results, 2, R.N), dtype=np.uint64) for j in range(nl)], axis=2)
        ct = S.import_ct(data, S.delta)
        msg_buf = np.zeros(S.wire_ct_bytes(args.results, 2, nl), dtype=np.uint8)
        exp_buf = np.zeros_like(data)
        out, n_out, h = (C.c_void_p * 1)(), C.c_size_t(), C.c_void_p()

        def wire():
            assert L.hydia_ct_to_wire(S.h, ct.h, vp(msg_buf), msg_buf.size, C.byref(written)) == 0
            assert L.hydia_ct_from_wire(R.h, vp(msg_buf), msg_buf.size, out, 1, C.byref(n_out)) == 0
            return im.Ciphertext(R, C.c_void_p(out[0]))

        def raw():
            assert L.hydia_ct_export(S.h, ct.h, vp(exp_buf)) == 0
            assert L.hydia_ct_import(R.h, vp(exp_buf), args.results, 2, nl, S.delta, C.byref(h)) == 0
            return im.Ciphertext(R, C.c_void_p(h.value))
        assert np.array_equal(wire().export(), data) and np.array_equal(raw().export(), data)
        t1, t2 = alternate(args.reps, wire, raw)
        print(json.dumps({"what": "ciphertexts to the other side and back into a handle", "count": args.results, "n_limbs": nl, "wire_ms": t1,
                          "export_import_ms": t2, "bytes": {"wire": int(msg_buf.size), "raw": int(data.nbytes)}}), flush=True)

    # 4. the kernels alone: HIP events around each launch, the ledger's bytes (rows read + rows written)
    data = np.stack([rng.integers(0, int(R.moduli[j]), size=(args.results, 2, R.N), dtype=np.uint64) for j in range(R.nQ)], axis=2)
    ct = S.import_ct(data, S.delta)
    msg = ct.to_wire()
    S.ct_from_wire(msg)
    im.byte_ledger(1)
    S.kernel_time_reset()
    for _ in range(args.reps):
        ct.to_wire()
        S.ct_from_wire(msg)
    ledger = im.byte_ledger(0)
    out = {"what": "kernels", "shape": [args.results, 2, R.nQ, R.N]}
    for k in ("k_wire_pack", "k_wire_unpack_check"):
        ms, n = S.kernel_time(k)
        out[k] = {"launches": n, "ms_per_launch": round(ms / n, 4), "bytes_per_launch": ledger[k][1] / ledger[k][0],
                  "GB_per_s": round(ledger[k][1] / ms / 1e6, 1)}
    if torch is not None:
        half = int(ledger["k_wire_pack"][1] / ledger["k_wire_pack"][0]) // 2  # a copy of `half` bytes reads and writes the same total
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda:0"), torch.empty(half, dtype=torch.uint8, device="cuda:0")
        dst.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / args.reps
        out["device_copy"] = {"bytes_moved": 2 * half, "ms": round(ms, 4), "GB_per_s": round(2 * half / ms / 1e6, 1)}
    print(json.dumps(out), flush=True)
    R.close()
    S.close()


if __name__ == "__main__":
    main()
