#!/usr/bin/env python3
"""NTT microbenchmark: ms and TB/s per limb-transform, forward and inverse, at several batch sizes.
--log-n 15 (default): the FP64 limbs (one-pass vs HYDIA_NTT_2PASS=1) and the 60-bit limbs of the default chain; algorithmic bytes =
512 KiB per limb-transform.
--log-n 16: the chain of hydia_params_for_approach(3) (13 + 5 limbs) through whatever hydia_ntt_engine names — the two-pass kernels of
ntt16.hip, or the ring-size-generic ones under HYDIA_NTT_GENERIC=1; 1 MiB per limb-transform."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_matching_amd as im  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=15, choices=(15, 16))
args = ap.parse_args()

if args.log_n == 15:
    if not os.environ.get("HYDIA_NTT_2PASS"):
        os.environ.setdefault("HYDIA_NTT_1PASS", "1")
    os.environ.setdefault("HYDIA_NTT_1PASS_MIN", "1")  # the microbenchmark compares the kernels at every batch size
    cc = im.Context()
    tag = "2-pass" if os.environ.get("HYDIA_NTT_2PASS") else "1-pass"
    groups = (("fp64 limbs 1-11", 1, 11, tag), ("60-bit q0+P", 12, 4, "2-pass"))
    each = "512 KiB"
else:
    cc = im.Context(im.params_for_approach(3))
    # (getattr: the tool also runs against a library from before hydia_ntt_engine — the A/B partner — whose 2^16 transforms are generic)
    tag = "ntt16" if getattr(cc, "ntt_engine", 0) == 16 else "generic"
    groups = (("fp64 limbs 1-12", 1, cc.nQ - 1, tag), ("60-bit P limbs", cc.nQ, cc.nP, tag))  # (q0, limb 0, is in neither group)
    each = "1 MiB"
for polys in (2, 64, 1024):
    for name, first, cnt, t in groups:
        for inv in (False, True):
            ms = cc.bench_ntt(polys, first, cnt, inv, 20 if polys < 1024 else 5)
            lp = polys * cnt
            print("%-7s %-16s %s polys=%5d: %8.3f ms  %7.3f us/limb-poly  %6.2f TB/s algorithmic (%s each)"
                  % (t, name, "inv" if inv else "fwd", polys, ms, ms * 1e3 / lp, lp * cc.N * 16 / ms / 1e9, each), flush=True)
cc.close()
