"""Host check of the N = 2^16 transform schedule (image_matching_amd/csrc/ntt16_sched.h, the header the kernels of ntt16.hip are built
from): tests/csrc/ntt16_arith_check.cpp drives FpA, IntP and IntA through the stage / fold / re-centre schedule of the two kernels on
worst-case rows for the edge primes of the ring, compares with a plain __int128 transform and asserts the lazy bounds the file header
of ntt16.hip derives for 8 + 8 stages."""
import os
import subprocess

from conftest import ROOT


def test_ntt16_schedule_against_int128(tmp_path):
    """Edge primes of 2^16 (the six IntP primes, the lean-threshold pair, the top 47-bit prime, ~2^30, and the three IntA edges) plus
    three default 45-bit scaling primes of the approach-3 chain.  Compiled without FMA contraction so the doubles round as the device's
    do; prints the largest magnitude seen per modulus and per class."""
    import oracle_lib as O
    exe = tmp_path / "ntt16_arith_check"
    src = os.path.join(ROOT, "tests", "csrc", "ntt16_arith_check.cpp")
    inc = os.path.join(ROOT, "image_matching_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", inc, src, "-o", str(exe)], check=True)
    P = O.Params(log_n=16, depth=12, dim=512)
    chain = [int(q) for q in P.moduli[1:4]]
    P.close()
    out = subprocess.run([str(exe)] + [str(q) for q in chain], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "ntt16 schedule ok" in out.stdout, out.stdout + out.stderr
    for cls in ("FpA lean", "FpA non-lean", "IntP", "IntA"):
        assert "worst " + cls in out.stdout
    # the edge primes the GPU test's chain names
    for q in (37383392985089, 37383395868673, 140737487306753, 1073872897, 140737488486401, 576460752300015617, (1 << 60) - 0x101ffff):
        assert "q=%d " % q in out.stdout, q
