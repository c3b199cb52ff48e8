"""Host check of the device arithmetic header (image_matching_amd/csrc/devmath.h) against unsigned __int128 %: single-word
Barrett, Shoup, reduce64, double-word Barrett and the four-product lazy-sum reduction, on the engine's moduli and at range edges."""
import os
import subprocess

from conftest import ROOT


def test_devmath_against_int128(tmp_path):
    exe = tmp_path / "devmath_check"
    src = os.path.join(ROOT, "tests", "csrc", "devmath_check.cpp")
    inc = os.path.join(ROOT, "image_matching_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", inc, src, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "devmath ok" in out.stdout, out.stdout + out.stderr


def test_database_address_map_is_a_bijection(tmp_path):
    """image_matching_amd/csrc/db_layout.h on the host: both resident layouts tile the allocation exactly (no overlap, no hole), and in
    the group-sequential one a loop-B workgroup's bytes are one contiguous run — the property the layout exists for."""
    exe = tmp_path / "db_layout_check"
    src = os.path.join(ROOT, "tests", "csrc", "db_layout_check.cpp")
    inc = os.path.join(ROOT, "image_matching_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", inc, src, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "db layout ok" in out.stdout, out.stdout + out.stderr


def test_ntt_arith_against_int128(tmp_path):
    """image_matching_amd/csrc/ntt_arith.h on the host (tests/csrc/ntt_arith_check.cpp): the IntA, IntP and FpA butterfly arithmetics
    against exact integer arithmetic at the edges of their prime classes — every IntP prime at N = 2^15 and the extreme ones at
    N = 2^11, FP64 primes at the lean threshold and at 47 bits, 48- to 60-bit Harvey primes — and on the default chain.  Compiled
    without FMA contraction so the doubles round as the device's do; prints each modulus and the worst bound observed per class."""
    import oracle_lib as O
    exe = tmp_path / "ntt_arith_check"
    src = os.path.join(ROOT, "tests", "csrc", "ntt_arith_check.cpp")
    inc = os.path.join(ROOT, "image_matching_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", inc, src, "-o", str(exe)], check=True)
    P = O.Params()
    chain = sorted({int(q) for q in P.moduli})
    P.close()
    out = subprocess.run([str(exe)] + [str(q) for q in chain], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "ntt_arith ok" in out.stdout, out.stdout + out.stderr
    for cls in ("IntA", "IntP", "FpA"):
        assert "worst " + cls in out.stdout
