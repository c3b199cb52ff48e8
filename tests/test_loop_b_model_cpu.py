"""CPU-only checks of the host side of the loop-B tests (tests/csrc/loop_b_ref.h, driven by tests/csrc/loop_b_ref_check.cpp, a
stand-alone program compiled with g++ — once plain, once under AddressSanitizer and UndefinedBehaviorSanitizer).  What the GPU file
tests/test_gpu_loop_b_edges.py compares the kernels with is pinned here without a GPU:

  * closed forms: with q - 1 on both sides every product is 1, so d0 = d2 = dim mod q and d1 = 2 dim mod q — on every limb of the
    default chain (N = 2^11 and 2^15) and of the two edge chains of tests/test_gpu_edge_primes.py, at dim 64 and 512; the
    one-by-one and the lazy branch of the recomputation agree;
  * `uniform` is k_fill_uniform_hash's hash on a few hundred indices; `holes` differs from q - 1 at between 1/32 and 1/8 of its
    positions, with special and hashed values among them; `edge` draws all of 0, 1, q - 2, q - 1;
  * the slot map is a bijection onto [0, Q G) for every (Q, G, ng) the GPU file runs, giant-major where ng > 0;
  * the range premises, in exact integers wider than the sums:

    Sums128 on the 60-bit q_0.  The kernels fold every 2^(125 - 2k) = 32 diagonals.  32 saturated Karatsuba products (2q - 2)^2
    plus a folded q - 1 stay below 2^128 — and so do 64: 64 (2q - 2)^2 + q < 256 q^2 < 2^128 for every q < 2^60.  The bound
    2^(2k+2) per product that the code budgets with is one bit above what residues below q can reach, so the "every 64 diagonals"
    that DESIGN.md and kernels.hip used to quote was wrong about the code but would not have wrapped; 65 products, and 128 (the next
    power of two), do wrap.  A fold interval of 128 is therefore the shortest wrong one, and saturated operands catch it; 128 products
    of the existing test's uniform residues (its own seeds) stay below 2^128 in every aligned run and every stride-4 run, which is
    why that test cannot.

    Halves24.  The three 64-bit partial sums of the Karatsuba term at all-ones halves: at dim 512 the widest (mid, halves of
    24 + 24 bits) takes 60 of 63 bits — THREE BITS OF MARGIN, which is all the GPU tests reach; at dim 4096 it takes all 63 (2^63
    minus 2^40), and 4097 diagonals pass 2^63: the launcher's limit is exact.  With 24 + 22-bit halves (46-bit residues) mid takes
    58 bits at dim 512 and 61 at 4096.  The 4096-diagonal limit itself is NOT reached by any GPU test: that dimension needs a ring
    of 4096 slots (N >= 2^13), where one block of 4096 packed ciphertexts is 4.6 GiB, and Halves24 runs only on the
    group-sequential layout of more than 8 blocks — over 40 GiB resident and hours of host recomputation."""
import os
import subprocess

import pytest

import oracle_lib as O
from conftest import ROOT
from test_gpu_edge_primes import evaluator_chain, transform_chain

INC = os.path.join(ROOT, "tests", "csrc")
SRC = os.path.join(INC, "loop_b_ref_check.cpp")


@pytest.fixture(scope="module")
def chain_args():
    out = []
    for name, log_n in (("default11", 11), ("default15", 15)):
        P = O.Params(log_n=log_n, depth=11, dim=64)
        out.append((name, log_n, [int(q) for q in P.moduli[:P.nQ]]))
        P.close()
    out.append(("evaluator11", 11, [int(q) for q in evaluator_chain(11)[:12]]))
    out.append(("transform11", 11, [int(q) for q in transform_chain(11)[:12]]))
    # what makes them edge chains: a 47- and a 48-bit scaling prime; a 59-bit and several 60-bit ones
    bits = [sorted({q.bit_length() for q in c[2][1:]}) for c in out]
    assert bits[0] == bits[1] == [45, 46] and {47, 48} <= set(bits[2]) and {48, 59, 60} <= set(bits[3]), bits
    assert all(c[2][0].bit_length() == 60 for c in out)
    return ["%s:%d:%s" % (n, l, ",".join(map(str, q))) for n, l, q in out]


def _run(exe, chain_args):
    out = subprocess.run([str(exe)] + chain_args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "loop B reference ok (4 chains)" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def test_loop_b_reference_against_closed_forms_and_exact_ranges(tmp_path, chain_args):
    exe = tmp_path / "loop_b_ref_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    text = _run(exe, chain_args)
    # the margins the docstring quotes are the program's own figures
    assert "Halves24 24+24 bits at dim 512: ll 59 bits, mid 60 bits, hh 59 bits (of 63)" in text
    assert "Halves24 24+24 bits at dim 4096: ll 62 bits, mid 63 bits, hh 62 bits (of 63)" in text
    assert "Halves24 24+22 bits at dim 512: ll 59 bits, mid 58 bits, hh 55 bits (of 63)" in text
    assert "Halves24 24+22 bits at dim 4096: ll 62 bits, mid 61 bits, hh 58 bits (of 63)" in text


def test_loop_b_reference_under_host_sanitizers(tmp_path, chain_args):
    """the same stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer (host code, run directly)"""
    exe = tmp_path / "loop_b_ref_check_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    _run(exe, chain_args)
