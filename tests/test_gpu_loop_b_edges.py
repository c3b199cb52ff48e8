"""Loop B (k_hydia_tensor<A, BPP, QW, NW> and k_hydia_tensor_sk<KS, QW>, the kernels the benchmark measures) against a host
recomputation with unsigned __int128 on residues that REACH the lazy sums' bounds — tests/csrc/loop_b_check.cpp with its pattern
flags, one subprocess per case, at N = 2^11.  Every comparison is bit for bit over every (query, block, limb, coefficient); the host
side (patterns, recomputation, slot map, and the range premises that say what these cases can see) is pinned without a GPU in
tests/test_loop_b_model_cpu.py.

Operand patterns, rotation set / database, for every case: sat/sat (q - 1 everywhere: every sum at its bound), holes/holes (q - 1
with one residue in 16 replaced, so every operand position still decides the result), sat/uniform, uniform/sat, edge/edge
(0, 1, q - 2, q - 1).  Each case also asserts, from the byte ledger the program prints, WHICH instantiations ran.

  a  default chain, 1 and 2 blocks, dim 512: k_hydia_tensor_sk<8, 1> on limb 0 (64 diagonals per wave: a fold at 32 and 32 more
     sums after it) and Sums128<true> at one and two blocks per wave.  1 block also at dim 1024, the ring's largest: 128 diagonals
     per wave, where a fold that never comes again wraps (64 saturated products still fit 128 bits — test_loop_b_model_cpu.py)
  b  4 and 8 blocks, dim 512: k_hydia_tensor_sk<4, 1> (128 diagonals per wave, three folds); two and four waves per workgroup
  c  16 blocks, dim 64 and 512: group-sequential with 46-bit residues — Sums128<false> streaming on limb 0 (one fold at dim 64,
     fifteen at 512) and Halves24<true>, whose three-deep loop leaves one diagonal over at dim 64 and two at 512
  d  16 blocks, dim 512, 48-bit group-sequential (Halves24<false>) and forced ciphertext-major (Sums128<true> at 16 blocks)
  e  evaluator_chain(11), 16 blocks, dim 64: 47- and 48-bit scaling primes -> 48-bit residues, Halves24<false> on high halves of a
     full 24 bits
  f  transform_chain(11), 2 and 16 blocks, dim 512: a 59-bit and 60-bit limbs among the scaling primes -> the database is unpacked
     and ciphertext-major, ONE Sums128<false> launch over all limbs with a fold interval of 32 / 128 / never per limb
  g  batches of 2 and 3 queries on 2, 8 and 16 blocks (46- and 48-bit): sk<8, 2>, sk<4, 2>, <Halves24<true>, 1, 2, 8>,
     <Sums128<true>, 1, 2, 8>, and the QW = 1 pass an odd batch ends with
  h  16 blocks as (block, giant step) pairs with 2 and 4 giant steps, 1 and 3 queries: the giant-major slot map
  i  the splits no other case takes, at dim 16 (the launcher picks (BPP, NW) from the block count alone): 9 blocks -> groups of one
     block, one block per wave and one wave; 12 blocks -> two blocks per wave, two waves; both with 46- and 48-bit residues, and as
     batches of 3 (one block per wave, NW = the group size 1 / 4); HYDIA_TENSOR_BPP=1 on 10 and 12 blocks of 48-bit residues ->
     Halves24<false> at one block per wave and two / four waves.  With them every k_hydia_tensor / k_hydia_tensor_sk instantiation
     the library ships is run by this file, except the five the launcher never selects: <Halves24<false>, 1, 2, *> and
     <Halves24<false>, 1, 1, 8> (a batch keeps Sums128<true> on 48-bit group-sequential residues)

No shape here is refused by the context or the launcher.  Not reached: Halves24 at its 4096-diagonal limit (tests/test_loop_b_model_cpu.py
says why), xcd_map = 0 (a ring below 1024 coefficients), N = 2^15 with saturated operands (the same kernels; minutes of host work).

Measured on one MI355X: the 24 cases a - h take 31 s, the i cases under 4 s each; the slowest are f-16-blocks 2.6 s, g-8-blocks-3q 2.5 s, d-48bit 2.5 s."""
import functools
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "loop_b_check")
LOG_N, N, NL = 11, 2048, 12
PAIRS = ("sat/sat", "holes/holes", "sat/uniform", "uniform/sat", "edge/edge")
GROUP, MAJOR = "group-sequential", "ciphertext-major"


def stream(policy, bpp, qw, nw):
    return "k_hydia_tensor<%s, %d, %d, %d>" % (policy, bpp, qw, nw)


def split(ks, qw):
    return "k_hydia_tensor_sk<%d, %d>" % (ks, qw)


S_PK, S_8B, H46, H48 = "Sums128<true>", "Sums128<false>", "Halves24<true>", "Halves24<false>"


@functools.lru_cache(maxsize=None)
def chain(name):
    from test_gpu_edge_primes import evaluator_chain, transform_chain
    moduli = {"evaluator": evaluator_chain, "transform": transform_chain}[name](LOG_N)
    assert len(moduli) == 16
    return ",".join(str(int(q)) for q in moduli)


def batch(names, queries):
    """the launches of a batch: a QW = 2 pass of each kernel, and for an odd batch the QW = 1 pass it ends with"""
    out = set()
    for n in names:
        two = re.sub(r", 1(, \d+>|>)$", r", 2\1", n)
        assert two != n
        out.add(two)
        if queries % 2:
            out.add(n)
    return out


# id, blocks, dim, layout mode, chain, queries, giants, layout text, residue text, kernels (as single-query QW = 1 names, one block per wave for
# batches)[, environment of the checker]
CASES = [
    ("a-1-blocks", 1, 512, 1, None, 1, 0, MAJOR, "48-bit packed", {split(8, 1), stream(S_PK, 1, 1, 1)}),
    ("a-2-blocks", 2, 512, 1, None, 1, 0, MAJOR, "48-bit packed", {split(8, 1), stream(S_PK, 2, 1, 1)}),
    ("a-1-blocks-dim1024", 1, 1024, 1, None, 1, 0, MAJOR, "48-bit packed", {split(8, 1), stream(S_PK, 1, 1, 1)}),
    ("b-4-blocks", 4, 512, 1, None, 1, 0, MAJOR, "48-bit packed", {split(4, 1), stream(S_PK, 2, 1, 2)}),
    ("b-8-blocks", 8, 512, 1, None, 1, 0, MAJOR, "48-bit packed", {split(4, 1), stream(S_PK, 2, 1, 4)}),
    ("c-dim64", 16, 64, 1, None, 1, 0, GROUP, "46-bit packed", {stream(S_8B, 2, 1, 4), stream(H46, 2, 1, 4)}),
    ("c-dim512", 16, 512, 1, None, 1, 0, GROUP, "46-bit packed", {stream(S_8B, 2, 1, 4), stream(H46, 2, 1, 4)}),
    ("d-48bit", 16, 512, 2, None, 1, 0, GROUP, "48-bit packed", {stream(S_8B, 2, 1, 4), stream(H48, 2, 1, 4)}),
    ("d-ct-major", 16, 512, 0, None, 1, 0, MAJOR, "48-bit packed", {stream(S_8B, 2, 1, 4), stream(S_PK, 2, 1, 4)}),
    ("e-evaluator-chain", 16, 64, 1, "evaluator", 1, 0, GROUP, "48-bit packed", {stream(S_8B, 2, 1, 4), stream(H48, 2, 1, 4)}),
    ("f-2-blocks", 2, 512, 1, "transform", 1, 0, MAJOR, "unpacked 8-byte", {stream(S_8B, 2, 1, 1)}),
    ("f-16-blocks", 16, 512, 1, "transform", 1, 0, MAJOR, "unpacked 8-byte", {stream(S_8B, 2, 1, 4)}),
]
for Q in (2, 3):
    CASES += [
        ("g-2-blocks-%dq" % Q, 2, 512, 1, None, Q, 0, MAJOR, "48-bit packed", batch({split(8, 1), stream(S_PK, 1, 1, 2)}, Q)),
        ("g-8-blocks-%dq" % Q, 8, 512, 1, None, Q, 0, MAJOR, "48-bit packed", batch({split(4, 1), stream(S_PK, 1, 1, 4)}, Q)),
        ("g-16-blocks-46bit-%dq" % Q, 16, 64, 1, None, Q, 0, GROUP, "46-bit packed", batch({stream(S_8B, 1, 1, 8), stream(H46, 1, 1, 8)}, Q)),
        ("g-16-blocks-48bit-%dq" % Q, 16, 64, 2, None, Q, 0, GROUP, "48-bit packed", batch({stream(S_8B, 1, 1, 8), stream(S_PK, 1, 1, 8)}, Q)),
    ]
for NG in (2, 4):
    CASES += [
        ("h-%d-giants-1q" % NG, 16, 64, 1, None, 1, NG, GROUP, "46-bit packed", {stream(S_8B, 2, 1, 4), stream(H46, 2, 1, 4)}),
        ("h-%d-giants-3q" % NG, 16, 64, 1, None, 3, NG, GROUP, "46-bit packed", batch({stream(S_8B, 1, 1, 8), stream(H46, 1, 1, 8)}, 3)),
    ]
CASES += [
    ("i-9-blocks", 9, 16, 1, None, 1, 0, GROUP, "46-bit packed", {stream(S_8B, 1, 1, 1), stream(H46, 1, 1, 1)}),
    ("i-9-blocks-48bit", 9, 16, 2, None, 1, 0, GROUP, "48-bit packed", {stream(S_8B, 1, 1, 1), stream(H48, 1, 1, 1)}),
    ("i-12-blocks", 12, 16, 1, None, 1, 0, GROUP, "46-bit packed", {stream(S_8B, 2, 1, 2), stream(H46, 2, 1, 2)}),
    ("i-12-blocks-48bit", 12, 16, 2, None, 1, 0, GROUP, "48-bit packed", {stream(S_8B, 2, 1, 2), stream(H48, 2, 1, 2)}),
    ("i-9-blocks-3q", 9, 16, 1, None, 3, 0, GROUP, "46-bit packed", batch({stream(S_8B, 1, 1, 1), stream(H46, 1, 1, 1)}, 3)),
    ("i-12-blocks-3q", 12, 16, 1, None, 3, 0, GROUP, "46-bit packed", batch({stream(S_8B, 1, 1, 4), stream(H46, 1, 1, 4)}, 3)),
    ("i-10-blocks-48bit-bpp1", 10, 16, 2, None, 1, 0, GROUP, "48-bit packed", {stream(S_8B, 1, 1, 2), stream(H48, 1, 1, 2)}, {"HYDIA_TENSOR_BPP": "1"}),
    ("i-12-blocks-48bit-bpp1", 12, 16, 2, None, 1, 0, GROUP, "48-bit packed", {stream(S_8B, 1, 1, 4), stream(H48, 1, 1, 4)}, {"HYDIA_TENSOR_BPP": "1"}),
]


@pytest.mark.parametrize("blocks,dim,mode,chain_name,queries,giants,layout,residues,kernels,env", [(c[1:] + ({},))[:10] for c in CASES],
                         ids=[c[0] for c in CASES])
def test_loop_b_on_saturated_and_edge_residues(blocks, dim, mode, chain_name, queries, giants, layout, residues, kernels, env):
    assert os.path.exists(EXE), "tests/csrc/loop_b_check is built by __graft_entry__.build()"
    cmd = [EXE, str(blocks), str(dim), str(LOG_N), str(mode), "--patterns", ",".join(PAIRS)]
    if chain_name:
        cmd += ["--moduli", chain(chain_name), "--np", "4"]
    if queries > 1:
        cmd += ["--queries", str(queries)]
    if giants:
        cmd += ["--giants", str(giants)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired as ex:
        pytest.fail("loop_b_check ran into its time limit: " + str(ex.stdout)[-2000:])
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    head = r.stdout.splitlines()[0]
    assert layout in head and residues in head, head
    triples = queries * blocks * NL * N
    for pair in PAIRS:
        assert "%s: loop B, %d queries x %d blocks x %d diagonals at N = 2^%d: 0 mismatches of %d " % (pair, queries, blocks, dim, LOG_N, triples) \
            in r.stdout, tail
        ran = set(re.findall(r"^ledger %s: (k_hydia_tensor\S*<.*>) x\d+$" % re.escape(pair), r.stdout, flags=re.M))
        assert ran == kernels, (pair, sorted(ran), sorted(kernels))
