"""CPU-only model of the accumulation bounds of loop B for a plain gallery (k_hydia_plain / k_hydia_plain_sk in
image_matching_amd/csrc/kernels.hip), in exact Python integers wider than the kernel's sums — the bounds written next to the kernel:

  Halves24.  Without Karatsuba's operand sums every half is below 2^24, so every product is below 2^48.  ll and hh take one product
  per diagonal, mid two.  At the launcher's limit of 4096 diagonals of saturated 48-bit operands the widest sum, mid, is
  4096 * 2 * (2^24 - 1)^2 < 2^61: two bits below the 2^63 the encrypted kernel's Karatsuba term reaches (tests/test_loop_b_model_cpu.py),
  and below 2^63 with room.  Four times the diagonals (16384) still fit, eight times (32768) pass 2^63 — the 4096 limit is kept,
  not needed.

  Sums128.  The fold chunk is the encrypted kernel's, 2^(125 - 2k) diagonals for a k-bit limb with 125 - 2k < 30 (else never):
  32 on a 60-bit limb, 128 on a 59-bit one.  A plain product of residues below q is below q^2 < 2^(2k), so a folded q - 1 plus a
  chunk of saturated products stays below 2^126: the chunk is conservative by two bits, and four chunks' worth of products would
  still fit 2^128 (five would not be guaranteed to).

Both accumulations are also RUN as the kernel runs them (64-bit wrapping sums of 24-bit half products recombined as
ll + mid 2^24 + hh 2^48; 128-bit wrapping sums folded every chunk) on saturated and on random operands and compared with the exact
sum modulo q."""
import random

import pytest

import oracle_lib as O
from test_gpu_edge_primes import evaluator_chain, transform_chain

M64, M128 = (1 << 64) - 1, (1 << 128) - 1


def chunk_of(q, dim):
    """Sums128's fold interval (kernels.hip): kbits = the bit length of q"""
    k = q.bit_length()
    return dim if 125 - 2 * k >= 30 else 1 << (125 - 2 * k)


def halves24_sum(a, b, q):
    """sum a_i b_i mod q as k_hydia_plain<Halves24> forms it: three wrapping 64-bit sums over 24-bit halves, one reduction"""
    ll = mid = hh = 0
    for x, y in zip(a, b):
        al, ah, bl, bh = x & 0xFFFFFF, x >> 24, y & 0xFFFFFF, y >> 24
        assert ah < 1 << 24 and bh < 1 << 24
        ll = (ll + al * bl) & M64
        mid = (mid + al * bh) & M64
        mid = (mid + ah * bl) & M64
        hh = (hh + ah * bh) & M64
    return (ll + (mid << 24) + (hh << 48)) % q


def sums128_sum(a, b, q, chunk):
    """the same sum as k_hydia_plain<Sums128> forms it: a wrapping 128-bit sum, folded (reduced mod q) every `chunk` diagonals"""
    s = 0
    for i, (x, y) in enumerate(zip(a, b)):
        if i and i % chunk == 0:
            s %= q
        s = (s + x * y) & M128
    return s % q


@pytest.fixture(scope="module")
def chains():
    out = {}
    for name, log_n in (("default11", 11), ("default15", 15)):
        P = O.Params(log_n=log_n, depth=11, dim=64)
        out[name] = [int(q) for q in P.moduli[:P.nQ]]
        P.close()
    out["evaluator11"] = [int(q) for q in evaluator_chain(11)[:12]]
    out["transform11"] = [int(q) for q in transform_chain(11)[:12]]
    return out


def test_halves24_sums_stay_below_2_63_at_the_launchers_limit():
    h = (1 << 24) - 1  # a saturated 48-bit operand: both halves all ones
    for dim, fits in ((512, True), (4096, True), (16384, True), (32768, False)):
        ll, mid, hh = dim * h * h, dim * 2 * h * h, dim * h * h
        assert (max(ll, mid, hh) < 1 << 63) == fits, dim
    assert 4096 * 2 * h * h < 1 << 61  # two bits of margin at the limit the launcher keeps
    # 46-bit residues: halves of 24 and 22 bits on the database side
    assert 4096 * (h * ((1 << 22) - 1) + h * h) < 1 << 61


def test_halves24_recombination_equals_the_exact_sum(chains):
    rng = random.Random(7)
    for name in ("default11", "evaluator11"):
        for q in chains[name][1:]:
            if q.bit_length() > 48:
                continue
            for dim in (64, 512, 4096):
                sat = [q - 1] * dim
                assert halves24_sum(sat, sat, q) == dim % q  # (q - 1)^2 = 1 mod q
                top = [(1 << 48) - 1] * dim  # what the 6-byte field can hold, canonical or not
                assert halves24_sum(top, top, q) == dim * ((1 << 48) - 1) ** 2 % q
            a = [rng.randrange(q) for _ in range(512)]
            b = [rng.randrange(q) for _ in range(512)]
            assert halves24_sum(a, b, q) == sum(x * y for x, y in zip(a, b)) % q


def test_sums128_with_the_existing_chunk_stays_below_2_128(chains):
    seen = set()
    for name, qs in chains.items():
        for q in qs:
            k = q.bit_length()
            for dim in (64, 512, 1024, 4096):
                ch = chunk_of(q, dim)
                seen.add((k, ch if ch < dim else 0))
                # a folded residue plus one chunk of saturated plain products: two bits below the 128 the sum has
                assert (q - 1) + ch * (q - 1) ** 2 < 1 << 126, (name, q, dim)
                # ... so the chunk is conservative by two bits: four times as many products still fit
                assert (q - 1) + 4 * ch * (q - 1) ** 2 < 1 << 128, (name, q, dim)
    assert (60, 32) in seen and (59, 128) in seen  # the fold path is exercised on 59/60-bit limbs
    q60 = max(q for qs in chains.values() for q in qs)
    assert q60.bit_length() == 60 and 32 * (q60 - 1) ** 2 + q60 < 1 << 128


def test_sums128_folded_accumulation_equals_the_exact_sum(chains):
    rng = random.Random(11)
    for name in ("default11", "transform11"):
        for q in chains[name]:
            if q.bit_length() < 59:
                continue
            for dim in (64, 512, 1024):
                ch = chunk_of(q, dim)
                sat = [q - 1] * dim
                assert sums128_sum(sat, sat, q, ch) == dim % q
                a = [rng.randrange(q) for _ in range(dim)]
                b = [rng.randrange(q) for _ in range(dim)]
                assert sums128_sum(a, b, q, ch) == sum(x * y for x, y in zip(a, b)) % q
                # the split-diagonal kernel: KS waves take every KS-th diagonal, fold every chunk of THEIR diagonals, partial sums added mod q
                for ks in (4, 8):
                    parts = [sums128_sum(a[w::ks], b[w::ks], q, ch) for w in range(ks)]
                    assert sum(parts) % q == sum(x * y for x, y in zip(a, b)) % q
