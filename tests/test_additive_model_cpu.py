"""The integer model of tests/additive_ref.py against the oracle's own addition and against plain Python integers, on both N = 2^11
chains, so that tests/test_gpu_additive_edges.py does not rest on unchecked Python.  Also stated as assertions: the conditions under
which that file's cases mean what it says (16 saturated residues fit 64 bits on every limb, 129 do not on q_0), and which sums make
reduce64 (image_matching_amd/csrc/devmath.h) take its conditional subtraction."""
import numpy as np
import pytest

import additive_ref as A
import oracle_lib as O


@pytest.fixture(scope="module", params=sorted(A.CHAINS))
def ring(request):
    P = A.CHAINS[request.param]()
    K = O.Keys(P, 41, rotations=[])
    return P, O.Oracle(P, K)


def test_sum_mod_equals_the_oracles_chained_add(ring):
    P, Or = ring
    rng = np.random.default_rng(5)
    cts = [Or.encrypt(rng.uniform(-1, 1, P.slots), 3, 10 + i) for i in range(5)]
    stack = np.stack([c.data() for c in cts])
    for X in (2, 3, 5):
        acc = cts[0].clone()
        for c in cts[1:X]:
            Or.add(acc, c)
        assert np.array_equal(A.sum_mod(stack[:X], P.moduli), acc.data()), X
    # the same on residues at the ends of the range, two and three components
    for npoly in (2, 3):
        for name in ("saturated", "alternating", "distinct"):
            s = A.BUILDERS[name](P.moduli, 3, npoly, P.nQ, P.N)
            acc = A.oracle_ct(P, s[0], P.delta)
            for x in (1, 2):
                Or.add(acc, A.oracle_ct(P, s[x], P.delta))
            assert np.array_equal(A.sum_mod(s, P.moduli), acc.data()), (npoly, name)


@pytest.mark.parametrize("X", (1, 2, 3, 16, 129))
def test_sum_mod_of_saturated_residues(ring, X):
    P, _ = ring
    got = A.sum_mod(A.saturated(P.moduli, X, 2, P.nQ, P.N), P.moduli)
    for j in range(P.nQ):
        q = int(P.moduli[j])
        assert np.all(got[:, j] == np.uint64(X * (q - 1) % q)), (X, j)


def test_raw_sum_is_the_plain_sum_and_refuses_a_wrap(ring):
    P, _ = ring
    s = A.saturated(P.moduli, 16, 3, P.nQ, P.N)
    got = A.raw_sum(s)
    for j in range(P.nQ):
        assert np.all(got[:, j] == np.uint64(16 * (int(P.moduli[j]) - 1))), j
    d = A.distinct(P.moduli, 16, 2, P.nQ, P.N, seed=3)
    want = np.zeros(d.shape[1:], dtype=object)
    for x in range(16):
        want = want + d[x].astype(object)
    assert np.array_equal(A.raw_sum(d).astype(object), want)
    with pytest.raises(AssertionError):
        A.raw_sum(A.saturated(P.moduli, 129, 2, 1, P.N))


def test_sixteen_saturated_residues_fit_64_bits_and_129_do_not(ring):
    """the raw-sum test is meaningful only while 16 (q_j - 1) < 2^64; of the add_many sizes only 129 separates a 64-bit accumulator
    from a 128-bit one, and only on the 60-bit limb"""
    P, _ = ring
    for j in range(P.nT):
        assert 16 * (int(P.moduli[j]) - 1) < (1 << 64), j
    q0 = int(P.moduli[0])
    assert 129 * (q0 - 1) >= (1 << 64) and 16 * (q0 - 1) < (1 << 64)
    for j in range(1, P.nQ):
        assert 129 * (int(P.moduli[j]) - 1) < (1 << 64), j
    # 16 saturated residues come within 16 (c + 1) of 2^64 on q_0 = 2^60 - c
    assert (1 << 64) - 16 * (q0 - 1) == 16 * ((1 << 60) - q0 + 1)


def _reduce64_estimate(a, q):
    """the quotient estimate of reduce64: floor(a floor(2^64 / q) / 2^64); the kernel then subtracts q once more if it has to"""
    return (a * ((1 << 64) // q)) >> 64


def test_which_sums_need_reduce64s_conditional_subtraction(ring):
    """16 (q_j - 1) leaves the residue q_j - 16: the estimate is already the true quotient there, so that sum does not notice a
    missing conditional subtraction.  A sum that is an exact multiple of q_j does (15 (q_j - 1) + 15 = 15 q_j, and (q_j - 1) + 1):
    the estimate is one short and the subtraction has to bring q_j down to 0.  The GPU file therefore runs both."""
    P, _ = ring
    for j in range(P.nQ):
        q = int(P.moduli[j])
        a = 16 * (q - 1)
        assert a - _reduce64_estimate(a, q) * q == q - 16
        for a in (15 * q, q):
            assert a - _reduce64_estimate(a, q) * q == q
