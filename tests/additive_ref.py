"""Helpers of the additive and comparator-leaf tests (tests/test_additive_model_cpu.py, tests/test_gpu_additive_edges.py): an exact
integer model of a sum of ciphertexts, residue arrays that sit on the ends of every limb's range, and the two N = 2^11 prime chains the
tests run on.  TEST INFRASTRUCTURE ONLY; no tests in here.

A batch is [X][npoly][nl][N] uint64, limb j holding residues of moduli[j].  The model never forms a 64-bit sum that could wrap: every
residue is split at 30 bits, the two halves are summed over the batch in uint64 (X < 2^22 keeps both below 2^64), and the halves are
joined as Python integers on the summed array, which is X times smaller than the batch."""
import numpy as np

import batch_ref as B
import oracle_lib as O
from test_gpu_edge_primes import evaluator_chain

LOG_N = 11
SPLIT = 30


def _exact_sum(stack):
    """[npoly][nl][N] object array of Python integers: the sum over axis 0, exact"""
    stack = np.asarray(stack, dtype=np.uint64)
    assert stack.ndim == 4 and stack.shape[0] < (1 << 22)
    lo = (stack & np.uint64((1 << SPLIT) - 1)).sum(axis=0, dtype=np.uint64)
    hi = (stack >> np.uint64(SPLIT)).sum(axis=0, dtype=np.uint64)
    return hi.astype(object) * (1 << SPLIT) + lo.astype(object)


def sum_mod(stack, moduli):
    """sum over the batch, reduced per limb: [npoly][nl][N] uint64 canonical residues"""
    total = _exact_sum(stack)
    out = np.empty(total.shape, dtype=np.uint64)
    for j in range(total.shape[1]):
        out[:, j] = (total[:, j] % int(moduli[j])).astype(np.uint64)
    return out


def raw_sum(stack):
    """sum over the batch as plain integers; the caller's inputs must keep it below 2^64 (asserted)"""
    total = _exact_sum(stack)
    assert int(total.max()) < (1 << 64), "the plain sum does not fit 64 bits"
    return total.astype(np.uint64)


# ---------------------------------------------------------------- input builders, each [X][npoly][nl][N] uint64
def constant(moduli, X, npoly, nl, N, value):
    """`value` everywhere (value < every modulus)"""
    assert all(int(value) < int(q) for q in moduli[:nl])
    return np.full((X, npoly, nl, N), value, dtype=np.uint64)


def zeros(moduli, X, npoly, nl, N):
    return constant(moduli, X, npoly, nl, N, 0)


def ones(moduli, X, npoly, nl, N):
    return constant(moduli, X, npoly, nl, N, 1)


def saturated(moduli, X, npoly, nl, N):
    """q_j - 1 everywhere"""
    out = np.empty((X, npoly, nl, N), dtype=np.uint64)
    for j in range(nl):
        out[:, :, j] = np.uint64(int(moduli[j]) - 1)
    return out


def alternating(moduli, X, npoly, nl, N):
    """0 at the even coefficients, q_j - 1 at the odd ones"""
    out = np.zeros((X, npoly, nl, N), dtype=np.uint64)
    for j in range(nl):
        out[:, :, j, 1::2] = np.uint64(int(moduli[j]) - 1)
    return out


def distinct(moduli, X, npoly, nl, N, seed=0):
    """uniform in [0, q_j) from a seeded generator: every (ciphertext, component, limb) row is drawn on its own, none is a copy"""
    rng = np.random.default_rng(seed)
    out = np.empty((X, npoly, nl, N), dtype=np.uint64)
    for j in range(nl):
        out[:, :, j] = rng.integers(0, int(moduli[j]), size=(X, npoly, N), dtype=np.uint64)
    return out


BUILDERS = {"saturated": saturated, "zeros": zeros, "alternating": alternating, "ones": ones, "distinct": distinct}


# ---------------------------------------------------------------- the two chains at N = 2^11
def default_params():
    """a 60-bit q_0 and eleven 45-bit scaling primes (+ 4 special primes)"""
    return O.Params(log_n=LOG_N, depth=11, dim=64)


def edge_params():
    """test_gpu_edge_primes.evaluator_chain: q_0 the IntP prime with the largest c, then the lean-edge pair, the top 47-bit prime and the
    smallest 48-bit prime ahead of default 45-bit primes"""
    return O.Params(log_n=LOG_N, depth=11, dim=64, moduli=evaluator_chain(LOG_N), n_p=4)


CHAINS = {"default": default_params, "edge": edge_params}


# ---------------------------------------------------------------- oracle ciphertexts that hold given residues
def oracle_ct(P, data, scale):
    """an oracle ciphertext holding `data` ([npoly][nl][N])"""
    data = np.asarray(data, dtype=np.uint64)
    ct = B.new_ct(P, data.shape[0], data.shape[1], scale)
    ct.data()[...] = data
    return ct


def crafted_encryption(Or, data, seed, nonce):
    """a fresh full-level encryption whose residues are overwritten in place with `data` ([2][nQ][N])"""
    P = Or.P
    ct = Or.encrypt(np.zeros(P.slots), seed, nonce)
    view = ct.data()
    assert view.shape == np.shape(data)
    view[...] = data
    return ct


def eval_sum_ref(Or, ct):
    """EvalSum on the oracle in the engine's order: m <- m + Rot_r(m) for r = 1, 2, 4, .., slots / 2; returns the residues"""
    m = ct.clone()
    r = 1
    while r < Or.P.slots:
        t = Or.rotate(m, r)
        Or.add(m, t)
        r *= 2
    return m.data().copy()


def powers_of_two(slots):
    return [1 << k for k in range(slots.bit_length() - 1)]
