"""Pins the references of tests/test_gpu_client_edges.py, without a GPU: the premises the crafted inputs rest on, the CPU oracle against
the Python-integer models of tests/client_ref.py (doubles compared as bit patterns), and, for every wrong form a receiver-side kernel
could have, a crafted input on which that form gives another double or residue than the right one.  Both N = 2^11 chains of
additive_ref: the default one (a 60-bit q_0, q_1 a scaling prime next to 2^45) and test_gpu_edge_primes.evaluator_chain (q_0 =
2^60 - c, q_1 the prime just below 2^45 + 2^41)."""
from fractions import Fraction

import numpy as np
import pytest

import additive_ref as A
import client_ref as R
import oracle_lib as O

SEED = 20260517


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module", params=sorted(A.CHAINS))
def chain(request):
    P = A.CHAINS[request.param]()
    yield P
    P.close()


@pytest.fixture(scope="module")
def keyed(chain):
    K = O.Keys(chain, SEED, rotations=[])
    return chain, K, O.Oracle(chain, K)


def impulse(P, residues):
    """[nu][N] coefficient form: the residues [nu] at index 0, 0 elsewhere"""
    t = np.zeros((len(residues), P.N), dtype=np.uint64)
    t[:, 0] = residues
    return t


# ------------------------------------------------------------------------------------------------------------------------ premises
def test_premise_constant_vector_encodes_to_coefficient_zero_alone(chain):
    P = chain
    d = P.delta
    for k, want in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (2.0 ** 63 - 1024, 2 ** 63 - 1024), (-(2.0 ** 63), -2 ** 63), (-1.0, -1),
                    (float((1 << 58) + (1 << 13)), (1 << 58) + (1 << 13))):
        co = P.encode_coeffs(np.full(P.slots, k / d))
        assert int(co[0]) == want and not co[1:].any(), k
        assert R.encode_const_coeff(k / d, d) == want, k
    slots, ks = R.encoder_slots(P.moduli, d, P.slots)
    for v, k in zip(slots, ks):
        co = P.encode_coeffs(v)
        assert int(co[0]) == R.encode_const_coeff(v[0], d) and not co[1:].any(), k
        assert Fraction(float(v[0])) * Fraction(d) == Fraction(k), k  # v = k / delta is exact: the model rounds k itself


def test_premise_encoder_inputs_stay_inside_the_64_bit_range(chain):
    P = chain
    slots, ks = R.encoder_slots(P.moduli, P.delta, P.slots)
    at_edge = 0
    for v, k in zip(slots, ks):
        m = R.encode_const_coeff(v[0], P.delta)
        assert abs(m) <= 2 ** 63 and (abs(m) < 2 ** 63 or m == -2 ** 63), k  # llrint is defined on [-2^63, 2^63) only
        at_edge += m == -2 ** 63
    assert at_edge == 1
    ms = [R.encode_const_coeff(v[0], P.delta) for v in slots]
    for j in (1, 2):  # the multiples of a limb's modulus are exact
        assert -int(P.moduli[j]) in ms and -2 * int(P.moduli[j]) in ms


def test_premise_double_rounding_values_separate_the_two_conversions(chain):
    Q = int(chain.moduli[0]) * int(chain.moduli[1])
    mag = (1 << 64) + (1 << 63) + 2049
    assert R.two_step(mag) == 2.7670116110564327e19 and float(mag) == 2.767011611056433e19
    dr = R.double_rounding_values(Q)
    assert len(dr) >= 4 and len(set(dr)) == len(dr)
    for m in dr:
        assert (1 << 64) <= m <= Q >> 1 and R.two_step(m) != float(m), m
    vals = R.values_nu2(chain.moduli, chain.delta)
    assert all(m in vals and Q - m in vals for m in dr)
    assert sum((a & R.MASK64) >= (1 << 63) and a >= (1 << 64) for a in vals) >= 3


def test_premise_threshold_inputs(chain):
    P = chain
    d = P.delta
    two = lambda a, s: R.decode_front_model(R.residues_of([a], P.moduli, 2), P.moduli, s)[0]
    assert two(int(d), d) == 1.0 and two(int(d) - 1, d) == 0.9999999999999716
    assert two(1 << 90, d * d) == 1.0 and two((1 << 90) - (1 << 37), d * d) == np.nextafter(1.0, 0.0)
    assert two(2 ** 100 + 2 ** 47 + 1, d) == (2.0 ** 100 + 2.0 ** 48) / d  # one unit above the tie: up


# ------------------------------------------------------------------------------------------------------------------------ oracle vs models
@pytest.mark.parametrize("nu", [2, 1])
def test_oracle_decode_equals_the_front_model_on_every_single_input(chain, nu):
    """fact 2 and the oracle's front in one: P.decode of the impulse a X^0 is the model's double in EVERY slot, for every crafted value and
    every scale"""
    P = chain
    vals = R.crafted_values(P.moduli, P.delta, nu)
    res = R.residues_of(vals, P.moduli, nu)
    for scale in R.scales(P):
        want = R.decode_front_model(res, P.moduli, scale)
        for i, a in enumerate(vals):
            got = P.decode(impulse(P, res[:, i]), scale)
            assert np.array_equal(bits(got), bits(np.full(P.slots, want[i]))), (a, scale, got[:2], want[i])
        assert not np.signbit(want[vals.index(0)])  # a zero coefficient is +0.0


def test_oracle_decode_of_the_issue_values(chain):
    P = chain
    q0, q1 = int(P.moduli[0]), int(P.moduli[1])
    Q = q0 * q1
    for a in (0, 1, Q >> 1, (Q >> 1) + 1, Q - 1, int(P.delta), int(P.delta) - 1, 2 ** 100 + 2 ** 47 + 1):
        cen = a - Q if a > Q >> 1 else a
        want = (-1.0 if cen < 0 else 1.0) * R.two_step(abs(cen)) / P.delta
        got = P.decode(impulse(P, [a % q0, a % q1]))
        assert np.array_equal(bits(got), bits(np.full(P.slots, want))), a


@pytest.mark.parametrize("nl", [12, 1])
@pytest.mark.parametrize("npoly", [2, 3])
@pytest.mark.parametrize("pattern", R.DEC_PATTERNS)
def test_oracle_decrypt_equals_the_dot_product_model(keyed, pattern, npoly, nl):
    P, K, Or = keyed
    batch = R.dec_patterns(P, 3, npoly, nl, pattern, SEED + npoly + nl)
    assert pattern == "sat" or not np.array_equal(batch[0], batch[1])
    nu = min(nl, 2)
    for x in range(3):
        t = R.dec_dot_model(batch[x], K.s_ntt(), P.moduli)
        coeff = np.stack([P.ntt_inv(t[j], j) for j in range(nu)])
        want = P.decode(coeff, P.delta)
        got = Or.decrypt(A.oracle_ct(P, batch[x], P.delta))
        assert np.array_equal(bits(got), bits(want)), (pattern, npoly, nl, x)


def test_oracle_encode_equals_the_constant_model(chain):
    P = chain
    slots, ks = R.encoder_slots(P.moduli, P.delta, P.slots)
    for v, k in zip(slots, ks):
        got = P.encode(v, P.delta, P.nQ)
        want = np.array(R.encode_const_model(v[0], P.delta, P.moduli[:P.nQ]), dtype=np.uint64)
        assert np.array_equal(got, np.repeat(want[:, None], P.N, axis=1)), k
    m = {k: R.encode_const_model(k / P.delta, P.delta, P.moduli[:P.nQ]) for k in ks}
    for j in (1, 2):  # a negative multiple of q_j is the residue 0 on limb j, never q_j
        assert m[-float(int(P.moduli[j]))][j] == 0 and m[-2.0 * float(int(P.moduli[j]))][j] == 0


# ------------------------------------------------------------------------------------------------------------------------ wrong forms
def differs(P, nu, **wrong):
    """crafted values on which the wrong form of the front gives another double than the right one, at some scale"""
    vals = R.crafted_values(P.moduli, P.delta, nu)
    res = R.residues_of(vals, P.moduli, nu)
    hit = set()
    for scale in R.scales(P):
        right, bad = R.decode_front_model(res, P.moduli, scale), R.decode_front_model(res, P.moduli, scale, **wrong)
        hit |= {vals[i] for i in np.flatnonzero(bits(right) != bits(bad))}
    return hit


def test_wrong_centring_comparisons_are_noticed(chain):
    q0, q1 = int(chain.moduli[0]), int(chain.moduli[1])
    assert differs(chain, 2, centre_ge=True) == {(q0 * q1) >> 1}
    assert differs(chain, 1, centre_ge=True) == {q0 >> 1}


def test_one_step_conversion_is_noticed(chain):
    Q = int(chain.moduli[0]) * int(chain.moduli[1])
    dr = R.double_rounding_values(Q)
    assert differs(chain, 2, one_step=True) >= set(dr) | {Q - m for m in dr}


def test_dropped_second_limb_is_noticed(chain):
    q0 = int(chain.moduli[0])
    assert {q0, q0 + 1, 1 << 90} <= differs(chain, 2, drop_second=True)


def test_unreduced_r0_is_noticed(chain):
    hit = differs(chain, 2, reduce_r0=False)
    assert int(chain.moduli[0]) - 1 in hit and len(hit) >= 4


def test_wrong_encoder_roundings_and_the_missing_zero_case_are_noticed(chain):
    P = chain
    ks = R.encoder_ks(P.moduli)
    q = P.moduli[:P.nQ]
    right = {k: R.encode_const_model(k / P.delta, P.delta, q) for k in ks}
    away = {k for k in ks if R.encode_const_model(k / P.delta, P.delta, q, rounding=R.half_away) != right[k]}
    trunc = {k for k in ks if R.encode_const_model(k / P.delta, P.delta, q, rounding=R.truncate) != right[k]}
    nozero = {k for k in ks if R.encode_const_model(k / P.delta, P.delta, q, zero_case=False) != right[k]}
    assert away == {s * k for k in (0.5, 2.5, 2.0 ** 51 + 0.5) for s in (1, -1)} and trunc == {1.5, -1.5}
    assert nozero == {-float(int(P.moduli[j])) * m for j in (1, 2) for m in (1, 2)}
    assert R.rne(Fraction(5, 2)) == 2 and R.rne(Fraction(-5, 2)) == -2 and R.rne(Fraction(7, 2)) == 4 and R.rne(Fraction(-7, 4)) == -2
    assert R.truncate(Fraction(-7, 4)) == -1 and R.half_away(Fraction(-5, 2)) == -3
