"""The oracle's rescale against a Python big-integer model (tests/batch_ref.rescale_model) on inputs that put the centred value exactly
on and around q_l / 2 at every coefficient — standalone and through the relinearised product.  This pins the centring rule
(y > (q_l >> 1) goes negative) independently of the oracle and of the GPU engine; tests/test_gpu_batch_shapes.py then holds the engine's
kernels to the oracle on the same inputs.  N = 2^11 on every coefficient, N = 2^15 on a strided sample (stride 61: odd, so the sample
meets all eight target values)."""
import numpy as np
import pytest

import batch_ref as B
import oracle_lib as O

LIMB_COUNTS = (12, 7, 2)  # the full chain, one in between, and the rescale onto the 60-bit limb alone


class Ring:
    def __init__(self, P):
        self.P = P
        self.K = O.Keys(P, 31, rotations=[])
        self.Or = O.Oracle(P, self.K)
        rng = np.random.default_rng(P.log_n)
        a = self.Or.encrypt(rng.uniform(-1, 1, P.slots), 3, 1)
        b = self.Or.encrypt(rng.uniform(-1, 1, P.slots), 3, 2)
        self.pairs = B.mult_chain(self.Or, a, b, LIMB_COUNTS)
        self.idx = np.arange(P.N) if P.log_n <= 11 else np.arange(0, P.N, 61)


@pytest.fixture(scope="module")
def rings(small_params, full_params):
    return {11: Ring(small_params), 15: Ring(full_params)}


def _check_targets(P, pre, targets):
    """the limb about to be dropped holds the targets exactly, and they meet both sides of the boundary"""
    l = pre.shape[1] - 1
    q_l = int(P.moduli[l])
    for p in range(2):
        assert np.array_equal(P.ntt_inv(pre[p, l], l), targets[p]), p
    assert {int(v) for v in targets[0][:8]} == {0, 1, (q_l >> 1) - 1, q_l >> 1, (q_l >> 1) + 1, (q_l >> 1) + 2, q_l - 2, q_l - 1}
    assert not np.array_equal(targets[0], targets[1])


@pytest.mark.parametrize("nl", LIMB_COUNTS)
@pytest.mark.parametrize("log_n", [11, 15])
def test_rescale_of_boundary_input_equals_model(rings, log_n, nl):
    R = rings[log_n]
    P, Or = R.P, R.Or
    for other in ("real", "random", "saturated"):
        ct = R.pairs[nl][0].clone()
        if other == "random":
            B.randomise(P, ct, np.random.default_rng(nl))
        elif other == "saturated":
            B.saturate(P, ct)
        t = B.craft_rescale_input(P, ct)
        pre = ct.data().copy()
        _check_targets(P, pre, t)
        Or.rescale(ct)
        assert (ct.npoly, ct.nl) == (2, nl - 1)
        assert np.array_equal(B.to_coeff(P, ct.data(), R.idx), B.rescale_model(P, pre, nl - 1, R.idx)), other


@pytest.mark.parametrize("nl", LIMB_COUNTS)
@pytest.mark.parametrize("log_n", [11, 15])
def test_mult_of_crafted_pair_equals_model(rings, log_n, nl):
    R = rings[log_n]
    P, Or = R.P, R.Or
    a, b = R.pairs[nl][0].clone(), R.pairs[nl][1].clone()
    t = B.craft_product_pair(P, Or, a, b)
    d = B.relinearised(Or, a, b)
    pre = d.data().copy()  # (data() is a view into d: d stays referenced until the copy is taken)
    _check_targets(P, pre, t)  # the crafted relinearised limb IS the targets
    got = Or.mult(a, b)
    assert (got.npoly, got.nl) == (2, nl - 1)
    assert np.array_equal(B.to_coeff(P, got.data(), R.idx), B.rescale_model(P, pre, nl - 1, R.idx))



def test_tile_varies_first_last_odd_and_even_positions():
    distinct = np.arange(4 * 3).reshape(4, 3)
    want = distinct * 10
    for X in (1, 2, 3, 4, 5, 16, 17, 129):
        batch, exp, src = B.tile(distinct, X, want)
        assert batch.shape == (X, 3) and np.array_equal(exp, batch * 10) and len(src) == X
        assert all(np.array_equal(batch[i], distinct[src[i]]) for i in range(X))
        assert src[:min(X, 4)] == list(range(min(X, 4)))
        if X > 1:
            assert src[-1] != src[0] and src[1] != src[0]
        if X >= 4:
            assert set(src) == {0, 1, 2, 3}
    assert B.tile(distinct[:2], 17)[2][-1] == 1 and B.tile(distinct[:3], 16)[2][-1] == 2
