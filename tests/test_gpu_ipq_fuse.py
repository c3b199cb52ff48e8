"""The relinearise + rescale product with the Q-limb inner product formed in the pipeline's last pass (k_ntt15_p2_ip_tail +
k_ntt15_p2_ipq: the sums reach the merged ModDown + Rescale epilogue in registers) against the parent's two kernels with the sums
through the accumulator (HYDIA_NO_IPQ_FUSE=1) and against the oracle, byte for byte.  N = 2^15: the path exists only there.

By default the path takes batches of at least 16 ciphertexts; HYDIA_IPQ_MIN=1 opens it to the small batches used here.

Limb counts: 12 = three digits, full last digit; 9 = three digits, one-limb last digit; 8 = two full digits; 5 = two digits, one-limb
last digit.  X = 3 exercises the grouping of the first launch (xb falls back to X) and an odd number of ciphertexts in the second;
X = 16 two groups of eight.
Epilogues: eval_mult -> ST 9; chebyshev_compare -> ST 10 (sub operand, doubling), addc, mult_add's addend, and beside them the steps
with a subtrahend K c (ST 11), which keep the parent's kernels; computeSimilarity on a hoisted database -> ST 3 on a 3-component
accumulator (no product source)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
KEY_SEED = 20250725
SWITCH = "HYDIA_NO_IPQ_FUSE"


def make_ctx(env):
    """the switches are read once, when the context is created"""
    import image_matching_amd as im
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv(SWITCH, raising=False)
        mp.delenv("HYDIA_INT_EPILOGUE", raising=False)
        mp.delenv("HYDIA_IPQ_MIN", raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        cc = im.Context()
    cc.keygen(KEY_SEED)
    return cc


@pytest.fixture(scope="module")
def oracle():
    P = O.Params()
    K = O.Keys(P, KEY_SEED)
    return P, O.Oracle(P, K)


@pytest.fixture(scope="module")
def pair(oracle):
    P = oracle[0]
    fused, parent = make_ctx({"HYDIA_IPQ_MIN": "1"}), make_ctx({SWITCH: "1"})
    assert np.array_equal(fused.moduli, P.moduli) and np.array_equal(parent.moduli, P.moduli)
    yield fused, parent
    fused.close()
    parent.close()


@pytest.fixture(scope="module")
def slots(oracle):
    return np.random.default_rng(5).uniform(-1, 1, (32, oracle[0].slots))


def gpu_operands(cc, z, X, nl):
    a, b = cc.encrypt(z[:X], 11, 40), cc.encrypt(z[16:16 + X], 12, 50)
    cc.level_reduce(a, nl)
    cc.level_reduce(b, nl)
    return a, b


def owned(ct):
    """data() is a view into the oracle's ciphertext: copy it while the ciphertext is alive"""
    return ct.data().copy()


def oracle_products(oracle, z, X, nl):
    P, Or = oracle
    ab, aa = [], []
    for i in range(X):
        a, b = Or.encrypt(z[i], 11, 40 + i), Or.encrypt(z[16 + i], 12, 50 + i)
        P.L.hyo_drop_to(P.h, a.h, nl)
        P.L.hyo_drop_to(P.h, b.h, nl)
        ab.append(owned(Or.mult(a, b)))
        aa.append(owned(Or.mult(a, a)))
    return np.stack(ab), np.stack(aa)


@pytest.mark.parametrize("nl,X", [(nl, X) for nl in (12, 9, 8, 5) for X in (1, 3)] + [(5, 16)])
def test_products_equal_parent_and_oracle(oracle, pair, slots, nl, X):
    want_ab, want_aa = oracle_products(oracle, slots, X, nl)
    got = []
    for cc in pair:
        a, b = gpu_operands(cc, slots, X, nl)
        ab, aa = cc.eval_mult(a, b), cc.eval_mult(a, a)
        assert ab.shape()[:3] == (X, 2, nl - 1)
        got.append((ab.export(), aa.export()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][0], want_ab) and np.array_equal(got[0][1], want_aa)


def test_integer_epilogue_takes_its_operand_from_registers(oracle, slots):
    """HYDIA_INT_EPILOGUE=1: p2_finish<9> instead of p2_finish3_fp on the limbs below 2^47 (three digits and two)"""
    cc = make_ctx({"HYDIA_INT_EPILOGUE": "1", "HYDIA_IPQ_MIN": "1"})
    try:
        for nl in (12, 5):
            want_ab, want_aa = oracle_products(oracle, slots, 3, nl)
            a, b = gpu_operands(cc, slots, 3, nl)
            assert np.array_equal(cc.eval_mult(a, b).export(), want_ab)
            assert np.array_equal(cc.eval_mult(a, a).export(), want_aa)
    finally:
        cc.close()


def test_comparator_equal_parent_and_oracle(oracle, pair):
    P, Or = oracle
    x = np.random.default_rng(9).uniform(-1, 1, (3, P.slots))
    got = []
    for cc in pair:
        ct = cc.encrypt(x, 2, 1)
        cc.level_reduce(ct, cc.nQ - 1)  # the comparator runs on a level-1 score ciphertext
        got.append(cc.chebyshev_compare(ct, 0.44, 10).export())
    assert np.array_equal(got[0], got[1])
    for i in range(3):
        oc = Or.encrypt(x[i], 2, 1 + i)
        P.L.hyo_drop_to(P.h, oc.h, P.nQ - 1)
        assert np.array_equal(got[0][i], owned(Or.chebyshev_compare(oc, 0.44, 10))), i


def test_similarity_three_hoisted_blocks_equal_parent_and_oracle(oracle, pair):
    """relin_rescale of the 3-component accumulators of three blocks: no product source, epilogue ST 3, X = 3 at twelve limbs"""
    import image_matching_amd as im
    P, Or = oracle
    n = 2 * P.slots + 40
    db = np.random.default_rng(77).integers(-99, 100, size=(n, 512)).astype(np.float64)
    query = np.ones(512)
    dbc = Or.enroll(db.copy(), 8, matvec="hoisted")
    oq = Or.encrypt_query(query, 2, 9)
    sim = Or.compute_similarity(oq, dbc, n)
    assert len(sim) == 3
    got = []
    for cc in pair:
        cc.set_matvec("hoisted")
        im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=8)
        cc.set_matvec("auto")
        assert cc.db_kind() == 5
        gq = im.DiagonalReceiver(cc, n).encryptQuery(query, seed=2, nonce=9)
        got.append(im.DiagonalSender(cc, n).computeSimilarity(gq).export())
    assert np.array_equal(got[0], got[1])
    for g in range(3):
        assert np.array_equal(got[0][g], sim[g].data()), g
