"""GPU (run with -m gpu): approach 2 (GROTE group testing) end to end — the 19 + 6 limb chain, the squaring kernel, alphaNormRows /
alphaNormColumns, GroteSender / GroteReceiver — bit exact on exported residues against the restatement of tests/approach2_ref.py (the
CPU oracle's primitives composed in the reference's order) unless noted.  Switches are compared on EXPORTED BYTES."""
import os

import numpy as np
import pytest

import approach1_ref as A
import approach2_ref as G
import oracle_lib as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def make_context(im, env=None, depth=18, rotations=None, seed=7):
    """a 2^11 context with approach 1's key set; env: switches read once at creation"""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        cc = im.Context(im.default_params(log_n=11, mult_depth=depth, vector_dim=64), 0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    cc.keygen_rotations(cc.base_rotations() if rotations is None else rotations, seed=seed)
    return cc


@pytest.fixture(scope="module")
def small(im):
    """2^11 ring with approach 2's chain (depth 18: 19 + 6 limbs), 64-dim vectors: vpc 16, rowLength 32, colLength 32"""
    P = O.Params(log_n=11, depth=18, dim=64)
    K = O.Keys(P, 7, rotations=A.approach1_rotations(P.slots))
    cc = make_context(im)
    yield P, K, O.Oracle(P, K), cc
    cc.close()


@pytest.fixture(scope="module")
def nosq(im):
    cc = make_context(im, {"HYDIA_GROTE_NO_SQ": "1"})
    yield cc
    cc.close()


def database(P, n, planted, seed):
    rng = np.random.default_rng(seed)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for i in planted:
        db[i] = rng.integers(1, 4, size=P.dim)
    query = np.ones(P.dim)
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))
    return db, query, cos


def upload(cc, cts):
    return cc.import_ct(A.stack(cts), cts[0].scale)


def test_context_on_the_19_plus_6_chain(im, small):
    """the chain no context had before: alpha 7, six special primes — the key switch's unfused "other counts" path"""
    P, K, Or, cc = small
    assert (cc.nQ, cc.nP, P.nQ, P.nP, P.alpha) == (19, 6, 19, 6, 7)
    assert np.array_equal(cc.moduli, P.moduli) and np.array_equal(cc.roots, P.roots)
    rng = np.random.default_rng(1)
    a, b = (Or.encrypt(rng.uniform(-1, 1, P.slots), 4, 10 + i) for i in range(2))
    assert np.array_equal(cc.eval_mult(upload(cc, [a]), upload(cc, [b])).export()[0], Or.mult(a, b).data())
    for r in (1, P.slots - 32):
        assert np.array_equal(cc.eval_rotate(upload(cc, [a]), r).export()[0], Or.rotate(a, r).data()), r


@pytest.mark.parametrize("count", [1, 3])
def test_square_kernel(im, small, nosq, count):
    """k_tensor_sq at full level and on a limb prefix read in place (limb stride != limbs), against the oracle's product of the
    ciphertext with itself and against the general product kernel (HYDIA_GROTE_NO_SQ): identical bytes"""
    P, K, Or, cc = small
    rng = np.random.default_rng(count)
    cts = [Or.encrypt(rng.uniform(-1, 1, P.slots), 4, 20 + i) for i in range(count)]
    for nl in (0, P.nQ - 5):
        want = A.stack([G.oracle_square_norelin(P, Or, c, nl or None) for c in cts])
        got = cc.eval_square_no_relin(upload(cc, cts), nl)
        assert got.shape()[:3] == (count, 3, nl or P.nQ)
        assert np.array_equal(got.export(), want), nl
        assert np.array_equal(nosq.eval_square_no_relin(upload(nosq, cts), nl).export(), want), nl
        x = upload(cc, cts)
        if nl:
            cc.level_reduce(x, nl)
        assert np.array_equal(cc.eval_mult_no_relin(x, x).export(), want), nl


@pytest.mark.parametrize("what,count,rl", [("rows", 1, 32), ("cols", 1, 32), ("rows", 5, 4), ("cols", 3, 512)])
def test_alpha_norm_on_a_callers_batch(im, small, nosq, what, count, rl):
    """rows (5, 4): vpc 256, the fifth ciphertext spills into a second output; columns (3, 512): two outputs"""
    P, K, Or, cc = small
    z = np.random.default_rng(count + rl).uniform(-0.8, 0.8, (count, P.slots))
    cts = G.fresh_scores(P, Or, z, 4)
    if what == "rows":
        want, plain = G.oracle_rows(P, Or, cts, G.ALPHA_DEPTH, rl), G.plain_rows(list(z), rl)
        got, other = cc.alpha_norm_rows(upload(cc, cts), G.ALPHA_DEPTH, rl), nosq.alpha_norm_rows(upload(nosq, cts), G.ALPHA_DEPTH, rl)
    else:
        want, plain = G.oracle_cols(P, Or, cts, G.ALPHA_DEPTH, rl), G.plain_cols(list(z), rl)
        got, other = cc.alpha_norm_columns(upload(cc, cts), G.ALPHA_DEPTH, rl), nosq.alpha_norm_columns(upload(nosq, cts), G.ALPHA_DEPTH, rl)
    assert len(got) == len(want) == (2 if count > 1 else 1)
    assert got.shape() == (len(want), 2, want[0].nl, want[0].scale)
    assert np.array_equal(got.export(), A.stack(want))
    assert np.array_equal(other.export(), A.stack(want))
    assert np.abs(cc.decrypt(got).reshape(-1) - plain).max() < 1e-4  # src/main_accuracy.cpp:359-360


def enrol(im, P, Or, cc, n, planted, seed):
    db, query, cos = database(P, n, planted, seed)
    a, b = db.copy(), db.copy()
    dbcts = A.oracle_enroll(P, Or, a, 99)
    im.BaseEnroller(cc, n).serializeDB(b, seed=99)
    receiver, sender = im.GroteReceiver(cc, n), im.GroteSender(cc, n)
    return dbcts, receiver, sender, receiver.encryptQuery(query, seed=5, nonce=1), Or.encrypt_query(query, 5, 1), cos


@pytest.mark.parametrize("planted", [[23], []])
def test_scenarios_bit_exact_small_ring(im, small, planted):
    P, K, Or, cc = small
    n = 40
    dbcts, receiver, sender, qc, q, cos = enrol(im, P, Or, cc, n, planted, 3)
    scores = A.oracle_compute_similarity(P, Or, q, dbcts)
    assert np.array_equal(sender.computeSimilarity(qc).export(), A.stack(scores))
    want_rows, want_cols = G.oracle_index_scenario(P, Or, scores)
    rows, cols = sender.indexScenario(qc)
    assert np.array_equal(rows.export(), A.stack(want_rows)) and np.array_equal(cols.export(), A.stack(want_cols))
    assert receiver.decryptIndex((rows, cols)) == G.plain_index(G.score_vectors(cos, P.slots)) == planted
    member = sender.membershipScenario(qc)
    want_member = A.oracle_membership_from_index(P, Or, [Or.chebyshev_compare(c) for c in scores])
    assert np.array_equal(member.export()[0], want_member.data())
    assert receiver.decryptMembership(member) is bool(planted)


@pytest.mark.parametrize("planted,want", [([2, 1061], [2, 1061]), ([2, 1061, 1099], [2, 1061, 1067, 1093, 1099])])
def test_two_matrices(im, small, planted, want):
    """n = 1100: 69 database ciphertexts, 2 score ciphertexts.  Three matches, two of them in matrix 1 on different rows and columns,
    decode to the four crossings of matrix 1: the reference's answer.  No two planted vectors share a row or a column of one matrix
    (their sum would leave the comparator's interval)."""
    P, K, Or, cc = small
    n = 1100
    assert G.no_shared_line(planted, P.slots)
    db, query, cos = database(P, n, planted, 11)
    assert G.plain_index(G.score_vectors(cos, P.slots)) == want
    im.BaseEnroller(cc, n).serializeDB(db.copy(), seed=99)
    assert cc.db_stats()[1] == 69
    receiver, sender = im.GroteReceiver(cc, n), im.GroteSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    rows, cols = sender.indexScenario(qc)
    assert (len(sender.computeSimilarity(qc)), len(rows), len(cols)) == (2, 1, 1)
    assert receiver.decryptIndex((rows, cols)) == want


@pytest.mark.parametrize("env", [{"HYDIA_BASE_CHUNK": "1"}, {"HYDIA_BASE_CHUNK": "5"}, {"HYDIA_GROTE_NO_SQ": "1"}])
def test_switches_give_identical_bytes(im, small, env):
    P, K, Or, cc = small
    n = 100
    db, query, _ = database(P, n, [77], 11)

    def run(c):
        im.BaseEnroller(c, n).serializeDB(db.copy(), seed=99)
        receiver, sender = im.GroteReceiver(c, n), im.GroteSender(c, n)
        index = sender.indexScenario(receiver.encryptQuery(query, seed=5, nonce=1))
        assert receiver.decryptIndex(index) == [77]
        return [x.export() for x in index]

    base = run(cc)
    other = make_context(im, env)
    got = run(other)
    other.close()
    for w, g in zip(base, got):
        assert np.array_equal(w, g), env


def test_error_paths(im, small):
    P, K, Or, cc = small
    n = 40
    db, query, _ = database(P, n, [], 3)
    im.BaseEnroller(cc, n).serializeDB(db.copy(), seed=99)
    receiver, sender = im.GroteReceiver(cc, n), im.GroteSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)

    def code(fn, *a):
        with pytest.raises(im.HydiaError) as e:
            fn(*a)
        return e.value.code, str(e.value)

    scores = sender.computeSimilarity(qc)
    assert code(cc.alpha_norm_rows, scores, 2, 48)[0] == -1 and code(cc.alpha_norm_columns, scores, 2, 2 * P.slots)[0] == -1
    assert code(cc.alpha_norm_rows, scores, 2, 1)[0] == -1
    rows, cols = sender.indexScenario(qc)
    assert code(im.GroteReceiver(cc, P.slots * 32 + 1).decryptIndex, (rows, cols))[0] == -1  # two row ciphertexts expected
    two = cc.alpha_norm_columns(cc.import_ct(np.concatenate([scores.export()] * 3), scores.shape()[3]), 2, 512)
    assert len(two) == 2 and code(receiver.decryptIndex, (rows, two))[0] == -1
    # a missing key is named before any work is enqueued
    other = make_context(im, rotations=[r for r in cc.base_rotations() if r != P.slots - 32])
    im.BaseEnroller(other, n).serializeDB(db.copy(), seed=99)
    oq = im.GroteReceiver(other, n).encryptQuery(query, seed=5, nonce=1)
    c, msg = code(im.GroteSender(other, n).indexScenario, oq)
    assert c == -2 and "rotation key %d" % (P.slots - 32) in msg
    c, msg = code(other.alpha_norm_columns, other.import_ct(scores.export(), scores.shape()[3]), 2, 32)
    assert c == -2 and "rotation key %d" % (P.slots - 32) in msg
    # another database kind resident
    other.keygen_rotations(other.base_rotations(), seed=7)
    im.HersEnroller(other, n).serializeDB(db.copy(), seed=99)
    assert other.db_kind() == 4 and code(im.GroteSender(other, n).indexScenario, oq)[0] == -2
    other.close()
    # approach 1's chain (depth 13) is too short for the comparator after the alpha norm
    short = make_context(im, depth=13)
    im.BaseEnroller(short, n).serializeDB(db.copy(), seed=99)
    sq = im.GroteReceiver(short, n).encryptQuery(query, seed=5, nonce=1)
    c, msg = code(im.GroteSender(short, n).indexScenario, sq)
    assert c == -2 and "too short" in msg
    low = im.GroteSender(short, n).computeSimilarity(sq)
    short.level_reduce(low, 5)
    assert code(short.alpha_norm_rows, low, 2, 32)[0] == -2  # 2 + 1 + 2 rescales need more than five limbs
    short.close()


@pytest.mark.slow
def test_full_ring_2p16(im):
    """hydia_params_for_approach(2): N = 2^16, 19 + 6 limbs, rowLength 256.  The first 128 vectors of tests/golden/dataset_2_10.npz (2
    database ciphertexts, the match at 0): rows, columns and membership bit exact against the restatement, decryptIndex == [0].  The
    CPU oracle sets the wall time, which is printed."""
    import time
    g = np.load(os.path.join(GOLDEN, "dataset_2_10.npz"))
    n, query, db = 128, g["query"].astype(np.float64), np.ascontiguousarray(g["db"][:128], dtype=np.float64)
    p = im.params_for_approach(2)
    cc = im.Context(p, 0)
    P = O.Params(log_n=16, depth=18, dim=512)
    assert (cc.nQ, cc.nP, cc.grote_row_length()) == (19, 6, 256) and np.array_equal(cc.moduli, P.moduli)
    K = O.Keys(P, 21, rotations=A.approach1_rotations(P.slots))
    Or = O.Oracle(P, K)
    cc.keygen_rotations(cc.base_rotations(), seed=21)
    a, b = db.copy(), db.copy()
    dbcts = A.oracle_enroll(P, Or, a, 99)
    im.BaseEnroller(cc, n).serializeDB(b, seed=99)
    assert len(dbcts) == 2
    receiver, sender = im.GroteReceiver(cc, n), im.GroteSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    rows, cols = sender.indexScenario(qc)
    assert receiver.decryptIndex((rows, cols)) == [0]
    member = sender.membershipScenario(qc)
    assert receiver.decryptMembership(member) is True
    t0 = time.time()
    scores = A.oracle_compute_similarity(P, Or, Or.encrypt_query(query, 5, 1), dbcts)
    want_rows, want_cols = G.oracle_index_scenario(P, Or, scores)
    want_member = A.oracle_membership_from_index(P, Or, [Or.chebyshev_compare(c) for c in scores])
    print("approach 2, N = 2^16, 128 vectors: restatement %.1f s on the host" % (time.time() - t0))
    assert np.array_equal(rows.export(), A.stack(want_rows)) and np.array_equal(cols.export(), A.stack(want_cols))
    assert np.array_equal(member.export()[0], want_member.data())
    cc.close()
