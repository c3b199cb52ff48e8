"""GPU (run with -m gpu): approach 3 (the Blind-Match method) end to end — BlindEnroller / BlindReceiver / BlindSender, the fused
sum-of-products kernel and compressCiphers — bit exact on exported residues against the restatement of
tests/approach3_ref.py (the CPU oracle's primitives composed in the reference's order) unless noted.  Pass sizes and the fused-path
switch are compared on EXPORTED BYTES, so a wrong fused kernel fails them.  There is no CLI test: tests/test_gpu_client.py pins
`./ImageMatching <file> 3` to the refusal, so the CLI has no approach-3 entry.  Small ring: N = 2^11, depth 12 (13 + 5 limbs), dim 64,
chunk_len 16: K = 4 chunks, 64 vectors per matrix."""
import os

import numpy as np
import pytest

import approach1_ref as A
import approach3_ref as B
import oracle_lib as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
TOL = 1e-4  # src/main_accuracy.cpp:359-360
CHUNK = 16


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def make_context(im, env=None, rotations=None, seed=7, dim=64):
    """a 2^11 context on approach 3's chain with approach 1's key set; env: switches read once at creation"""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        cc = im.Context(im.default_params(log_n=11, mult_depth=12, vector_dim=dim), 0)
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
    P = O.Params(log_n=11, depth=12, dim=64)
    K = O.Keys(P, 7, rotations=A.approach1_rotations(P.slots))
    cc = make_context(im)
    assert (cc.nQ, cc.nP) == (P.nQ, P.nP) == (13, 5)
    yield P, K, O.Oracle(P, K), cc
    cc.close()


@pytest.fixture(scope="module")
def nodot(im):
    cc = make_context(im, {"HYDIA_BLIND_NO_DOT": "1"})
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


def roles(im, cc, n):
    return im.BlindReceiver(cc, n, CHUNK), im.BlindSender(cc, n)


def scores_at_decoded_slots(P, cos, outputs):
    want = np.zeros((outputs, P.slots))
    for i, c in enumerate(cos):
        want[B.score_slot(i, P.slots, CHUNK)] = c
    return want


def test_enrolment_ragged_bit_exact(im, small):
    """n = 100: 2 matrices, 8 ciphertexts, the second matrix ragged; the same doubles after the in-place normalisation"""
    P, K, Or, cc = small
    n = 100
    db, _, _ = database(P, n, [77], 3)
    a, b = db.copy(), db.copy()
    want = B.oracle_enroll(P, Or, a, CHUNK, 99)
    im.BlindEnroller(cc, n).serializeDB(b, CHUNK, seed=99)
    assert np.array_equal(a, b)
    assert cc.db_kind() == 3 and cc.blind_db_num_cts(n, CHUNK) == 8 and len(want) == 2
    assert cc.db_stats() == (n, 8, 8 * 2 * P.nQ * P.N * 8) and cc.db_residue_bits() == 64
    for m, cts in enumerate(want):
        for c, w in enumerate(cts):
            assert np.array_equal(cc.db_export_ct(m * 4 + c), w.data()), (m, c)
    with pytest.raises(im.HydiaError) as e:  # no file format for kind 3 (include/hydia.h)
        cc.db_save("/dev/null")
    assert e.value.code == -2


@pytest.mark.parametrize("K", [1, 4, 8])
def test_dot_kernel_on_saturated_residues(im, small, nodot, K):
    """every residue of q and b is q_j - 1, M = 5 matrices (a ragged last group: a thread walks two): d0 and d2 sum K products of
    (q_j - 1)^2, d1 sums 2K — 8 at K = 4, 16 at K = 8, past the four-product range of the cheap reduction on the 60-bit limb 0.
    Against Python integers on every limb, and against the unfused path"""
    P, _, _, cc = small
    M = 5
    sat = (P.moduli[:P.nQ] - np.uint64(1))[None, None, :, None]
    q = np.broadcast_to(sat, (K, 2, P.nQ, P.N))
    b = np.broadcast_to(sat, (M * K, 2, P.nQ, P.N))
    want = np.zeros((M, 3, P.nQ, P.N), dtype=np.uint64)
    for j in range(P.nQ):
        m = int(P.moduli[j])
        assert j > 0 or m.bit_length() == 60
        want[:, 0, j] = want[:, 2, j] = (K * (m - 1) * (m - 1)) % m
        want[:, 1, j] = (2 * K * (m - 1) * (m - 1)) % m
    got = cc.eval_dot_no_relin(cc.import_ct(q, P.delta), cc.import_ct(b, P.delta))
    assert got.shape() == (M, 3, P.nQ, P.delta * P.delta)
    assert np.array_equal(got.export(), want)
    assert np.array_equal(nodot.eval_dot_no_relin(nodot.import_ct(q, P.delta), nodot.import_ct(b, P.delta)).export(), want)


def test_dot_kernel_on_limb_strided_inputs(im, small, nodot):
    """random residues (fresh ciphertexts), K = 4, M = 3, both operands as views of the first n_q - 5 limbs read in place (limb stride
    != limbs): the oracle's four products summed in ascending c, on those limbs"""
    P, _, Or, cc = small
    K, M, nl = 4, 3, P.nQ - 5
    rng = np.random.default_rng(12)
    qs = [Or.encrypt(rng.uniform(-1, 1, P.slots), 4, 30 + i) for i in range(K)]
    bs = [Or.encrypt(rng.uniform(-1, 1, P.slots), 4, 60 + i) for i in range(M * K)]
    prods = [B.oracle_dot_norelin(P, Or, qs, bs[m * K:(m + 1) * K]) for m in range(M)]  # data() is a view: the ciphertexts stay alive
    want = np.stack([p.data()[:, :nl] for p in prods])
    for c in (cc, nodot):
        q, b = upload(c, qs), upload(c, bs)
        got = c.eval_dot_no_relin(c.ct_limb_prefix(q, nl), c.ct_limb_prefix(b, nl))
        assert got.shape()[:3] == (M, 3, nl)
        assert np.array_equal(got.export(), want)


@pytest.mark.parametrize("planted", [[77], []])
def test_sender_bit_exact_small_ring(im, small, planted):
    """n = 100 (2 matrices, ragged): computeSimilarity, indexScenario and membershipScenario bit for bit"""
    P, K, Or, cc = small
    n = 100
    db, query, cos = database(P, n, planted, 3)
    a, b = db.copy(), db.copy()
    dbcts = B.oracle_enroll(P, Or, a, CHUNK, 99)
    im.BlindEnroller(cc, n).serializeDB(b, CHUNK, seed=99)
    receiver, sender = roles(im, cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    qs = B.oracle_encrypt_query(P, Or, query, CHUNK, 5, 1)
    assert np.array_equal(qc.export(), A.stack(qs))
    sim = sender.computeSimilarity(qc)
    want = B.oracle_compute_similarity(P, Or, qs, dbcts, CHUNK)
    assert sim.shape() == (1, 2, P.nQ - 2, want[0].scale)
    assert np.array_equal(sim.export(), A.stack(want))
    assert np.abs(cc.decrypt(sim) - scores_at_decoded_slots(P, cos, 1)).max() < TOL
    index = sender.indexScenario(qc)
    want_index = B.oracle_index_scenario(P, Or, want)
    assert np.array_equal(index.export(), A.stack(want_index))
    assert receiver.decryptIndex(index) == planted
    member = sender.membershipScenario(qc)
    assert np.array_equal(member.export()[0], A.oracle_membership_from_index(P, Or, want_index).data())
    assert receiver.decryptMembership(member) is bool(planted)


def test_spill_into_a_second_output(im, small):
    """n = 17 * 64 - 30: 17 matrices, the last ragged, a second compressed ciphertext; matches in matrix 0, in matrix 16 and at an
    offset != 0 inside a matrix: the -(i mod chunk_len) placements and the decode across outputs"""
    P, K, Or, cc = small
    n = 17 * 64 - 30
    planted = [5, 9 * 64 + 33, 16 * 64 + 2]
    db, query, cos = database(P, n, planted, 21)
    a, b = db.copy(), db.copy()
    dbcts = B.oracle_enroll(P, Or, a, CHUNK, 99)
    assert len(dbcts) == 17
    im.BlindEnroller(cc, n).serializeDB(b, CHUNK, seed=99)
    receiver, sender = roles(im, cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    sim = sender.computeSimilarity(qc)
    want = B.oracle_compute_similarity(P, Or, B.oracle_encrypt_query(P, Or, query, CHUNK, 5, 1), dbcts, CHUNK)
    assert len(sim) == len(want) == 2
    assert np.array_equal(sim.export(), A.stack(want))
    assert np.abs(cc.decrypt(sim) - scores_at_decoded_slots(P, cos, 2)).max() < TOL
    # decryptIndex walks output 0 slot by slot, then output 1: vector 9*64+33 sits at slot 33*16+9, vector 5 at slot 5*16
    assert receiver.decryptIndex(sender.indexScenario(qc)) == [5, 9 * 64 + 33, 16 * 64 + 2]
    assert receiver.decryptMembership(sender.membershipScenario(qc)) is True


@pytest.mark.parametrize("dimension,count", [(16, 3), (4, 5), (16, 17)])
def test_compress_ciphers_on_a_callers_batch(im, small, dimension, count):
    """(4, 5) and (16, 17) spill into a second output"""
    P, K, Or, cc = small
    rng = np.random.default_rng(dimension + count)
    z = rng.uniform(-1, 1, (count, P.slots))
    cts = [Or.encrypt(v, 4, 50 + i) for i, v in enumerate(z)]
    got = cc.compress_ciphers(upload(cc, cts), dimension)
    want = B.oracle_compress(P, Or, cts, dimension)
    assert np.array_equal(got.export(), A.stack(want))
    plain = np.stack(B.plain_compress(list(z), dimension))
    assert np.abs(cc.decrypt(got) - plain).max() < 1e-5


VARIANTS = [{"HYDIA_BLIND_PASS": "1"}, {"HYDIA_BLIND_PASS": "2"}, {"HYDIA_BLIND_PASS": "5"}, {"HYDIA_BLIND_NO_DOT": "1"},
            {"HYDIA_BLIND_NO_DOT": "1", "HYDIA_BLIND_PASS": "3"}]


def test_passes_and_switches_give_identical_bytes(im, small):
    """the same database (7 matrices, ragged) with the automatic pass, passes of 1, 2, 5 matrices and the fused product off: the
    exported bytes of computeSimilarity, indexScenario and membershipScenario are those of the default context"""
    P, K, Or, cc = small
    n = 6 * 64 + 20
    db, query, _ = database(P, n, [5 * 64 + 7], 11)

    def run(c):
        im.BlindEnroller(c, n).serializeDB(db.copy(), CHUNK, seed=99)
        receiver, sender = roles(im, c, n)
        qc = receiver.encryptQuery(query, seed=5, nonce=1)
        index = sender.indexScenario(qc)
        assert receiver.decryptIndex(index) == [5 * 64 + 7]
        return sender.computeSimilarity(qc).export(), index.export(), sender.membershipScenario(qc).export()

    base = run(cc)
    for env in VARIANTS:
        other = make_context(im, env)
        got = run(other)
        other.close()
        for w, g in zip(base, got):
            assert np.array_equal(w, g), env


def test_error_paths(im, small):
    P, K, Or, cc = small
    n = 100
    db, query, _ = database(P, n, [], 3)

    def code(fn, *a, **kw):
        with pytest.raises(im.HydiaError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    other = make_context(im, rotations=[r for r in cc.base_rotations() if r != P.slots - 1])
    receiver, sender = roles(im, other, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    # no database; an approach-1 database resident
    assert code(sender.computeSimilarity, qc)[0] == -2
    im.BaseEnroller(other, n).serializeDB(db.copy(), seed=99)
    assert other.db_kind() == 1 and code(sender.indexScenario, qc)[0] == -2
    # a chunk length that is not a power of two, does not divide dim, or gives is below 2
    for bad in (12, 128, 0, 1):
        assert code(im.BlindEnroller(other, n).serializeDB, db.copy(), bad, seed=99)[0] == -1, bad
        assert code(im.BlindReceiver(other, n, bad).encryptQuery, query, seed=5)[0] == -1, bad
        assert other.blind_db_num_cts(n, bad) == 0
    assert other.db_kind() == 1  # a refused enrolment leaves the resident database alone
    wide = make_context(im, dim=128, rotations=[1])
    assert code(im.BlindEnroller(wide, 4).serializeDB, np.ones((4, 128)), 2, seed=1)[0] == -1  # K = 64 > 32
    many = wide.encrypt(np.zeros((33, P.slots)), seed=1, nonce0=5)
    assert code(wide.eval_dot_no_relin, many, many)[0] == -1
    wide.close()
    # a missing key is named before any work is enqueued
    im.BlindEnroller(other, n).serializeDB(db.copy(), CHUNK, seed=99)
    c, msg = code(sender.computeSimilarity, qc)
    assert c == -2 and "rotation key %d" % (P.slots - 1) in msg
    assert code(other.compress_ciphers, qc, CHUNK)[0] == -2
    other.keygen_rotations(other.base_rotations(), seed=7)
    # a query of the wrong count; a 3-component one; one below full level
    three = other.encrypt(np.zeros((3, P.slots)), seed=1, nonce0=5)
    assert code(sender.computeSimilarity, three)[0] == -1
    assert code(sender.indexScenario, other.eval_mult_no_relin(qc, qc))[0] == -1
    low = other.encrypt(np.zeros((4, P.slots)), seed=1, nonce0=9)
    other.rescale(low)
    assert code(sender.membershipScenario, low)[0] == -1
    assert code(other.compress_ciphers, qc, 48)[0] == -1 and code(other.compress_ciphers, qc, 2 * P.slots)[0] == -1
    assert code(other.eval_dot_no_relin, qc, three)[0] == -1
    # the context is still usable: the query it could not answer before now decodes
    assert receiver.decryptIndex(sender.indexScenario(qc)) == []
    # other senders refuse a chunk-packed database
    assert code(im.BaseSender(other, n).computeSimilarity, other.encrypt(np.zeros(P.slots), seed=1, nonce0=3))[0] == -2
    other.close()


def test_full_ring_2p16(im):
    """hydia_params_for_approach(3): N = 2^16, 13 + 5 limbs, dim 512, chunk_len 128 (K = 4, 256 vectors per matrix).  The first 300
    vectors of tests/golden/dataset_2_10.npz (2 matrices, the second ragged, the match at 0): indexScenario bit exact against the
    restatement, decryptIndex == [0], membership true.  The CPU oracle sets the wall time, which is printed."""
    import time
    g = np.load(os.path.join(GOLDEN, "dataset_2_10.npz"))
    n, query, db = 300, g["query"].astype(np.float64), np.ascontiguousarray(g["db"][:300], dtype=np.float64)
    p = im.params_for_approach(3)
    cc = im.Context(p, 0)
    P = O.Params(log_n=16, depth=12, dim=512)
    assert (cc.nQ, cc.nP) == (13, 5) and np.array_equal(cc.moduli, P.moduli)
    K = O.Keys(P, 21, rotations=A.approach1_rotations(P.slots))
    Or = O.Oracle(P, K)
    cc.keygen_rotations(cc.base_rotations(), seed=21)
    a, b = db.copy(), db.copy()
    dbcts = B.oracle_enroll(P, Or, a, B.CHUNK_LEN, 99)
    im.BlindEnroller(cc, n).serializeDB(b, seed=99)
    assert len(dbcts) == 2 and cc.db_stats()[1] == 8 and np.array_equal(a, b)
    receiver, sender = im.BlindReceiver(cc, n), im.BlindSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    index = sender.indexScenario(qc)
    assert receiver.decryptIndex(index) == [0]
    assert receiver.decryptMembership(sender.membershipScenario(qc)) is True
    t0 = time.time()
    scores = B.oracle_compute_similarity(P, Or, B.oracle_encrypt_query(P, Or, query, B.CHUNK_LEN, 5, 1), dbcts, B.CHUNK_LEN)
    want_index = B.oracle_index_scenario(P, Or, scores)
    print("approach 3, N = 2^16, 300 vectors: restatement %.1f s on the host" % (time.time() - t0))
    assert len(index) == 1 and np.array_equal(index.export()[0], want_index[0].data())
    cc.close()
