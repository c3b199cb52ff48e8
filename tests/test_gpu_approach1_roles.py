"""GPU (run with -m gpu): approach 1 (the literature baseline) end to end — BaseEnroller / BaseReceiver / BaseSender, mergeCiphers and
the CLI entry — bit exact against the restatement of tests/approach1_ref.py (the CPU oracle's primitives composed in the reference's
order) unless noted.  Chunk sizes and fused-path switches are compared on EXPORTED BYTES, so a wrong fused kernel fails them."""
import os
import subprocess

import numpy as np
import pytest

import approach1_ref as A
import oracle_lib as O
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TOL = 1e-4  # src/main_accuracy.cpp:359-360


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def make_context(im, seed=7):
    cc = im.Context(im.default_params(log_n=11, mult_depth=13, vector_dim=64), 0)
    cc.keygen_rotations(cc.base_rotations(), seed=seed)
    return cc


@pytest.fixture(scope="module")
def small(im):
    """2^11 ring with approach 1's chain (depth 13: 14 + 5 limbs), 64-dim vectors (vpc 16), the approach-1 key set."""
    P = O.Params(log_n=11, depth=13, dim=64)
    K = O.Keys(P, 7, rotations=A.approach1_rotations(P.slots))
    cc = make_context(im)
    yield P, K, O.Oracle(P, K), cc
    cc.close()


def database(P, n, planted, seed):
    rng = np.random.default_rng(seed)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for i in planted:
        db[i] = rng.integers(1, 4, size=P.dim)
    query = np.ones(P.dim)
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))
    return db, query, cos


def test_enrolment_ragged_bit_exact(im, small):
    P, K, Or, cc = small
    n = 40
    db, _, _ = database(P, n, [23], 3)
    a, b = db.copy(), db.copy()
    want = A.oracle_enroll(P, Or, a, 99)
    im.BaseEnroller(cc, n).serializeDB(b, seed=99)
    assert np.array_equal(a, b)  # normalised in place, the same doubles
    assert cc.db_kind() == 1 and cc.base_db_num_cts(n) == len(want) == 3
    assert cc.db_stats() == (n, 3, 3 * 2 * P.nQ * P.N * 8) and cc.db_residue_bits() == 64
    for t, w in enumerate(want):
        assert np.array_equal(cc.db_export_ct(t), w.data()), t
    with pytest.raises(im.HydiaError) as e:  # no file format for kind 1 (include/hydia.h)
        cc.db_save("/dev/null")
    assert e.value.code == -2


@pytest.mark.parametrize("planted", [[23], []])
def test_sender_bit_exact_small_ring(im, small, planted):
    """n = 40 (3 ciphertexts, ragged): computeSimilarity as the merged batch, indexScenario and membershipScenario bit for bit"""
    P, K, Or, cc = small
    n = 40
    db, query, cos = database(P, n, planted, 3)
    a, b = db.copy(), db.copy()
    dbcts = A.oracle_enroll(P, Or, a, 99)
    im.BaseEnroller(cc, n).serializeDB(b, seed=99)
    receiver, sender = im.BaseReceiver(cc, n), im.BaseSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    q = Or.encrypt_query(query, 5, 1)
    assert np.array_equal(qc.export()[0], q.data())
    sim = sender.computeSimilarity(qc)
    want = A.oracle_compute_similarity(P, Or, q, dbcts)
    assert sim.shape() == (1, 2, P.nQ - 3, want[0].scale)
    assert np.array_equal(sim.export(), A.stack(want))
    scores = cc.decrypt(sim)[0]
    assert max(np.abs(scores[:n] - cos).max(), np.abs(scores[n:]).max()) < TOL
    index = sender.indexScenario(qc)
    want_index = [Or.chebyshev_compare(c) for c in want]
    assert np.array_equal(index.export(), A.stack(want_index))
    assert receiver.decryptIndex(index) == planted
    member = sender.membershipScenario(qc)
    assert np.array_equal(member.export()[0], A.oracle_membership_from_index(P, Or, want_index).data())
    assert receiver.decryptMembership(member) is bool(planted)


@pytest.mark.parametrize("dimension,count", [(64, 3), (16, 2), (16, 17)])
def test_merge_ciphers_on_a_callers_batch(im, small, dimension, count):
    """dimension 16 gives vpc 64 and three mask multiplies (segments 1, 16, 64); 17 ciphertexts at vpc 64 spill into a second output"""
    P, K, Or, cc = small
    rng = np.random.default_rng(dimension + count)
    z = rng.uniform(-1, 1, (count, P.slots))
    cts = [Or.encrypt(v, 4, 50 + i) for i, v in enumerate(z)]
    got = cc.merge_ciphers(cc.import_ct(A.stack(cts), cts[0].scale), dimension)
    want = A.oracle_merge_ciphers(P, Or, cts, dimension)
    assert np.array_equal(got.export(), A.stack(want))
    flat = cc.decrypt(got).reshape(-1)
    picked = z[:, ::dimension].reshape(-1)
    assert np.abs(flat[:picked.size] - picked).max() < 1e-5 and np.abs(flat[picked.size:]).max() < 1e-5


VARIANTS = [{"HYDIA_BASE_CHUNK": "1"}, {"HYDIA_BASE_CHUNK": "2"}, {"HYDIA_BASE_CHUNK": "5"}, {"HYDIA_BASE_NO_ROTADD": "1"},
            {"HYDIA_BASE_NO_BCAST": "1"}, {"HYDIA_BASE_NO_BCAST": "1", "HYDIA_BASE_NO_ROTADD": "1", "HYDIA_BASE_CHUNK": "3"}]


def test_chunks_and_switches_give_identical_bytes(im, small, monkeypatch):
    """the same database (7 ciphertexts, ragged) with the automatic chunk, chunks of 1, 2, 5 and each fused path off: the exported
    bytes of computeSimilarity, indexScenario and membershipScenario are those of the default context"""
    P, K, Or, cc = small
    n = 100
    db, query, _ = database(P, n, [77], 11)

    def run(c):
        im.BaseEnroller(c, n).serializeDB(db.copy(), seed=99)
        receiver, sender = im.BaseReceiver(c, n), im.BaseSender(c, n)
        qc = receiver.encryptQuery(query, seed=5, nonce=1)
        index = sender.indexScenario(qc)
        assert receiver.decryptIndex(index) == [77]
        return sender.computeSimilarity(qc).export(), index.export(), sender.membershipScenario(qc).export(), c.eval_sum(qc).export()

    base = run(cc)
    for env in VARIANTS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        other = make_context(im)
        for k in env:
            monkeypatch.delenv(k)
        got = run(other)
        other.close()
        for w, g in zip(base, got):
            assert np.array_equal(w, g), env


def test_database_larger_than_one_output(im, small):
    """n = 1024 + 17 vectors: 66 ciphertexts of 16 scores, two outputs, the second ragged; global indices; a chunk boundary (7 does
    not divide 64) falls inside the first output"""
    P, K, Or, cc = small
    n = P.slots + 17
    planted = [5, P.slots - 1, P.slots + 9]
    db, query, cos = database(P, n, planted, 21)
    a, b = db.copy(), db.copy()
    dbcts = A.oracle_enroll(P, Or, a, 99)
    assert len(dbcts) == 66
    im.BaseEnroller(cc, n).serializeDB(b, seed=99)
    receiver, sender = im.BaseReceiver(cc, n), im.BaseSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    sim = sender.computeSimilarity(qc)
    want = A.oracle_compute_similarity(P, Or, Or.encrypt_query(query, 5, 1), dbcts)
    assert len(sim) == len(want) == 2
    assert np.array_equal(sim.export(), A.stack(want))
    scores = cc.decrypt(sim).reshape(-1)
    assert np.abs(scores[:n] - cos).max() < TOL and np.abs(scores[n:]).max() < TOL
    assert receiver.decryptIndex(sender.indexScenario(qc)) == planted
    assert receiver.decryptMembership(sender.membershipScenario(qc)) is True


def test_chunk_boundary_inside_an_output(im, small, monkeypatch):
    P, K, Or, cc = small
    n = P.slots + 17
    db, query, _ = database(P, n, [5], 21)
    im.BaseEnroller(cc, n).serializeDB(db.copy(), seed=99)
    qc = im.BaseReceiver(cc, n).encryptQuery(query, seed=5, nonce=1)
    want = im.BaseSender(cc, n).computeSimilarity(qc).export()
    monkeypatch.setenv("HYDIA_BASE_CHUNK", "7")
    other = make_context(im)
    monkeypatch.delenv("HYDIA_BASE_CHUNK")
    im.BaseEnroller(other, n).serializeDB(db.copy(), seed=99)
    got = im.BaseSender(other, n).computeSimilarity(im.BaseReceiver(other, n).encryptQuery(query, seed=5, nonce=1)).export()
    other.close()
    assert np.array_equal(want, got)


def test_error_paths(im, small):
    P, K, Or, cc = small
    n = 40
    db, query, _ = database(P, n, [], 3)
    im.BaseEnroller(cc, n).serializeDB(db.copy(), seed=99)
    qc = im.BaseReceiver(cc, n).encryptQuery(query, seed=5, nonce=1)

    def code(fn, *a):
        with pytest.raises(im.HydiaError) as e:
            fn(*a)
        return e.value.code, str(e.value)

    # a diagonal-sender or HERS call on a row-packed database
    assert code(im.DiagonalSender(cc, n).computeSimilarity, qc)[0] == -2
    assert code(im.HersSender(cc, n).computeSimilarity, qc)[0] == -2
    # wrong query shape: two ciphertexts; a 3-component one; one below full level
    two = cc.encrypt(np.zeros((2, P.slots)), seed=1, nonce0=5)
    assert code(im.BaseSender(cc, n).computeSimilarity, two)[0] == -1
    assert code(im.BaseSender(cc, n).indexScenario, cc.eval_mult_no_relin(qc, qc))[0] == -1
    low = cc.encrypt(np.zeros(P.slots), seed=1, nonce0=9)
    cc.rescale(low)
    assert code(im.BaseSender(cc, n).membershipScenario, low)[0] == -1
    assert code(cc.merge_ciphers, qc, 48)[0] == -1 and code(cc.merge_ciphers, qc, 2 * P.slots)[0] == -1
    # a missing key is named before any work is enqueued; another database kind resident
    other = im.Context(im.default_params(log_n=11, mult_depth=13, vector_dim=64), 0)
    other.keygen_rotations([r for r in other.base_rotations() if r != P.slots - 1], seed=7)
    im.BaseEnroller(other, n).serializeDB(db.copy(), seed=99)
    oq = im.BaseReceiver(other, n).encryptQuery(query, seed=5, nonce=1)
    c, msg = code(im.BaseSender(other, n).computeSimilarity, oq)
    assert c == -2 and "rotation key %d" % (P.slots - 1) in msg
    assert code(other.merge_ciphers, oq, 64)[0] == -2
    other.keygen_rotations(other.base_rotations(), seed=7)
    im.HersEnroller(other, n).serializeDB(db.copy(), seed=99)
    assert other.db_kind() == 4 and code(im.BaseSender(other, n).computeSimilarity, oq)[0] == -2
    other.close()
    # a vector_dim that is not a power of two never reaches enrolment: the context refuses it
    assert code(im.Context, im.default_params(log_n=11, mult_depth=13, vector_dim=48), 0)[0] == -1


def test_full_ring_2p16_dataset_2_10(im):
    """hydia_params_for_approach(1): N = 2^16, dim 512, vpc 64.  tests/golden/dataset_2_10.npz (1024 vectors, 16 database ciphertexts)
    through the roles: membership true, index [0], all 1024 scores within 1e-4 of plaintext cosine; the merged result of all 16
    ciphertexts, the comparator's output and the membership ciphertext bit exact against the restatement (nothing left out).
    The C-ABI exposes no per-ciphertext result of steps 3-4, so the separate comparison of the first two database ciphertexts through
    those steps is replaced by the merged result of all 16, which every ciphertext's steps 3-4 enter (and by the exported database
    ciphertexts 0 and 15).  The restatement's wall time is printed (about 2 minutes on 8 host cores)."""
    import time
    g = np.load(os.path.join(GOLDEN, "dataset_2_10.npz"))
    n, query, db = int(g["n"]), g["query"].astype(np.float64), np.ascontiguousarray(g["db"], dtype=np.float64)
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))
    p = im.params_for_approach(1)
    cc = im.Context(p, 0)
    P = O.Params(log_n=16, depth=13, dim=512)
    assert cc.base_rotations() == A.approach1_rotations(P.slots)
    K = O.Keys(P, 21, rotations=A.approach1_rotations(P.slots))
    Or = O.Oracle(P, K)
    cc.keygen_rotations(cc.base_rotations(), seed=21)
    a, b = db.copy(), db.copy()
    dbcts = A.oracle_enroll(P, Or, a, 99)
    im.BaseEnroller(cc, n).serializeDB(b, seed=99)
    assert len(dbcts) == 16 and cc.db_stats()[1] == 16
    for t in (0, 15):
        assert np.array_equal(cc.db_export_ct(t), dbcts[t].data()), t
    receiver, sender = im.BaseReceiver(cc, n), im.BaseSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    q = Or.encrypt_query(query, 5, 1)
    sim = sender.computeSimilarity(qc)
    scores = cc.decrypt(sim)[0]
    err = max(np.abs(scores[:n] - cos).max(), np.abs(scores[n:]).max())
    print("approach 1, N = 2^16, 2_10: max score error %.3e" % err)
    assert err < TOL
    index = sender.indexScenario(qc)
    assert receiver.decryptIndex(index) == [0]
    member = sender.membershipScenario(qc)
    assert receiver.decryptMembership(member) is True
    t0 = time.time()
    want = A.oracle_compute_similarity(P, Or, q, dbcts)
    want_index = [Or.chebyshev_compare(want[0])]
    print("approach 1, N = 2^16, 2_10: restatement (16 ciphertexts + comparator) %.1f s on the host" % (time.time() - t0))
    assert len(sim) == len(want) == 1 and np.array_equal(sim.export()[0], want[0].data())
    assert np.array_equal(index.export()[0], want_index[0].data())
    assert np.array_equal(member.export()[0], A.oracle_membership_from_index(P, Or, want_index).data())
    cc.close()


def test_cli_approach_1_on_reference_dataset(tmp_path):
    """./ImageMatching 2_10.dat 1 through the C++ Base* roles: stdout and the latency.csv row"""
    exe = os.path.join(ROOT, "image_matching_amd", "ImageMatching")
    assert os.path.exists(exe), "CLI not built"
    g = np.load(os.path.join(GOLDEN, "dataset_2_10.npz"))
    dat = tmp_path / "2_10.dat"
    with open(dat, "w") as f:
        f.write("%d\n" % int(g["n"]))
        f.write(" ".join(str(int(v)) for v in g["query"]) + " \n")
        for row in g["db"]:
            f.write(" ".join(str(int(v)) for v in row) + " \n")
    (tmp_path / "latency.csv").write_text("")
    out = subprocess.run([exe, str(dat), "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "Experimental approach: Literature baseline" in out.stdout
    assert "Membership scenario: true" in out.stdout and "Index scenario: [ 0 ]" in out.stdout
    row = (tmp_path / "latency.csv").read_text().strip().split(",")
    assert row[0] == "Baseline" and row[1] == "1024" and row[10] == "true" and row[11] == "[ 0 ]"
