"""GPU parity of the receiver / enroller / key-generation side (run with -m gpu): ChaCha20-addressed sampling, CKKS
encode/decode, encryption, decryption and DiagonalEnroller packing on the GPU against the CPU oracle — bit exact on
ciphertext residues; decoded doubles are compared exactly as well (same IEEE operation order, no contraction).  The data here is
generated; the edges of decryption, decoding, the threshold and the encoder's rounding are in tests/test_gpu_client_edges.py."""
import os

import numpy as np
import pytest

import oracle_lib as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module")
def small(im):
    P = O.Params(log_n=11, depth=11, dim=64)
    K = O.Keys(P, 7)
    cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    cc.keygen(7)
    yield P, K, O.Oracle(P, K), cc
    cc.close()


def test_keygen_bit_exact(small):
    P, K, Or, cc = small
    assert np.array_equal(cc.export_secret_key(), K.s_ntt())
    assert np.array_equal(cc.export_public_key(), K.pk())
    assert np.array_equal(cc.export_eval_key(0), K.relin())
    for r in (1, 2, 63, 64, 512):
        assert np.array_equal(cc.export_eval_key(r), K.rot_key(r)), r
    assert all(cc.has_eval_key(r) for r in K.rotations) and not cc.has_eval_key(65)


def test_encrypt_decrypt_bit_exact(small):
    P, K, Or, cc = small
    rng = np.random.default_rng(2)
    z = rng.uniform(-1, 1, (3, P.slots))
    z[2] = 0.0
    g = cc.encrypt(z, 11, 40)
    data = g.export()
    for i in range(3):
        want = Or.encrypt(z[i], 11, 40 + i)
        assert np.array_equal(data[i], want.data()), i
    dec = cc.decrypt(g)
    for i in range(3):
        assert np.array_equal(dec[i], Or.decrypt(Or.encrypt(z[i], 11, 40 + i)))
        assert np.abs(dec[i] - z[i]).max() < 1e-7
    # decrypt at lower levels / 3-component / single limb
    a = Or.encrypt(z[0], 1, 1)
    d = Or.mult_norelin(a, a)
    assert np.array_equal(cc.decrypt(cc.import_ct(d.data(), d.scale))[0], Or.decrypt(d))
    cur = a
    while cur.nl > 1:
        cur = Or.mult(cur, cur)
    assert np.array_equal(cc.decrypt(cc.import_ct(cur.data(), cur.scale))[0], Or.decrypt(cur))


@pytest.mark.parametrize("n", [1, 64, 1000, 1024, 1500])
def test_enroller_bit_exact(im, small, n):
    P, K, Or, cc = small
    rng = np.random.default_rng(n)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    if n > 10:
        db[7] = 0.0  # zero vector passes through normalisation
    a, b = db.copy(), db.copy()
    dbc = Or.enroll(a, 99)
    im.DiagonalEnroller(cc, n).serializeDB(b, seed=99)
    assert np.array_equal(a, b)  # both normalise in place (enroller_diag.cpp:32-35)
    assert cc.db_stats()[:2] == (n, len(dbc))
    for t in sorted(set([0, 1, P.dim - 1, len(dbc) - 1, len(dbc) // 2])):
        assert np.array_equal(cc.db_export_ct(t), dbc[t].data()), t


def test_query_encryption_bit_exact(im, small):
    P, K, Or, cc = small
    q = np.arange(1.0, P.dim + 1)
    g = im.DiagonalReceiver(cc, 10).encryptQuery(q, seed=5, nonce=1)
    assert np.array_equal(g.export()[0], Or.encrypt_query(q, 5, 1).data())


@pytest.mark.parametrize("n,matches", [(1500, [0, 700, 1499]), (1024, []), (3, [2])])
def test_end_to_end_on_gpu_small_ring(im, small, n, matches):
    """The reference driver's flow (src/main.cpp:245-374) with every step on the GPU."""
    P, K, Or, cc = small
    rng = np.random.default_rng(n + 1)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for i in matches:
        db[i] = rng.integers(1, 4, size=P.dim)
    query = np.ones(P.dim)
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))
    im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=99)
    receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    scores = cc.decrypt(sender.computeSimilarity(qc)).reshape(-1)
    assert np.abs(scores[:n] - cos).max() < TOL
    assert receiver.decryptMembership(sender.membershipScenario(qc)) == (len(matches) > 0)
    assert receiver.decryptIndex(sender.indexScenario(qc)) == sorted(matches)


def test_reference_datasets_end_to_end_full_ring(im):
    """./ImageMatching ../test/2_10.dat 5 and 2_11.dat entirely on the GPU: expected `true`, `[0]`, scores within 1e-4."""
    cc = im.Context()
    cc.keygen(20250725)
    for name in ("2_10", "2_11"):
        g = np.load(os.path.join(GOLDEN, "dataset_%s.npz" % name))
        n, query, db = int(g["n"]), g["query"].astype(np.float64), g["db"].astype(np.float64)
        im.DiagonalEnroller(cc, n).serializeDB(db, seed=99)
        receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
        qc = receiver.encryptQuery(query, seed=5, nonce=1)
        scores = cc.decrypt(sender.computeSimilarity(qc))[0]
        assert np.abs(scores[:n] - g["cosine"]).max() < TOL and np.abs(scores[n:]).max() < TOL
        assert receiver.decryptMembership(sender.membershipScenario(qc)) is True
        assert receiver.decryptIndex(sender.indexScenario(qc)) == [0]
    cc.close()


@pytest.mark.parametrize("n", [40000, 70000])
def test_multi_block_full_ring_end_to_end(im, n):
    """G = 3 and G = 5 blocks at N = 2^15 (odd block counts exercise the loop-B launch fallbacks and the batched comparator):
    decrypted scores vs plaintext cosine (1e-4, src/main_accuracy.cpp:359-360), index = planted matches, membership true."""
    cc = im.Context()
    cc.keygen(11)
    rng = np.random.default_rng(n)
    db = rng.integers(-99, 100, size=(n, 512)).astype(np.float64)
    planted = sorted([3, 16384 + 77, n - 1])
    for i in planted:
        db[i] = rng.integers(1, 4, size=512)
    query = np.ones(512)
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))
    im.DiagonalEnroller(cc, n).serializeDB(db, seed=3)
    receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5, nonce=1)
    sim = sender.computeSimilarity(qc)
    assert len(sim) == -(-n // 16384)
    scores = cc.decrypt(sim).reshape(-1)
    assert np.abs(scores[:n] - cos).max() < TOL and np.abs(scores[n:]).max() < TOL
    assert receiver.decryptIndex(sender.indexScenario(qc)) == planted
    assert receiver.decryptMembership(sender.membershipScenario(qc)) is True
    cc.close()


def test_cli_image_matching_on_reference_dataset(tmp_path):
    """./ImageMatching ../test/2_10.dat 5 (BASELINE config 1) through the C++ role classes: stdout and latency.csv row."""
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "image_matching_amd", "ImageMatching")
    if not os.path.exists(exe):
        pytest.skip("CLI not built")
    g = np.load(os.path.join(GOLDEN, "dataset_2_10.npz"))
    dat = tmp_path / "2_10.dat"
    with open(dat, "w") as f:
        f.write("%d\n" % int(g["n"]))
        f.write(" ".join(str(int(v)) for v in g["query"]) + " \n")
        for row in g["db"]:
            f.write(" ".join(str(int(v)) for v in row) + " \n")
    (tmp_path / "latency.csv").write_text("")
    out = subprocess.run([exe, str(dat), "5"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "Membership scenario: true" in out.stdout and "Index scenario: [ 0 ]" in out.stdout
    row = (tmp_path / "latency.csv").read_text().strip().split(",")
    assert row[0] == "Diagonal" and row[1] == "1024" and row[10] == "true" and row[11] == "[ 0 ]"
    # approach 4 (HERS) on the same stack
    out = subprocess.run([exe, str(dat), "4"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "Membership scenario: true" in out.stdout and "Index scenario: [ 0 ]" in out.stdout
    # approaches 1-3 are not part of this framework: explicit refusal, no silent fallback
    out = subprocess.run([exe, str(dat), "3"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "only approach 5" in out.stderr


@pytest.mark.parametrize("n,matches", [(1300, [0, 1299]), (5, [2])])
def test_hers_bit_exact_small_ring(im, small, n, matches):
    """Approach 4 (HERS): enrolment, the vector_dim query ciphertexts, similarity, index and membership on
    the GPU, bit exact against the oracle's restatement of src/{enroller,receiver,sender}/*_hers.cpp."""
    P, K, Or, cc = small
    rng = np.random.default_rng(n + 7)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for i in matches:
        db[i] = rng.integers(1, 4, size=P.dim)
    query = np.ones(P.dim)
    a, b = db.copy(), db.copy()
    dbc = Or.hers_enroll(a, 4)
    im.HersEnroller(cc, n).serializeDB(b, seed=4)
    assert np.array_equal(a, b) and cc.db_stats()[1] == len(dbc)
    for t in sorted(set([0, 3, len(dbc) - 1])):
        assert np.array_equal(cc.db_export_ct(t), dbc[t].data()), t
    q = Or.hers_encrypt_query(query, 6, 1000)
    gq = im.HersReceiver(cc, n).encryptQuery(query, seed=6, nonce=1000)
    gqd = gq.export()
    for i in (0, 1, P.dim - 1):
        assert np.array_equal(gqd[i], q[i].data()), i
    sender = im.HersSender(cc, n)
    sim, gsim = Or.hers_compute_similarity(q, dbc, n), sender.computeSimilarity(gq).export()
    for g in range(len(sim)):
        assert np.array_equal(gsim[g], sim[g].data())
    idx, gidx = Or.hers_index_scenario(q, dbc, n), sender.indexScenario(gq)
    assert np.array_equal(gidx.export()[0], idx[0].data())
    # (small vector_dim: a random row may legitimately clear 0.44, so the expectation is the oracle's own decryption)
    found = im.DiagonalReceiver(cc, n).decryptIndex(gidx)
    assert found == Or.decrypt_index(idx) and set(matches) <= set(found)
    mem, gmem = Or.hers_membership_scenario(q, dbc, n), sender.membershipScenario(gq)
    assert np.array_equal(gmem.export()[0], mem.data())
    # the diagonal sender refuses a column-packed database (and vice versa): no silent mixing of layouts
    with pytest.raises(im.HydiaError):
        im.DiagonalSender(cc, n).computeSimilarity(im.DiagonalReceiver(cc, n).encryptQuery(query, seed=1, nonce=1))


def test_hers_reference_dataset_full_ring(im):
    """./ImageMatching ../test/2_10.dat 4 on the GPU: expected `true`, `[0]`, scores within 1e-4 of plaintext cosine."""
    cc = im.Context()
    cc.keygen(5)
    g = np.load(os.path.join(GOLDEN, "dataset_2_10.npz"))
    n, query, db = int(g["n"]), g["query"].astype(np.float64), g["db"].astype(np.float64)
    im.HersEnroller(cc, n).serializeDB(db, seed=9)
    receiver, sender = im.HersReceiver(cc, n), im.HersSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5)
    assert len(qc) == 512
    scores = cc.decrypt(sender.computeSimilarity(qc))[0]
    assert np.abs(scores[:n] - g["cosine"]).max() < TOL and np.abs(scores[n:]).max() < TOL
    assert receiver.decryptMembership(sender.membershipScenario(qc)) is True
    assert receiver.decryptIndex(sender.indexScenario(qc)) == [0]
    cc.close()


def test_full_size_2p20_properties(im):
    """BASELINE's headline size on one GPU (2^20 vectors, 64 blocks, 32768 database ciphertexts, 142.5 GiB resident) through
    size-independent properties: (1) every one of the 2^20 decrypted scores within 1e-4 of plaintext cosine
    (src/main_accuracy.cpp:359-360); (2) index = planted matches, membership true; (3) additivity in the query ciphertext:
    similarity(qa + qb) decrypts to similarity(qa) + similarity(qb); (4) block independence (sender_diag.cpp:28-30): the score
    ciphertext of block g out of the 64-block batched pass is BIT-identical to running that block alone in a second context
    — which chains the batched full-size path to the single-block path that is bit-exact against the oracle."""
    n = 1 << 20
    cc = im.Context()
    cc.keygen(21)
    rng = np.random.default_rng(20250725)
    db = rng.integers(-99, 100, size=(n, 512), dtype=np.int8).astype(np.float64)
    planted = sorted([0, 12345, n // 2, n - 1])
    for i in planted:
        db[i] = rng.integers(1, 4, size=512)
    qa = np.ones(512)
    qb = rng.integers(-5, 6, size=512).astype(np.float64)
    norms = np.linalg.norm(db, axis=1)
    cos_a = (db @ (qa / np.linalg.norm(qa))) / norms
    cos_b = (db @ (qb / np.linalg.norm(qb))) / norms
    im.DiagonalEnroller(cc, n).serializeDB(db, seed=4)
    del db
    assert cc.db_stats()[1] == 32768
    receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
    ca, cb = receiver.encryptQuery(qa, seed=5, nonce=1), receiver.encryptQuery(qb, seed=5, nonce=2)
    sim_a = sender.computeSimilarity(ca)
    assert len(sim_a) == 64
    sa = cc.decrypt(sim_a).reshape(-1)
    assert np.abs(sa - cos_a).max() < TOL
    sb = cc.decrypt(sender.computeSimilarity(cb)).reshape(-1)
    assert np.abs(sb - cos_b).max() < TOL
    cab = cc.import_ct(ca.export(), ca.shape()[3])
    cc.eval_add(cab, cb)  # in place (EvalAddInPlace)
    sab = cc.decrypt(sender.computeSimilarity(cab)).reshape(-1)
    assert np.abs(sab - (sa + sb)).max() < TOL
    assert receiver.decryptIndex(sender.indexScenario(ca)) == planted
    assert receiver.decryptMembership(sender.membershipScenario(ca)) is True
    assert np.abs(cos_b).max() < 0.3 and receiver.decryptMembership(sender.membershipScenario(cb)) is False
    # (4) one block alone, same ciphertexts, second context with the same keys
    g = 37
    sim_a_host = sim_a.export()
    c2 = im.Context()
    c2.keygen(21)
    c2.db_alloc(16384)
    for i in range(512):
        c2.db_import_ct(i, cc.db_export_ct(g * 512 + i))
    alone = im.DiagonalSender(c2, 16384).computeSimilarity(c2.import_ct(ca.export(), ca.shape()[3])).export()
    assert np.array_equal(alone[0], sim_a_host[g])
    c2.close()
    cc.close()


def test_custom_chain_full_ring_end_to_end(im):
    """The fast N = 2^15 kernels (FP64 / integer NTT paths chosen by modulus width, 48-bit packed database, fused passes) on
    a caller-supplied prime chain with caller-supplied roots (hydia_ctx_create_custom): the reference's 2_10
    data set still answers `true`, `[0]` with scores within 1e-4."""
    moduli, roots = O.alt_prime_chain(15)
    cc = im.Context(moduli=moduli, roots=roots, n_p=4)
    assert np.array_equal(cc.moduli, moduli) and cc.db_stats is not None
    cc.keygen(5)
    g = np.load(os.path.join(GOLDEN, "dataset_2_10.npz"))
    n, query, db = int(g["n"]), g["query"].astype(np.float64), g["db"].astype(np.float64)
    im.DiagonalEnroller(cc, n).serializeDB(db, seed=9)
    receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
    qc = receiver.encryptQuery(query, seed=5)
    scores = cc.decrypt(sender.computeSimilarity(qc))[0]
    assert np.abs(scores[:n] - g["cosine"]).max() < TOL and np.abs(scores[n:]).max() < TOL
    assert receiver.decryptMembership(sender.membershipScenario(qc)) is True
    assert receiver.decryptIndex(sender.indexScenario(qc)) == [0]
    cc.close()


ENROLLER_SEED_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "hydia_roles.hpp"
// exit code 0 = every check holds.  (a) an enroller WITHOUT a caller seed enrols the same plaintext database twice: the resident
// ciphertexts differ (a fresh sampler key per serializeDB call) and both answer the query; (b) an enroller WITH a caller seed refuses
// a second enrolment (HYDIA_ERR_STATE) and leaves the first database resident.
int main() {
    using namespace hydia;
    CryptoContext cc = GenCryptoContext(11, 45, 64, 11);
    if (!cc->h || !cc->KeyGen()) return 10;
    const size_t n = 300, dim = 64;
    std::vector<std::vector<double>> db(n, std::vector<double>(dim, 1.0));
    for (size_t i = 1; i < n; i++)
        for (size_t j = 0; j < dim; j++) db[i][j] = (double)((int)((i * 31 + j * 17) % 199) - 99);
    const size_t words = 2ull * cc->info.n_q * cc->info.n;
    std::vector<uint64_t> a(words), b(words);
    DiagonalEnroller free_seed(cc, PublicKey{cc.get()}, n);
    std::vector<std::vector<double>> d1 = db, d2 = db;
    free_seed.serializeDB(d1);
    if (hydia_db_export_ct(cc->h, 0, a.data()) != 0) return 11;
    free_seed.serializeDB(d2);
    if (hydia_db_export_ct(cc->h, 0, b.data()) != 0) return 12;
    if (std::memcmp(a.data(), b.data(), words * 8) == 0) return 13;          // same (seed, nonce) reused
    size_t same = 0;
    for (size_t i = 0; i < words; i++) same += a[i] == b[i];
    if (same > words / 1000) return 14;                                       // both components re-randomised
    DiagonalReceiver receiver(cc, PublicKey{cc.get()}, PrivateKey{cc.get()}, n);
    DiagonalSender sender(cc, PublicKey{cc.get()}, n);
    auto q = receiver.encryptQuery(std::vector<double>(dim, 1.0));
    auto idx = sender.indexScenario(q);
    auto found = receiver.decryptIndex(idx);
    if (found.empty() || found[0] != 0) return 15;
    uint8_t seed[32] = {7};
    DiagonalEnroller fixed(cc, n, seed);
    std::vector<std::vector<double>> d3 = db;
    fixed.serializeDB(d3);
    if (cc->last_status != 0) return 16;
    if (hydia_db_export_ct(cc->h, 0, a.data()) != 0) return 17;
    fixed.serializeDB(d3);                                                     // refused, message on cerr
    if (cc->last_status != HYDIA_ERR_STATE) return 18;
    if (hydia_db_export_ct(cc->h, 0, b.data()) != 0 || std::memcmp(a.data(), b.data(), words * 8) != 0) return 19;
    return 0;
}
"""


def test_role_enroller_never_reuses_a_sampler_key(tmp_path):
    """Round-2 advisor finding: the C++ DiagonalEnroller drew its sampler key once per object while the database nonces restart at
    the same base on every serializeDB — two enrolments on one object encrypted under the same (seed, nonce) pairs.  Now every call
    without a caller seed redraws the key, and a caller-supplied seed enrols one database only."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "enroller_seed.cpp", tmp_path / "enroller_seed"
    src.write_text(ENROLLER_SEED_PROGRAM)
    libdir = os.path.join(root, "image_matching_amd")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"), "-o", str(exe), str(src), "-L", libdir, "-lhydia",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert "ONE database" in out.stderr
