"""CPU-only checks of seeded keys and seeded secret-key queries (include/hydia.h, hydia_keygen_seeded / hydia_encrypt_query_seeded):
the restatement tests/seeded_ref.py is itself sound on the CPU oracle (a restated query decrypts to the probe, restated keys rotate
and multiply), the C++ role header compiles with the new methods, and the byte counts the README quotes follow from the parameters.
Ring: N = 2^11, 64-dim vectors."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import seeded_ref as SR
from conftest import ROOT
from db_rekey_ref import as_oracle_cts

TOL = 1e-4
SEED, A_SEED = 7, 1007


@pytest.fixture(scope="module")
def small():
    P = O.Params(log_n=11, depth=11, dim=64)
    K = O.Keys(P, SEED, rotations=[1, P.dim - 1])
    yield P, K
    P.close()


def probe(P, seed):
    return np.random.default_rng(seed).integers(-99, 100, size=P.dim).astype(np.float64)


def test_restated_query_decrypts_to_the_probe(small):
    P, K = small
    Or = O.Oracle(P, K)
    for query, nonce in ((probe(P, 1), 1), (np.zeros(P.dim), 2), (probe(P, 2), (1 << 40) - 1)):
        c0, a = SR.seeded_query(P, K, query, SEED, A_SEED, nonce)
        assert np.array_equal(a[3], O.sample_uniform(A_SEED, (9 << 56) | (nonce << 16) | 3, int(P.moduli[3]), P.N))
        ct = as_oracle_cts(P, Or, [np.stack([c0, a])])[0]
        assert np.abs(Or.decrypt(ct) - SR.tiled_probe(P, query)).max() < TOL
    # the public seed alone changes c1 and c0, the nonce too
    c0, a = SR.seeded_query(P, K, probe(P, 1), SEED, A_SEED, 1)
    c0b, ab = SR.seeded_query(P, K, probe(P, 1), SEED, A_SEED + 1, 1)
    c0c, ac = SR.seeded_query(P, K, probe(P, 1), SEED, A_SEED, 2)
    assert not np.array_equal(a, ab) and not np.array_equal(c0, c0b) and not np.array_equal(a, ac) and not np.array_equal(c0, c0c)


def test_restatement_arithmetic_against_python_integers(small):
    """seeded_ref.mulmod / rebase (uint64 throughout) on random and on saturated residues of the widest and a narrow modulus"""
    P, _ = small
    rng = np.random.default_rng(5)
    for q in (int(P.moduli[0]), int(P.moduli[1]), int(P.moduli[P.nT - 1])):
        a, b, c, d = [rng.integers(0, q, size=64, dtype=np.uint64) for _ in range(4)]
        for arr in (a, b, c, d):
            arr[:4] = (0, 1, q - 1, q - 2)
        b[:4] = (q - 1, q - 1, q - 1, 0)
        assert [int(v) for v in SR.mulmod(a, b, q)] == [int(x) * int(y) % q for x, y in zip(a, b)]
        want = [(int(w) + (int(x) - int(y)) * int(z)) % q for w, x, y, z in zip(a, b, c, d)]
        assert [int(v) for v in SR.rebase(a, b, c, d, q)] == want


def test_installed_seeded_keys_are_keys(small):
    """the restated key set, written over the oracle's own: the secret stays, every a half is the public seed's expansion, and the
    oracle rotates and multiplies under it"""
    P, _ = small
    K = O.Keys(P, SEED, rotations=[1, P.dim - 1])  # a key set of this test's own: install overwrites it
    plain = O.Keys(P, SEED, rotations=[1])
    keys, pk = SR.install(K, P, SEED, A_SEED)
    assert np.array_equal(K.s_ntt(), plain.s_ntt())
    assert not np.array_equal(K.relin()[:, 1], plain.relin()[:, 1]) and not np.array_equal(K.relin()[:, 0], plain.relin()[:, 0])
    assert np.array_equal(K.rot_key(1), keys[1]) and np.array_equal(K.pk(), pk)
    for d in range(P.dnum):
        assert np.array_equal(keys[1][d, 1, 5], O.sample_uniform(A_SEED, SR.stream(SR.DOM_EVK_A, 1, d, 5), int(P.moduli[5]), P.N))
    Or = O.Oracle(P, K)
    query = probe(P, 3)
    slots = SR.tiled_probe(P, query)
    c0, a = SR.seeded_query(P, K, query, SEED, A_SEED, 1)
    ct = as_oracle_cts(P, Or, [np.stack([c0, a])])[0]
    for r in (1, P.dim - 1):
        assert np.abs(Or.decrypt(Or.rotate(ct, r)) - np.roll(slots, -r)).max() < TOL
    assert np.abs(Or.decrypt(Or.mult(ct, ct)) - slots * slots).max() < TOL
    # and a public-key encryption under the installed public key opens under the unchanged secret
    assert np.abs(Or.decrypt(Or.encrypt(slots, 11, 1)) - slots).max() < TOL


# A driver written against the seeded methods of include/hydia_roles.hpp: the receiver generates a seeded key set and ships half keys and
# half queries, the sender (a context of its own, no secret) imports, expands and serves them
ROLES_SEEDED = r"""
#include "hydia_roles.hpp"
using namespace std;
using hydia::CryptoContext; using hydia::Ciphertext; using hydia::GenCryptoContext;
using hydia::DiagonalReceiver; using hydia::DiagonalSender; using hydia::DiagonalEnroller;
using hydia::SeededQuery; using hydia::SeededKeys; using hydia::DeviceRows;

int run(size_t numVectors, vector<double> queryVector, vector<vector<double>> probes, vector<vector<double>> plaintextVectors, const void *devRows) {
    CryptoContext rc = GenCryptoContext(11, 45), sc = GenCryptoContext(11, 45);
    auto keyPair = rc->KeyGenSeeded();
    if (!keyPair) return -1;
    DiagonalReceiver receiver(rc, keyPair.publicKey, keyPair.secretKey, numVectors);
    DiagonalSender sender(sc, numVectors);
    SeededKeys keys = receiver.exportKeysSeeded();
    if (!keys || !sender.importKeysSeeded(keys)) return -2;
    DiagonalEnroller enroller(sc, numVectors);
    enroller.serializeDB(plaintextVectors);
    SeededQuery one = receiver.encryptQuerySeeded(queryVector);
    SeededQuery many = receiver.encryptQueriesSeeded(probes);
    SeededQuery dev = receiver.encryptQueriesSeeded(DeviceRows(devRows, HYDIA_F32, probes.size(), 512));
    size_t wire = one.nbytes() + many.nbytes() + dev.nbytes() + (one ? 1 : 0);
    vector<Ciphertext> queryCipher = sender.expandQuery(one);
    vector<vector<Ciphertext>> queryCiphers = sender.expandQueries(many);
    Ciphertext membershipCipher = sender.membershipScenario(queryCipher);
    auto indexCiphers = sender.indexScenarioMulti(queryCiphers);
    return (int)wire + (int)indexCiphers.size() + (membershipCipher ? 1 : 0) + (int)many.nonce0 + (int)keys.evalKeys.size() + keys.aSeed[0];
}
int main() { return 0; }
"""


def test_roles_header_compiles_with_the_seeded_methods(tmp_path):
    src = tmp_path / "roles_seeded.cpp"
    src.write_text(ROLES_SEEDED)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_readme_byte_counts_follow_from_the_parameters():
    import image_matching_amd as im
    if not os.path.exists(im.lib_path()):
        from image_matching_amd.hydia import build_library
        build_library()
    info, _, _ = im.describe_params(im.default_params())
    N, nQ, nT, dnum, dim, slots = info["n"], info["n_q"], info["n_q"] + info["n_p"], info["dnum"], info["vector_dim"], info["slots"]
    key_words, half_words = dnum * 2 * nT * N, dnum * nT * N
    n_keys, r = 1 + (dim - 1), dim  # relinearisation, rotations 1 .. dim-1, then dim, 2 dim, .. below the slot count
    while r < slots:
        n_keys, r = n_keys + 1, r * 2
    assert (key_words * 8, half_words * 8, n_keys) == (25165824, 12582912, 517)
    query, half_query = 2 * nQ * N * 8, nQ * N * 8
    assert (query, half_query) == (6291456, 3145728)
    text = re.sub(r"(?<=\d) (?=\d{3}\b)", "", open(os.path.join(ROOT, "README.md")).read())
    for figure in (key_words * 8, half_words * 8, query, half_query, n_keys):
        assert re.search(r"\b%d\b" % figure, text), figure
    for gb in (n_keys * key_words * 8, n_keys * half_words * 8):  # quoted in GB with one decimal
        assert "%.1f GB" % (gb / 1e9) in text, gb
    header = open(os.path.join(ROOT, "include", "hydia.h")).read()
    header = re.sub(r"(?<=\d) (?=\d{3}\b)", "", header)
    for figure in (key_words * 8, half_words * 8, query, half_query):
        assert str(figure) in header
