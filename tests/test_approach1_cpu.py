"""CPU (no GPU needed): approach 1 (the literature baseline) — the mask and rotation schedule on plain slot vectors, the restatement of
steps 1-6 through the CPU oracle at N = 2^11, the host-only key-set entry point, the symbol table and the CLI's argument handling."""
import os
import re
import subprocess

import numpy as np
import pytest

import approach1_ref as A
import oracle_lib as O
from conftest import ROOT

TOL = 1e-4  # src/main_accuracy.cpp:359-360


@pytest.mark.parametrize("slots,dim,n", [(1024, 64, 40), (1024, 64, 16), (1024, 64, 1024 + 17), (32768, 512, 1024), (32768, 512, 64 * 513 + 5)])
def test_plain_model_places_every_score(slots, dim, n):
    """steps 1, 3, 4, 5 on float slot vectors: slot j of output o is the cosine of vector o slots + j, every other slot is zero"""
    rng = np.random.default_rng(n)
    db = rng.integers(-99, 100, size=(n, dim)).astype(np.float64)
    query = rng.integers(-99, 100, size=dim).astype(np.float64)
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))
    out = A.plain_compute_similarity(db, query, slots, dim)
    vpc = slots // dim
    assert len(out) == -(-(-(-n // vpc) * vpc) // slots)
    flat = np.concatenate(out)
    assert np.abs(flat[:n] - cos).max() < 1e-12
    assert np.abs(flat[n:]).max() < 1e-12


def test_merge_schedule_counts():
    """dim 512 at 32768 slots: two mask multiplies and six rotate-and-add steps of two rotations each; dim 64 at 1024: masks at i = 1 only"""
    s = A.merge_schedule(32768, 512)
    assert [a for w, a in s if w == "mask"] == [1, 64]
    assert [A.binary_rotations(a, 32768) for w, a in s if w == "rotadd"] == [[512 * i, 32768 - i] for i in (1, 2, 4, 8, 16, 32)]
    assert [a for w, a in A.merge_schedule(1024, 64) if w == "mask"] == [1, 16]
    assert [a for w, a in A.merge_schedule(1024, 16) if w == "mask"] == [1, 16, 64]
    need = set(A.approach1_rotations(32768))
    for i in range(512):
        assert set(A.binary_rotations(-((64 * i) % 32768), 32768)) <= need


@pytest.fixture(scope="module")
def small():
    P = O.Params(log_n=11, depth=13, dim=64)
    K = O.Keys(P, 7, rotations=A.approach1_rotations(P.slots))
    return P, K, O.Oracle(P, K)


@pytest.mark.parametrize("planted", [True, False])
def test_restatement_through_the_oracle(small, planted):
    """N = 2^11, dim 64, n = 40 (3 ciphertexts, ragged): scores within 1e-4 of cosine, index and membership right"""
    P, K, Or = small
    n = 40
    rng = np.random.default_rng(3)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    if planted:
        db[23] = rng.integers(1, 4, size=P.dim)
    query = np.ones(P.dim)
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))
    dbcts = A.oracle_enroll(P, Or, db, 99)
    assert len(dbcts) == 3
    q = Or.encrypt_query(query, 5, 1)
    sim = A.oracle_compute_similarity(P, Or, q, dbcts)
    assert len(sim) == 1 and sim[0].nl == P.nQ - 3
    scores = Or.decrypt(sim[0])
    err = max(np.abs(scores[:n] - cos).max(), np.abs(scores[n:]).max())
    print("approach 1 restatement, N = 2^11: max score error %.3e" % err)
    assert err < TOL
    index = [Or.chebyshev_compare(c) for c in sim]
    assert A.decrypt_index(P, Or, index) == ([23] if planted else [])
    assert Or.decrypt_membership(A.oracle_membership_from_index(P, Or, index)) is planted


def test_vectorised_mult_plain_equals_the_integer_one(small):
    from test_gpu_approach1_ring import oracle_mult_plain
    P, K, Or = small
    rng = np.random.default_rng(8)
    ct = Or.encrypt(rng.uniform(-1, 1, P.slots), 4, 2)
    mask = A.merge_mask(P.slots, P.dim, 1)
    assert np.array_equal(A.oracle_mult_plain(P, Or, ct, mask).data(), oracle_mult_plain(P, Or, ct, mask).data())


def test_base_rotations_entry_point():
    import image_matching_amd as im
    for slots in (1024, 16384, 32768):
        assert im.base_rotations(slots) == A.approach1_rotations(slots)
    assert len(im.base_rotations(32768)) == 29
    with pytest.raises(im.HydiaError):
        im.base_rotations(1000)


def test_symbols_declared_exported_and_mirrored():
    import image_matching_amd as im
    L = im.load_library()
    hdr = open(os.path.join(ROOT, "include", "hydia.h")).read()
    for name in ("hydia_base_db_num_cts", "hydia_base_db_enroll", "hydia_base_compute_similarity", "hydia_base_index_scenario",
                 "hydia_base_membership_scenario", "hydia_merge_ciphers", "hydia_base_rotations"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L._hydia_symbols and getattr(L, name)
    for cls in ("BaseEnroller", "BaseReceiver", "BaseSender"):
        assert hasattr(im, cls)
    assert issubclass(im.BaseSender, im.HersSender) and issubclass(im.BaseReceiver, im.HersReceiver)


ROLES_APPROACH1 = r"""
#include "hydia_roles.hpp"
using namespace hydia::ofhe;  // the reference's template spelling of the handle types
using std::vector;
using hydia::Sender; using hydia::Receiver; using hydia::HersSender; namespace OpenFHEWrapper = hydia::OpenFHEWrapper;
using hydia::BaseEnroller; using hydia::BaseReceiver; using hydia::BaseSender; using hydia::VECTOR_DIM;
int run(CryptoContext<DCRTPoly> cc, vector<vector<double>> &db, vector<double> &query, size_t numVectors) {
    auto keyPair = cc->KeyGenBaseline();
    PublicKey<DCRTPoly> pk = keyPair.publicKey;
    PrivateKey<DCRTPoly> sk = keyPair.secretKey;
    BaseEnroller *enroller = new BaseEnroller(cc, pk, numVectors);
    enroller->serializeDB(db);
    delete enroller;
    Receiver *receiver = new BaseReceiver(cc, pk, sk, numVectors);
    Sender *sender = new BaseSender(cc, pk, numVectors);
    HersSender *as_hers = static_cast<BaseSender *>(sender);
    (void)as_hers;
    vector<Ciphertext<DCRTPoly>> queryCipher = receiver->encryptQuery(query);
    vector<Ciphertext<DCRTPoly>> scores = sender->computeSimilarity(queryCipher);
    vector<Ciphertext<DCRTPoly>> merged = OpenFHEWrapper::mergeCiphers(cc, scores, VECTOR_DIM);
    bool member = receiver->decryptMembership(*new Ciphertext<DCRTPoly>(sender->membershipScenario(queryCipher)));
    auto indexCipher = sender->indexScenario(queryCipher);
    size_t hits = receiver->decryptIndex(indexCipher).size();
    delete receiver;
    delete sender;
    return (int)hits + (member ? 1 : 0) + (int)merged.size();
}
int main() { return 0; }
"""


def test_cli_takes_approach_1_and_roles_header_compiles(tmp_path):
    """`./ImageMatching <file> 1` passes the argument check (it prints the baseline's banner and fails, if at all, on the missing GPU);
    2 keeps the old refusal; the header with the Base* classes compiles alone"""
    exe = os.path.join(ROOT, "image_matching_amd", "ImageMatching")
    assert os.path.exists(exe), "CLI not built"
    (tmp_path / "latency.csv").write_text("")
    dat = tmp_path / "tiny.dat"
    dat.write_text("1\n" + " ".join(["1"] * 512) + "\n" + " ".join(["2"] * 512) + "\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")  # argument handling only: never start a query here
    out = subprocess.run([exe, str(dat), "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120, env=env)
    assert "Experimental approach: Literature baseline" in out.stdout, (out.stdout, out.stderr)
    assert "approach must be" not in out.stderr and "only approach 5" not in out.stderr
    assert out.returncode == 2, (out.returncode, out.stderr)  # context creation failed: no HIP device
    assert (tmp_path / "latency.csv").read_text().startswith("Baseline,")
    out = subprocess.run([exe, str(dat), "2"], cwd=tmp_path, capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode != 0 and "only approach 5" in out.stderr
    src = tmp_path / "roles_a1.cpp"
    src.write_text(ROLES_APPROACH1)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
