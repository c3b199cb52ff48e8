"""CPU-only: a driver written in the reference's call shape for approach 2 — `new BaseEnroller(cc, pk, n)`, `new GroteReceiver(cc, pk,
sk, n)`, `new GroteSender(cc, pk, n)`, the timed calls through the abstract Sender / Receiver pointers (what
/root/reference/src/main.cpp:236-238, :319-327, :333-374 do; own text, not the reference's file) — compiles against
include/hydia_roles.hpp with -Wall -Werror (the mechanism of tests/test_capi_cpu.py)."""
import os
import subprocess

from conftest import ROOT

ROLES_CALL_SHAPE = r"""
#include "hydia_roles.hpp"
using namespace std;
using namespace hydia::ofhe;
using hydia::Sender; using hydia::Receiver; using hydia::GenCryptoContext; namespace OpenFHEWrapper = hydia::OpenFHEWrapper;
using hydia::BaseEnroller; using hydia::GroteReceiver; using hydia::GroteSender;

int run(size_t numVectors, vector<double> queryVector, vector<vector<double>> plaintextVectors) {
    hydia_params prm;
    if (hydia_params_for_approach(2, &prm) != 0) return -1;
    CryptoContext<DCRTPoly> cc = GenCryptoContext(OpenFHEWrapper::computeRequiredDepth(2), prm.scale_bits, hydia::VECTOR_DIM, prm.log_n);
    auto keyPair = cc->KeyGenBaseline();
    PublicKey<DCRTPoly> pk = keyPair.publicKey;
    PrivateKey<DCRTPoly> sk = keyPair.secretKey;
    BaseEnroller *enroller = new BaseEnroller(cc, pk, numVectors);
    enroller->serializeDB(plaintextVectors);
    delete enroller;
    Receiver *receiver = new GroteReceiver(cc, pk, sk, numVectors);
    Sender *sender = new GroteSender(cc, pk, numVectors);
    vector<Ciphertext<DCRTPoly>> queryCipher = receiver->encryptQuery(queryVector);
    vector<Ciphertext<DCRTPoly>> scores = sender->computeSimilarity(queryCipher);
    Ciphertext<DCRTPoly> membershipCipher = sender->membershipScenario(queryCipher);
    bool membershipResult = receiver->decryptMembership(membershipCipher);
    auto indexCipher = sender->indexScenario(queryCipher);
    vector<size_t> indexResults = receiver->decryptIndex(indexCipher);
    delete receiver;
    delete sender;
    return (membershipResult ? 1 : 0) + (int)indexResults.size() + (int)scores.size() + (int)hydia_grote_row_length((uint32_t)cc->GetBatchSize());
}
int main() { return 0; }
"""


def test_grote_roles_compile_in_the_reference_call_shape(tmp_path):
    src = tmp_path / "grote_roles.cpp"
    src.write_text(ROLES_CALL_SHAPE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
