"""The multi-query sender without a GPU: the three C entry points are declared in include/hydia.h, exported by the library and
bound in image_matching_amd.hydia; a C++ caller of DiagonalSender's *Multi methods compiles against include/hydia_roles.hpp
with -Werror."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hydia_compute_similarity_multi", "hydia_index_scenario_multi", "hydia_membership_scenario_multi")

MULTI_CALL_SHAPE = r"""
#include "hydia_roles.hpp"
#include <iostream>
using namespace std;
using namespace hydia::ofhe;
using hydia::GenCryptoContext; namespace OpenFHEWrapper = hydia::OpenFHEWrapper;
using hydia::DiagonalEnroller; using hydia::DiagonalReceiver; using hydia::DiagonalSender;

int run(size_t numVectors, vector<vector<double>> queries, vector<vector<double>> plaintextVectors) {
    CryptoContext<DCRTPoly> cc = GenCryptoContext(OpenFHEWrapper::computeRequiredDepth(5), 45);
    auto keyPair = cc->KeyGen();
    cc->EvalMultKeyGen(keyPair.secretKey);
    DiagonalEnroller enroller(cc, keyPair.publicKey, numVectors);
    enroller.serializeDB(plaintextVectors);
    DiagonalReceiver receiver(cc, keyPair.publicKey, keyPair.secretKey, numVectors);
    DiagonalSender sender(cc, keyPair.publicKey, numVectors);
    vector<vector<Ciphertext<DCRTPoly>>> queryCiphers;
    for (auto &q : queries) queryCiphers.push_back(receiver.encryptQuery(q));
    vector<vector<Ciphertext<DCRTPoly>>> sims = sender.computeSimilarityMulti(queryCiphers);
    vector<vector<Ciphertext<DCRTPoly>>> indices = sender.indexScenarioMulti(queryCiphers);
    vector<Ciphertext<DCRTPoly>> members = sender.membershipScenarioMulti(queryCiphers);
    if (sims.size() != queries.size() || indices.size() != queries.size() || members.size() != queries.size()) return 1;
    for (size_t q = 0; q < queries.size(); q++) {
        vector<size_t> idx = receiver.decryptIndex(indices[q]);
        bool member = receiver.decryptMembership(members[q]);
        cout << q << " " << idx.size() << " " << member << " " << sims[q].size() << endl;
    }
    return 0;
}
int main() { return 0; }
"""


def test_multi_entry_points_declared_exported_and_bound():
    import image_matching_amd as im
    header = open(os.path.join(ROOT, "include", "hydia.h")).read()
    L = im.load_library()
    for name in NAMES:
        assert re.search(r"int\s+%s\s*\(hydia_ctx \*ctx, const hydia_ct \*const \*queries, uint32_t n_queries, hydia_ct \*\*out\);" % name, header), name
        assert hasattr(L, name) and name in L._hydia_symbols, name
    for meth in ("computeSimilarityMulti", "indexScenarioMulti", "membershipScenarioMulti"):
        assert callable(getattr(im.DiagonalSender, meth)), meth


def test_roles_multi_methods_compile(tmp_path):
    src = tmp_path / "multi.cpp"
    src.write_text(MULTI_CALL_SHAPE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
