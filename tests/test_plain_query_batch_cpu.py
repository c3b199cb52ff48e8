"""CPU-only checks of a BATCH of plain queries (hydia_*_pq_multi, DiagonalSender.*PlainMulti): the new symbols, the Python refusals
that never reach the library, the roles header in the reference's call shape, and the batch slot map of loop B in integers."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

NEW_SYMBOLS = ("hydia_compute_similarity_pq_multi", "hydia_index_scenario_pq_multi", "hydia_membership_scenario_pq_multi",
               "hydia_set_pq_batch_width")
ROLE_METHODS = ("computeSimilarityPlainMulti", "indexScenarioPlainMulti", "membershipScenarioPlainMulti", "encodeQueries")


def test_new_symbols_are_declared_exported_and_bound():
    import image_matching_amd as im
    text = open(os.path.join(ROOT, "include", "hydia.h")).read()
    raw = ctypes.CDLL(im.lib_path())
    L = im.load_library()
    for n in NEW_SYMBOLS:
        assert "int %s(" % n in text, n
        assert hasattr(raw, n), n
        assert n in L._hydia_symbols, n
    for n in ROLE_METHODS:
        assert hasattr(im.DiagonalSender, n), n
    assert hasattr(im.Context, "set_pq_batch_width")


def test_role_methods_refuse_what_is_not_a_plaintext_without_calling_the_library():
    """*PlainMulti raise ERR_ARG for a Ciphertext (or anything that is no Plaintext) and ERR_STATE on what is no single-GPU context,
    before they touch the context (there is none here); the *Multi methods keep refusing a Plaintext"""
    import image_matching_amd as im
    pt = im.Plaintext.__new__(im.Plaintext)
    ct = im.Ciphertext.__new__(im.Ciphertext)
    sender = im.DiagonalSender(None, 1)
    for name in ROLE_METHODS[:3]:
        for batch in ([ct], [pt, ct], [ct, pt, pt], [None]):
            with pytest.raises(im.HydiaError) as e:
                getattr(sender, name)(batch)
            assert e.value.code == -1 and "Plaintext" in str(e.value), (name, batch)
        with pytest.raises(im.HydiaError) as e:  # the context is no im.Context: what encodeQuery answers on a sharded one
            getattr(sender, name)([pt, pt])
        assert e.value.code == -2 and "sharded" in str(e.value), name
    with pytest.raises(im.HydiaError) as e:
        sender.encodeQueries([[1.0, 2.0]])
    assert e.value.code == -2
    for call in (lambda: sender.computeSimilarityMulti([pt, pt]), lambda: sender.indexScenarioMulti([pt]), lambda: sender.membershipScenarioMulti([pt])):
        with pytest.raises(im.HydiaError) as e:
            call()
        assert e.value.code == -1 and "plain query" in str(e.value)


# ---- the batch slot map.  Loop B's "blocks" gi of a BSGS database are (database block, giant) pairs, block-major: gi = block NG + giant
# (ciphertext t = (block NG + giant) B + baby, evaluator.cpp).  giant_step_sum takes [NG][X0] giant-major accumulators and returns [X0],
# and the batch's tails take X0 = Q G query-major, so the slot of (giant, query, block) must be  giant (Q G) + query G + block;  on a
# hoisted database (ng = 0) the tails take  query G + block.
def expected_slot(giant, query, block, Q, G, NG):
    return giant * (Q * G) + query * G + block


def mq_slot(q, gi, G, ng, nblk, Qt):
    """kernels.hip mq_slot in Python integers (G: loop B's block count, NG x database blocks when ng > 0)"""
    return ((gi % ng) * Qt + q) * nblk + gi // ng if ng > 0 else q * G + gi


def test_the_model_is_the_kernels_slot_map():
    """the kernel's expression, compared without its spacing (the GPU tests are what hold the stores to the map)"""
    text = re.sub(r"\s+", "", open(os.path.join(ROOT, "image_matching_amd", "csrc", "kernels.hip")).read())
    assert "returnng>0?((size_t)(gi%ng)*Qt+q)*nblk+gi/ng:(size_t)q*G+gi;" in text


@pytest.mark.parametrize("Q", [1, 2, 3])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("NG", [1, 8])
def test_batch_slot_map_is_what_the_giant_steps_and_the_tails_expect(Q, G, NG):
    # hoisted: ng = 0, loop B over G blocks
    slots = set()
    for q in range(Q):
        for block in range(G):
            s = mq_slot(q, block, G, 0, 0, Q)
            assert s == expected_slot(0, q, block, Q, G, 1)
            slots.add(s)
    assert slots == set(range(Q * G))
    # BSGS: ng = NG, loop B over G NG (block, giant) pairs, nblk = G (the launcher: G_loop / ng)
    slots = set()
    for q in range(Q):
        for block in range(G):
            for giant in range(NG):
                s = mq_slot(q, block * NG + giant, G * NG, NG, (G * NG) // NG, Q)
                assert s == expected_slot(giant, q, block, Q, G, NG), (giant, q, block)
                slots.add(s)
    assert slots == set(range(Q * G * NG))


BATCH_DRIVER = r"""
#include "hydia_roles.hpp"
using namespace std;
using namespace hydia::ofhe;
using hydia::Receiver; using hydia::GenCryptoContext; namespace OpenFHEWrapper = hydia::OpenFHEWrapper;
using hydia::DiagonalEnroller; using hydia::DiagonalReceiver; using hydia::DiagonalSender; using hydia::Plaintext;

int run(size_t numVectors, vector<vector<double>> probes, vector<vector<double>> database) {
    CryptoContext<DCRTPoly> cc = GenCryptoContext(OpenFHEWrapper::computeRequiredDepth(5), 45);
    auto keyPair = cc->KeyGen();
    PublicKey<DCRTPoly> pk = keyPair.publicKey;
    PrivateKey<DCRTPoly> sk = keyPair.secretKey;
    cc->EvalMultKeyGen(sk);
    cc->EvalSumKeyGen(sk);
    DiagonalEnroller enroller(cc, pk, numVectors);
    enroller.serializeDB(database);
    Receiver *receiver = new DiagonalReceiver(cc, pk, sk, numVectors);
    DiagonalSender *sender = new DiagonalSender(cc, pk, numVectors);
    vector<Plaintext> batch;
    for (auto &probe : probes) batch.push_back(sender->encodeQuery(probe));  // the sender knows the probes: no key, no seed
    vector<vector<Ciphertext<DCRTPoly>>> similarityCiphers = sender->computeSimilarityPlainMulti(batch);
    vector<Ciphertext<DCRTPoly>> membershipCiphers = sender->membershipScenarioPlainMulti(batch);
    vector<vector<Ciphertext<DCRTPoly>>> indexCiphers = sender->indexScenarioPlainMulti(batch);
    int found = 0;
    for (size_t q = 0; q < indexCiphers.size(); q++) {
        found += receiver->decryptMembership(membershipCiphers[q]) ? 1 : 0;
        found += (int)receiver->decryptIndex(indexCiphers[q]).size();
    }
    // the single-query overloads are still there beside the batch
    auto one = sender->indexScenario(batch[0]);
    delete receiver;
    delete sender;
    return found + (int)similarityCiphers.size() + (int)one.size();
}
int main() { return 0; }
"""


def test_batch_driver_compiles_with_werror(tmp_path):
    src = tmp_path / "plain_query_batch_driver.cpp"
    src.write_text(BATCH_DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
