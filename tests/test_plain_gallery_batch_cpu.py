"""CPU-only checks of a BATCH of encrypted queries against a plain gallery (hydia_*_gallery_multi, DiagonalSender.*GalleryMulti): the
new symbols, the Python refusals that never reach the library, the roles header in the reference's call shape, the batch slot map of
loop B in integers (kind 7, and kind 8 giant-major), and an integer model of k_hydia_plain_mq's per-query sums against the single
form's (tests/test_plain_gallery_model_cpu.py)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT
from test_plain_gallery_model_cpu import M64, M128, chains, chunk_of, halves24_sum, sums128_sum  # noqa: F401 (chains: a fixture)

NEW_SYMBOLS = ("hydia_compute_similarity_gallery_multi", "hydia_index_scenario_gallery_multi", "hydia_membership_scenario_gallery_multi",
               "hydia_set_gallery_batch_width")
ROLE_METHODS = ("computeSimilarityGalleryMulti", "indexScenarioGalleryMulti", "membershipScenarioGalleryMulti")


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
    assert hasattr(im.Context, "set_gallery_batch_width")
    roles = open(os.path.join(ROOT, "include", "hydia_roles.hpp")).read()
    for n in ROLE_METHODS:
        assert " %s(std::vector<std::vector<Ciphertext>> &queryCiphers)" % n in roles, n


def test_role_methods_refuse_what_is_not_a_ciphertext_without_calling_the_library():
    """*GalleryMulti raise ERR_ARG for a Plaintext (or anything that is no Ciphertext) and ERR_STATE on what is no single-GPU context,
    before they touch the context (there is none here)"""
    import image_matching_amd as im
    pt = im.Plaintext.__new__(im.Plaintext)
    ct = im.Ciphertext.__new__(im.Ciphertext)
    sender = im.DiagonalSender(None, 1)
    for name in ROLE_METHODS:
        for batch in ([pt], [ct, pt], [pt, ct, ct], [None], [ct, 3.0]):
            with pytest.raises(im.HydiaError) as e:
                getattr(sender, name)(batch)
            assert e.value.code == -1 and "Ciphertext" in str(e.value), (name, batch)
        with pytest.raises(im.HydiaError) as e:  # the context is no im.Context: a sharded one
            getattr(sender, name)([ct, ct])
        assert e.value.code == -2 and "sharded" in str(e.value), name


# ---- the batch slot map.  Kind 8: loop B's "blocks" gi are (gallery block, giant) pairs, block-major: gi = block NG + giant (plaintext
# t = (block NG + giant) B + baby).  giant_step_sum takes [NG][X0] giant-major accumulators and returns [X0], and the batch's tails
# take X0 = Q G query-major, so the slot of (giant, query, block) must be  giant (Q G) + query G + block;  on kind 7 (ng = 0) the tails
# take  query G + block.
def mq_slot(q, gi, G, ng, nblk, Qt):
    """kernels.hip mq_slot in Python integers (G: loop B's block count, NG x gallery blocks when ng > 0)"""
    return ((gi % ng) * Qt + q) * nblk + gi // ng if ng > 0 else q * G + gi


def test_the_model_is_the_slot_map_of_the_kernels_and_the_batch_writes_through_it():
    text = re.sub(r"\s+", "", open(os.path.join(ROOT, "image_matching_amd", "csrc", "kernels.hip")).read())
    assert "returnng>0?((size_t)(gi%ng)*Qt+q)*nblk+gi/ng:(size_t)q*G+gi;" in text
    body = text[text.index("voidk_hydia_plain_mq("):text.index("voidk_hydia_plain_mq_sk(")]
    assert "u64*o=acc+(mq_slot(q0+q,g,G,ng,nblk,Qt)*2*nl+j)*N+c;" in body
    assert "loop_b_split<FormCtPlainMq,KS,QW>(mod,N,rot,rqs,db,acc,dim,nl,L,G,ng,nblk,q0,Qt);" in text


@pytest.mark.parametrize("Q", [1, 2, 3, 5])
@pytest.mark.parametrize("G", [1, 3, 10])
@pytest.mark.parametrize("NG", [1, 8])
def test_batch_slot_map_is_what_the_giant_steps_and_the_tails_expect(Q, G, NG):
    slots = set()  # kind 7: ng = 0, loop B over G blocks
    for q in range(Q):
        for block in range(G):
            s = mq_slot(q, block, G, 0, 0, Q)
            assert s == q * G + block
            slots.add(s)
    assert slots == set(range(Q * G))
    slots = set()  # kind 8: ng = NG, loop B over G NG (block, giant) pairs, nblk = G (the launcher: G_loop / ng)
    for q in range(Q):
        for block in range(G):
            for giant in range(NG):
                s = mq_slot(q, block * NG + giant, G * NG, NG, (G * NG) // NG, Q)
                assert s == giant * (Q * G) + q * G + block, (giant, q, block)
                slots.add(s)
    assert slots == set(range(Q * G * NG))


# ---- the sums.  k_hydia_plain_mq as it runs, in integers: per diagonal ONE gallery operand m_i (cut once), and per query its two
# operands (c0_i, c1_i), each multiplied into that query's own sum — wrapping 64-bit sums of 24-bit half products, or a wrapping 128-bit
# sum folded every chunk diagonals (all queries' sums at the same diagonals).  Every per-query sum is compared with the single form's
# (halves24_sum / sums128_sum of tests/test_plain_gallery_model_cpu.py) and with the exact sum modulo q.
def batch_sums(queries, gallery, q, chunk, halves):
    """queries: [QW][2][dim] residues, gallery: [dim] -> [QW][2] residues as the batch kernel forms them"""
    QW, dim = len(queries), len(gallery)
    if halves:
        s = [[[0, 0, 0] for _ in range(2)] for _ in range(QW)]  # ll, mid, hh
        for i in range(dim):
            bl, bh = gallery[i] & 0xFFFFFF, gallery[i] >> 24  # the cut, once per diagonal
            for k in range(QW):
                for p in range(2):
                    x = queries[k][p][i]
                    al, ah = x & 0xFFFFFF, x >> 24
                    t = s[k][p]
                    t[0] = (t[0] + al * bl) & M64
                    t[1] = (t[1] + al * bh) & M64
                    t[1] = (t[1] + ah * bl) & M64
                    t[2] = (t[2] + ah * bh) & M64
        return [[(t[0] + (t[1] << 24) + (t[2] << 48)) % q for t in sk] for sk in s]
    s = [[0, 0] for _ in range(QW)]
    for i in range(dim):
        if i and i % chunk == 0:
            s = [[v % q for v in sk] for sk in s]
        for k in range(QW):
            for p in range(2):
                s[k][p] = (s[k][p] + queries[k][p][i] * gallery[i]) & M128
    return [[v % q for v in sk] for sk in s]


@pytest.mark.parametrize("QW", [1, 2, 4])
def test_batch_sums_equal_the_single_forms_sums(chains, QW):  # noqa: F811
    rng = random.Random(31 + QW)
    for name in ("default11", "evaluator11", "transform11"):
        for q in {x.bit_length(): x for x in chains[name]}.values():  # one limb per width of the chain
            k = q.bit_length()
            for dim in (512, 1024) if k >= 59 else (64, 4096):
                ch = chunk_of(q, dim)
                if k >= 59:
                    assert ch < dim  # 59/60-bit limbs: the sums cross a fold boundary (every 128 / 32 diagonals)
                sat = [q - 1] * dim
                rnd = lambda: [rng.randrange(q) for _ in range(dim)]  # noqa: E731
                for gallery in (sat, rnd()):
                    # every query saturated; then one query that is not, in every position of the pass
                    sets = [[[sat, sat] for _ in range(QW)]] + [[[sat, sat] if j != pos else [rnd(), rnd()] for j in range(QW)] for pos in range(QW)]
                    for queries in sets:
                        forms = [False] if k > 48 else [False, True]
                        for halves in forms:
                            got = batch_sums(queries, gallery, q, ch, halves)
                            for kq in range(QW):
                                for p in range(2):
                                    a = queries[kq][p]
                                    single = halves24_sum(a, gallery, q) if halves else sums128_sum(a, gallery, q, ch)
                                    assert got[kq][p] == single == sum(x * y for x, y in zip(a, gallery)) % q, (name, q, dim, kq, p, halves)


def test_the_bounds_do_not_depend_on_the_queries_beside_a_sum():
    """a sum of the batch takes ONE product of two canonical residues per diagonal, whatever QW: FormPlain's bounds as they stand"""
    h = (1 << 24) - 1
    assert 4096 * 2 * h * h < 1 << 61  # Halves24 mid at the launcher's limit of diagonals
    q60 = (1 << 60) - 1
    assert (q60 - 1) + 32 * (q60 - 1) ** 2 < 1 << 126  # Sums128: a folded residue plus one chunk of saturated products


GALLERY_DRIVER = r"""
#include "hydia_roles.hpp"
using namespace std;
using namespace hydia::ofhe;
using hydia::Receiver; using hydia::GenCryptoContext; namespace OpenFHEWrapper = hydia::OpenFHEWrapper;
using hydia::PlainEnroller; using hydia::DiagonalReceiver; using hydia::DiagonalSender;

int run(size_t numVectors, vector<vector<double>> probes, vector<vector<double>> database) {
    CryptoContext<DCRTPoly> cc = GenCryptoContext(OpenFHEWrapper::computeRequiredDepth(5), 45);
    auto keyPair = cc->KeyGen();
    PublicKey<DCRTPoly> pk = keyPair.publicKey;
    PrivateKey<DCRTPoly> sk = keyPair.secretKey;
    cc->EvalMultKeyGen(sk);
    cc->EvalSumKeyGen(sk);
    PlainEnroller enroller(cc, numVectors);
    enroller.serializeDB(database);
    Receiver *receiver = new DiagonalReceiver(cc, pk, sk, numVectors);
    DiagonalSender *sender = new DiagonalSender(cc, pk, numVectors);
    vector<vector<Ciphertext<DCRTPoly>>> queryCiphers;
    for (auto &probe : probes) queryCiphers.push_back(receiver->encryptQuery(probe));  // many clients, one public key
    vector<vector<Ciphertext<DCRTPoly>>> similarityCiphers = sender->computeSimilarityGalleryMulti(queryCiphers);
    vector<Ciphertext<DCRTPoly>> membershipCiphers = sender->membershipScenarioGalleryMulti(queryCiphers);
    vector<vector<Ciphertext<DCRTPoly>>> indexCiphers = sender->indexScenarioGalleryMulti(queryCiphers);
    int found = 0;
    for (size_t q = 0; q < indexCiphers.size(); q++) {
        found += receiver->decryptMembership(membershipCiphers[q]) ? 1 : 0;
        found += (int)receiver->decryptIndex(indexCiphers[q]).size();
    }
    // the single-query methods are still there beside the batch
    auto one = sender->indexScenario(queryCiphers[0]);
    delete receiver;
    delete sender;
    return found + (int)similarityCiphers.size() + (int)one.size();
}
int main() { return 0; }
"""


def test_gallery_driver_compiles_with_werror(tmp_path):
    src = tmp_path / "plain_gallery_batch_driver.cpp"
    src.write_text(GALLERY_DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
