"""CPU-only checks behind the candidate-list entries (include/hydia.h "candidate lists and matches"; kernels in
image_matching_amd/csrc/select_kernels.hip, GPU cases in tests/test_gpu_candidates.py).

  model      tests/candidates_ref.py's select and topk against a naive Python sort with an explicit comparator, on every crafted content
             the GPU file uses, at sizes around a wave and a tile.
  wrong forms  in the tradition of tests/test_client_edges_cpu.py: for each plausible slip of a kernel (> for >=, zeros not
             canonicalised, negative keys not reversed, NaN ranked high, ties taken from the end, the tie quota off by one, a tile's last
             element dropped) a crafted input of that list on which the slip changes the answer — so the GPU cases can tell them apart.
             The restated key (candidates_ref.key64) itself orders like the model.
  boundary   the library exports and the Python layer binds the seven new entries; a driver in the reference's call shape that uses the
             four OpenFHEWrapper functions of include/openFHE_wrapper.h the drop-in header lacked, and the new role methods, compiles
             against include/hydia_roles.hpp under -Wall -Werror."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import candidates_ref as CR
from conftest import ROOT

SIZES = [1, 63, 64, 65, CR.TILE - 1, CR.TILE, CR.TILE + 1]
NEW_ENTRIES = ["hydia_decrypt_device", "hydia_slots_select_device", "hydia_slots_topk_device", "hydia_decrypt_matches", "hydia_decrypt_topk",
               "hydia_decrypt_matches_multi", "hydia_decrypt_topk_multi"]


def naive_topk(v, k):
    """the rule of include/hydia.h spelled as a comparator: NaN after every number, value descending with the zeros equal, then index"""
    def cmp(a, b):
        x, y = v[a], v[b]
        nx, ny = math.isnan(x), math.isnan(y)
        if nx != ny:
            return 1 if nx else -1
        if not nx and x != y:  # (-0.0 != 0.0 is False: they tie)
            return -1 if x > y else 1
        return a - b
    order = sorted(range(len(v)), key=functools.cmp_to_key(cmp))[:k]
    return np.array(order, dtype=np.int64)


def all_contents():
    rng = np.random.default_rng(20261021)
    for n in SIZES:
        for name, v in CR.contents(n, rng).items():
            yield n, name, v


def test_model_against_a_naive_sort():
    for n, name, v in all_contents():
        lst = v.tolist()
        for k in sorted({1, 2, max(1, n - 1), n, n + 5}):
            idx, val = CR.topk(v, k)
            assert np.array_equal(idx, naive_topk(lst, k)), (name, n, k)
            assert np.array_equal(CR.bits(val), CR.bits(v[idx]))
        present = v[n // 2]
        for t in ([present, np.nextafter(present, np.inf)] if not np.isnan(present) else [0.0]):
            want = np.array([i for i, x in enumerate(lst) if x >= t], dtype=np.int64)
            idx, val, total = CR.select(v, t)
            assert np.array_equal(idx, want) and total == want.size and np.array_equal(CR.bits(val), CR.bits(v[want])), (name, n, t)
            idx, val, total = CR.select(v, t, 3)
            assert np.array_equal(idx, want[:3]) and total == want.size


def test_restated_key_orders_like_the_model():
    """sorting by (key descending, index) is the model's order: the radix select's key is order-preserving with the zeros merged and
    NaN lowest"""
    for n, name, v in all_contents():
        key = CR.key64(v)
        by_key = np.lexsort((np.arange(n), ~key))
        assert np.array_equal(by_key, CR.topk(v, n)[0]), (name, n)
    assert CR.key64(np.array([-np.inf]))[0] > CR.key64(np.array([np.nan]))[0] == 0
    assert CR.key64(np.array([0.0]))[0] == CR.key64(np.array([-0.0]))[0] == 1 << 63


def differs_topk(form):
    hits = []
    for n, name, v in all_contents():
        g = CR.top_group(v)
        for k in sorted({1, 2, max(1, g - 1), g, g + 1, max(1, n - 1), n} & set(range(1, n + 1))):
            want = CR.topk(v, k)[0]
            got = CR.wrong_topk(form, v, k)[0]
            if got.size != want.size or not np.array_equal(got, want):
                hits.append((name, n, k))
    return hits


def differs_select(form):
    hits = []
    for n, name, v in all_contents():
        present = v[n - 1]
        if np.isnan(present):
            continue
        want = CR.select(v, present)
        got = CR.wrong_select(form, v, present)
        if want[2] != got[2] or not np.array_equal(want[0], got[0]):
            hits.append((name, n))
    return hits


@pytest.mark.parametrize("form,content", [("zeros_not_canonical", "zeros"), ("negatives_not_reversed", "negatives"), ("nan_high", "specials"),
                                          ("ties_from_end", "four"), ("quota_off_by_one", "equal")])
def test_each_wrong_topk_form_changes_a_crafted_input(form, content):
    hits = differs_topk(form)
    assert any(name == content for name, _, _ in hits), (form, hits[:5])


@pytest.mark.parametrize("form,size", [("gt_for_ge", 65), ("tile_last_dropped", CR.TILE)])
def test_each_wrong_select_form_changes_a_crafted_input(form, size):
    """the threshold is a value that is present — the tile's last element itself in the tile-sized case"""
    hits = differs_select(form)
    assert any(n == size for _, n in hits), (form, hits[:5])


def test_the_right_forms_change_nothing():
    for n, name, v in all_contents():
        for k in (1, n, n + 5):
            assert np.array_equal(CR.wrong_topk("none", v, k)[0], CR.topk(v, k)[0]), (name, n, k)


def test_new_entries_are_exported_declared_and_bound():
    import ctypes
    import image_matching_amd as im
    L = im.load_library()
    raw = ctypes.CDLL(im.lib_path())
    header = open(os.path.join(ROOT, "include", "hydia.h")).read()
    for name in NEW_ENTRIES:
        assert hasattr(raw, name) and name in L._hydia_symbols and ("int %s(" % name) in header, name
    for cls, names in ((im.Context, ["decrypt_device", "slots_select", "slots_topk"]),
                       (im.DiagonalReceiver, ["decryptMatches", "decryptTopK", "decryptMatchesMulti", "decryptTopKMulti"]),
                       (im.DiagonalSender, ["scoresToWire"])):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)


# A driver in the reference's call shape (own text): the four OpenFHEWrapper functions of include/openFHE_wrapper.h that take the key
# handles, and the candidate-list methods of the roles
CANDIDATES_CALL_SHAPE = r"""
#include "hydia_roles.hpp"
using namespace std;
using namespace hydia::ofhe;
using hydia::GenCryptoContext; namespace OpenFHEWrapper = hydia::OpenFHEWrapper;
using hydia::DiagonalReceiver; using hydia::DiagonalSender;

size_t run(size_t numVectors, vector<double> queryVector) {
    CryptoContext<DCRTPoly> cc = GenCryptoContext(OpenFHEWrapper::computeRequiredDepth(5), 45);
    auto keyPair = cc->KeyGen();
    PublicKey<DCRTPoly> pk = keyPair.publicKey;
    PrivateKey<DCRTPoly> sk = keyPair.secretKey;
    Ciphertext<DCRTPoly> one = OpenFHEWrapper::encryptFromVector(cc, pk, queryVector);
    vector<double> slots = OpenFHEWrapper::decryptToVector(cc, sk, one);
    vector<double> same = OpenFHEWrapper::decryptToVector(cc, one);
    vector<Ciphertext<DCRTPoly>> several{one, one};
    vector<double> both = OpenFHEWrapper::decryptVectorToVector(cc, sk, several);
    Ciphertext<DCRTPoly> compared = OpenFHEWrapper::chebyshevCompare(cc, one, hydia::MATCH_THRESHOLD, hydia::COMP_DEPTH);

    DiagonalReceiver receiver(cc, pk, sk, numVectors);
    DiagonalSender sender(cc, pk, numVectors);
    vector<Ciphertext<DCRTPoly>> queryCipher = receiver.encryptQuery(queryVector);
    vector<Ciphertext<DCRTPoly>> scores = sender.computeSimilarity(queryCipher);
    vector<uint8_t> message = sender.scoresToWire(scores, 2);
    vector<Ciphertext<DCRTPoly>> arrived = receiver.resultFromWire(message);
    DiagonalReceiver::Candidates best = receiver.decryptTopK(arrived, 10, numVectors);
    DiagonalReceiver::Candidates hits = receiver.decryptMatches(arrived, hydia::MATCH_THRESHOLD, numVectors);
    vector<vector<Ciphertext<DCRTPoly>>> batch{arrived, scores};
    vector<DiagonalReceiver::Candidates> bests = receiver.decryptTopKMulti(batch, 10, numVectors);
    vector<DiagonalReceiver::Candidates> all = receiver.decryptMatchesMulti(batch, hydia::MATCH_THRESHOLD, numVectors, 100);
    return slots.size() + same.size() + both.size() + (compared ? 1 : 0) + best.index.size() + best.value.size() + hits.total + bests.size() + all.size();
}
int main() { return 0; }
"""


def test_candidates_driver_compiles_against_the_roles_header(tmp_path):
    src = tmp_path / "candidates_driver.cpp"
    src.write_text(CANDIDATES_CALL_SHAPE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
