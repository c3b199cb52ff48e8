"""CPU-only checks of re-keying a resident database (hydia_keygen_switch / hydia_db_rekey): the restated switching key against its
defining relation, the restatement of the re-key (tests/db_rekey_ref.py) on the oracle alone — every ciphertext opens under the new
key to what it held under the old one, the scenarios find the planted rows, twice in a row — the C-ABI boundary and the role
methods' call shape.  (The kernels add no granule helper to csrc/db_accum.h: k_db_rekey_store calls db_accumulate_pair /
db_accumulate_granule46 and db_pack_pair48 / db_pack_granule46 as tests/csrc/db_accumulate_check.cpp already checks them.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from conftest import ROOT
from db_rekey_ref import as_oracle_cts, rekey, switch_key, switch_key_parts
from db_update_ref import _CtList
from keyswitch_ref import _ints, _u64

TOL = 1e-4
PLANTED = (5, 400, 1023)


@pytest.fixture(scope="module")
def keys8(small_params):
    return O.Keys(small_params, 8)


@pytest.fixture(scope="module")
def keys9(small_params):
    return O.Keys(small_params, 9)


@pytest.fixture(scope="module")
def enrolled(small_params, small_keys):
    """one block of random templates with three planted matches of the all-ones query, enrolled under key 7 (hoisted)"""
    P = small_params
    rng = np.random.default_rng(11)
    db = rng.integers(-99, 100, size=(P.slots, P.dim)).astype(np.float64)
    for i in PLANTED:
        db[i] = rng.integers(1, 4, size=P.dim)
    arr = O.Oracle(P, small_keys).enroll(db, 41, matvec="hoisted")
    return arr, [arr[t].data().copy() for t in range(len(arr))]


def test_restated_key_satisfies_its_relation(small_params, small_keys, keys8):
    """b + a s_new - P [limb in digit d] s_old = NTT(e), e the sampled Gaussian, on every digit and limb"""
    P = small_params
    key, errs = switch_key_parts(P, small_keys, keys8, 1234)
    assert key.shape == (P.dnum, 2, P.nT, P.N) and np.abs(errs).max() > 0
    q = [int(v) for v in P.moduli]
    PP = 1
    for m in range(P.nQ, P.nT):
        PP *= q[m]
    s_new, s_old = keys8.s_ntt(), small_keys.s_ntt()
    for d in range(P.dnum):
        for m in range(P.nT):
            assert int(key[d].max()) < max(q) and int(key[d, :, m].max()) < q[m]
            v = _ints(key[d, 0, m]) + _ints(key[d, 1, m]) * _ints(s_new[m])
            if m < P.nQ and m // P.alpha == d:
                v = v - PP * _ints(s_old[m])
            want = P.ntt_fwd(_u64(_ints(errs[d]) % q[m]), m)
            assert np.array_equal(_u64(v % q[m]), want), (d, m)
    # another seed is another key; the same seed the same key
    assert not np.array_equal(switch_key(P, small_keys, keys8, 1235), key)
    assert np.array_equal(switch_key(P, small_keys, keys8, 1234), key)


def check_rekeyed(P, K_old_cts_plain, new_arrays, K_new, n):
    """every ciphertext decrypts under the new key to the slots it held; the scenarios under the new keys find the planted rows"""
    Or_new = O.Oracle(P, K_new)
    cts = as_oracle_cts(P, Or_new, new_arrays)
    for t, c in enumerate(cts):
        assert np.abs(Or_new.decrypt(c) - K_old_cts_plain[t]).max() < TOL, t
    db = _CtList(cts, P.dim, P.dim)
    q = Or_new.encrypt_query(np.ones(P.dim), 5, 1)
    assert set(PLANTED) <= set(Or_new.decrypt_index(Or_new.index_scenario(q, db, n)))
    assert Or_new.decrypt_membership(Or_new.membership_scenario(q, db, n)) is True


def test_restatement_on_the_oracle_rekey_and_rekey_again(small_params, small_keys, keys8, keys9, enrolled):
    P = small_params
    arr, old = enrolled
    Or7 = O.Oracle(P, small_keys)
    plain = [Or7.decrypt(arr[t]) for t in range(len(arr))]
    key78 = switch_key(P, small_keys, keys8, 100)
    under8 = rekey(P, old, key78)
    assert len(under8) == P.dim and not np.array_equal(under8[0], old[0])
    check_rekeyed(P, plain, under8, keys8, P.slots)
    # the old key no longer opens it
    assert np.abs(Or7.decrypt(as_oracle_cts(P, Or7, under8[:1])[0]) - plain[0]).max() > TOL
    # 7 -> 8 -> 9: one more key switch's noise, the same rule
    under9 = rekey(P, under8, switch_key(P, keys8, keys9, 101))
    check_rekeyed(P, plain, under9, keys9, P.slots)


def test_header_declares_and_library_exports_the_rekey_entries():
    import image_matching_amd as im
    if not os.path.exists(im.lib_path()):
        from image_matching_amd.hydia import build_library
        build_library()
    doc = open(os.path.join(ROOT, "include", "hydia.h")).read()
    text = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    raw = ctypes.CDLL(im.lib_path())
    for ret, name in (("int", "hydia_keygen_switch"), ("int", "hydia_db_rekey"), ("size_t", "hydia_switch_key_words")):
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), text), "include/hydia.h does not declare " + name
        assert hasattr(raw, name), "libhydia.so does not export " + name
    assert re.search(r"#define\s+HY_EVK_ID_SWITCH\s+\(1ull << 24\)", text)
    # what the header owes its reader: the trust model, the noise, the follow-up, the mixed database
    for words in ("proxy re-encryption", "TRUST MODEL", "NOISE", "FRESH seed", "NEW public key", "MIXED database"):
        assert words in doc, words
    L = im.load_library()
    assert {"hydia_keygen_switch", "hydia_db_rekey", "hydia_switch_key_words"} <= set(L._hydia_symbols)


# A driver in the reference's call shape (see tests/test_capi_cpu.py) that hands its gallery over to a new receiver key
REKEY_CALL_SHAPE = r"""
#include "hydia_roles.hpp"
using namespace std;
using namespace hydia::ofhe;
using hydia::GenCryptoContext; namespace OpenFHEWrapper = hydia::OpenFHEWrapper;
using hydia::DiagonalEnroller; using hydia::DiagonalReceiver; using hydia::DiagonalSender;

int run(size_t numVectors, vector<vector<double>> plaintextVectors, vector<vector<double>> newcomers, const uint8_t *seed32) {
    CryptoContext<DCRTPoly> cc = GenCryptoContext(OpenFHEWrapper::computeRequiredDepth(5), 45);       // the sender's, under the old key
    auto keyPair = cc->KeyGen();
    DiagonalEnroller *enroller = new DiagonalEnroller(cc, keyPair.publicKey, numVectors);
    enroller->serializeDB(plaintextVectors);
    vector<uint64_t> oldSecret((size_t)(cc->info.n_q + cc->info.n_p) * cc->info.n);
    if (hydia_export_secret_key(cc->h, oldSecret.data()) != HYDIA_OK) return 2;
    CryptoContext<DCRTPoly> ccNew = GenCryptoContext(OpenFHEWrapper::computeRequiredDepth(5), 45);    // the new custodian's
    auto newPair = ccNew->KeyGen();
    DiagonalReceiver *receiver = new DiagonalReceiver(ccNew, newPair.publicKey, newPair.secretKey, numVectors);
    vector<uint64_t> key = receiver->genSwitchKey(oldSecret);
    vector<uint64_t> again = receiver->genSwitchKey(oldSecret, seed32);
    bool ok = !key.empty() && key.size() == again.size() && enroller->rekeyDB(key);
    ok = enroller->appendDB(newcomers) && ok;
    delete receiver;
    delete enroller;
    return ok ? 0 : 1;
}
int main() { return 0; }
"""


def test_roles_header_rekey_methods_compile(tmp_path):
    src = tmp_path / "roles_rekey.cpp"
    src.write_text(REKEY_CALL_SHAPE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
