"""CPU-only checks of a plain gallery's in-place update and files (hydia_plain_db_update, hydia_plain_db_save / hydia_plain_db_load):
the C-ABI boundary, the role methods' call shape, the facts about the encoder on the oracle that the documented contract rests on
(a created block is the enrolment's, encode(x) + encode(-x) = 0, encode(a) + encode(b) within 1 of encode(a + b) per coefficient),
the restatement (tests/plain_gallery_update_ref.py) through the oracle's index scenario, and the file header restated with struct
(the GPU tests craft their bad files from it)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from conftest import ROOT
from plain_gallery_ref import PlainRef
from plain_gallery_update_ref import PlainUpdateRef, add_mod

NEW_SYMBOLS = ("hydia_plain_db_update", "hydia_plain_db_save", "hydia_plain_db_load")
ALL_SYMBOLS = NEW_SYMBOLS + ("hydia_plain_db_enroll", "hydia_plain_db_alloc")  # the five entry points that give a gallery its life

# ---- the file header (Context::db_save's DbFileHeader): magic, logN, nQ, dim, packed, kind, babies, n_vectors, n_cts, ct_bytes, moduli[32]
HEADER = struct.Struct("<8s6I3Q32Q")
FIELDS = ("magic", "logN", "nQ", "dim", "packed", "kind", "babies", "n_vectors", "n_cts", "ct_bytes")


def read_header(raw):
    v = HEADER.unpack_from(raw)
    h = dict(zip(FIELDS, v[:10]))
    h["moduli"] = list(v[10:])
    return h


def write_header(h):
    return HEADER.pack(*[h[k] for k in FIELDS], *h["moduli"])


def poly_bytes(N, nQ, packed):
    """one polynomial in the ciphertext-major layout: limb 0 as 8-byte residues, the others as 6-byte ones when packed"""
    return N * 8 + (nQ - 1) * N * 6 if packed else nQ * N * 8


def residue_offset(N, nQ, packed, t, j, c):
    """byte offset in the FILE of residue c of limb j of plaintext t, and its width"""
    es = 6 if packed and j > 0 else 8
    limb = j * N * 8 if not packed else (0 if j == 0 else N * 8 + (j - 1) * N * 6)
    return HEADER.size + t * poly_bytes(N, nQ, packed) + limb + c * es, es


def test_the_header_restatement_round_trips():
    assert HEADER.size == 8 + 24 + 24 + 256
    h = dict(magic=b"HYDIADB1", logN=11, nQ=12, dim=64, packed=1, kind=8, babies=8, n_vectors=2045, n_cts=128,
             ct_bytes=poly_bytes(2048, 12, True), moduli=list(range(1, 33)))
    raw = write_header(h)
    assert len(raw) == HEADER.size and read_header(raw) == h
    assert residue_offset(2048, 12, True, 1, 0, 0) == (HEADER.size + h["ct_bytes"], 8)
    assert residue_offset(2048, 12, True, 0, 2, 3) == (HEADER.size + 2048 * 8 + 2048 * 6 + 18, 6)


def test_header_declares_and_library_exports_the_entries():
    import image_matching_amd as im
    if not os.path.exists(im.lib_path()):
        from image_matching_amd.hydia import build_library
        build_library()
    doc = open(os.path.join(ROOT, "include", "hydia.h")).read()
    text = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    raw = ctypes.CDLL(im.lib_path())
    L = im.load_library()
    for name in ALL_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "include/hydia.h does not declare " + name
        assert hasattr(raw, name), "libhydia.so does not export " + name
        assert name in L._hydia_symbols, name
    for m in ("plain_db_update", "plain_db_save", "plain_db_load"):
        assert hasattr(im.Context, m), m
    for m in ("updateRows", "appendDB"):
        assert hasattr(im.PlainEnroller, m), m
    # what the header owes its reader: the rounding note, the exact inverse, and what a bad file leaves behind
    assert "ROUNDING" in doc and "THE EXACT INVERSE" in doc and "leaves NO database resident" in doc


UPDATE_CALL_SHAPE = r"""
#include "hydia_roles.hpp"
using namespace std;
using namespace hydia::ofhe;
using hydia::GenCryptoContext; namespace OpenFHEWrapper = hydia::OpenFHEWrapper;
using hydia::PlainEnroller; using hydia::DiagonalReceiver; using hydia::DiagonalSender;

int run(size_t numVectors, vector<vector<double>> gallery, vector<vector<double>> newcomers, vector<vector<double>> revoked,
        vector<vector<double>> delta) {
    CryptoContext<DCRTPoly> cc = GenCryptoContext(OpenFHEWrapper::computeRequiredDepth(5), 45);
    auto keyPair = cc->KeyGen();
    PublicKey<DCRTPoly> pk = keyPair.publicKey;
    PrivateKey<DCRTPoly> sk = keyPair.secretKey;
    PlainEnroller *enroller = new PlainEnroller(cc, pk, numVectors);
    enroller->serializeDB(gallery);
    bool ok = enroller->appendDB(newcomers);  // no seed: nothing is sampled
    for (auto &row : revoked)
        for (double &x : row) x = -x;
    ok = enroller->updateRows(17, revoked) && ok;
    ok = enroller->updateRows(3, delta, false) && ok;
    size_t n = enroller->size();
    DiagonalSender *sender = new DiagonalSender(cc, pk, n);  // rebuilt for the new vector count
    DiagonalReceiver *receiver = new DiagonalReceiver(cc, pk, sk, n);
    delete receiver;
    delete sender;
    delete enroller;
    return ok ? 0 : 1;
}
int main() { return 0; }
"""


def test_roles_header_update_methods_compile(tmp_path):
    src = tmp_path / "roles_plain_update.cpp"
    src.write_text(UPDATE_CALL_SHAPE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ on the oracle
@pytest.fixture(scope="module")
def tiny():
    P = O.Params(log_n=11, depth=11, dim=16)
    K = O.Keys(P, 3)
    yield P, K, O.Oracle(P, K)
    P.close()


def images(P, rng):
    """dense slot images, and sparse ones as an update of a few rows makes them"""
    dense = [rng.uniform(-1, 1, P.slots) for _ in range(3)]
    sparse = []
    for k in (1, 5):
        s = np.zeros(P.slots)
        s[rng.choice(P.slots, size=k, replace=False)] = rng.uniform(-1, 1, k)
        sparse.append(s)
    return dense + sparse


@pytest.mark.parametrize("babies", [None, 4])
def test_a_created_block_equals_the_enrolments_encoding(tiny, babies):
    """appending rows that open a block: its plaintexts are PlainRef's (the enrolment's) of the same rows, bit for bit"""
    P, K, Or = tiny
    rng = np.random.default_rng(3)
    n0, extra = P.slots, 40
    rows = rng.integers(-99, 100, size=(n0 + extra, P.dim)).astype(np.float64)
    whole = PlainRef(P, Or, rows.copy(), babies)
    up = PlainUpdateRef(P, babies).enroll(PlainRef(P, Or, rows[:n0].copy(), babies))
    touched = up.update(n0, rows[n0:].copy(), 1)
    assert touched == list(range(P.dim, 2 * P.dim)) and up.n == n0 + extra and len(up.pts) == 2 * P.dim
    for t in range(2 * P.dim):
        assert np.array_equal(up.pts[t], whole.encode(t)), t


def test_encode_is_odd(tiny):
    """encode(x) + encode(-x) = 0 in every residue: the encoder rounds symmetrically"""
    P, K, Or = tiny
    for k, x in enumerate(images(P, np.random.default_rng(4))):
        assert not add_mod(P, P.encode(x), P.encode(-x)).any(), k
        assert np.array_equal(P.encode_coeffs(x), -P.encode_coeffs(-x)), k


def test_encode_is_additive_up_to_one_per_coefficient(tiny):
    """encode(a) + encode(b) - encode(a + b) stays within +-1 per coefficient before the transform"""
    P, K, Or = tiny
    xs = images(P, np.random.default_rng(5))
    seen = set()
    for a in xs:
        for b in xs:
            d = P.encode_coeffs(a) + P.encode_coeffs(b) - P.encode_coeffs(a + b)
            assert np.abs(d).max() <= 1
            seen |= set(np.unique(d).tolist())
    assert seen <= {-1, 0, 1} and len(seen) > 1  # the rounding residue is real: an updated block is not a fresh enrolment's


@pytest.mark.parametrize("babies", [None, 4])
def test_index_scenario_over_the_updated_trivial_ciphertexts(tiny, babies):
    """append a planted row, remove another: the oracle's index scenario over the updated trivial ciphertexts finds the first and
    no longer finds the second; the removal restores the untouched encoding of an all-zero slot exactly"""
    P, K, Or = tiny
    rng = np.random.default_rng(6)
    n0 = P.slots - 5
    rows = rng.integers(-99, 100, size=(n0 + 10, P.dim)).astype(np.float64)
    rows[17] = rng.integers(1, 4, size=P.dim)       # a match that is revoked
    rows[n0 + 7] = rng.integers(1, 4, size=P.dim)   # a match among the appended rows (they open block 1)
    ref = PlainRef(P, Or, rows[:n0].copy(), babies)
    up = PlainUpdateRef(P, babies).enroll(ref)
    q = Or.encrypt_query(np.ones(P.dim), 5, 1)
    assert 17 in Or.decrypt_index(Or.index_scenario(q, up.array(), up.n))
    up.update(n0, rows[n0:].copy(), 1)
    assert (up.n, len(up.pts)) == (n0 + 10, 2 * P.dim)
    before = list(up.pts)
    gone = -ref.rows[17:18].copy()  # the negated (normalised) template
    touched = up.update(17, gone.copy(), 1)
    assert touched == list(range(P.dim))
    hits = Or.decrypt_index(Or.index_scenario(q, up.array(), up.n))
    assert n0 + 7 in hits and 17 not in hits
    up.update(17, -gone, 1)  # and back: the exact inverse
    for t in range(2 * P.dim):
        assert np.array_equal(up.pts[t], before[t]), t
