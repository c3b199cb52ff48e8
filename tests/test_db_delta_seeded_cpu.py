"""CPU-only checks of the seeded database delta (include/hydia.h, "seeded database deltas"): the restatement
(tests/db_delta_seeded_ref.py) is itself sound on the CPU oracle — a restated block decrypts to the rows, c0 + a s is the plaintext
plus e0 bit for bit, and it agrees with tests/seeded_ref.py's query on a shared (a_seed, nonce) — the container round-trips,
hydia_db_delta_seeded_peek through ctypes without a GPU, the sizes the documents quote, the role methods, and the container validator
(image_matching_amd/csrc/delta_seeded_format.h) as a stand-alone program under AddressSanitizer / UndefinedBehaviorSanitizer.
Ring: N = 2^11, 64-dim vectors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import db_delta_ref as DR
import db_delta_seeded_ref as SD
import oracle_lib as O
import seeded_ref as SR
import wire_ref as WR
from conftest import ROOT
from db_rekey_ref import as_oracle_cts
from db_update_ref import DB_NONCE_BASE, UpdateRef

ERR_ARG = -1
TOL = 1e-4
SEED, A_SEED = 7, 1007


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    if not os.path.exists(im.lib_path()):
        from image_matching_amd.hydia import build_library
        build_library()
    return im


@pytest.fixture(scope="module")
def small():
    P = O.Params(log_n=11, depth=11, dim=64)
    K = O.Keys(P, SEED, rotations=[1])
    yield P, K
    P.close()


# ------------------------------------------------------------------------------------------------ 1. the restatement on the oracle
@pytest.mark.parametrize("B,first_block", [(64, 0), (8, 3)])
def test_restated_block_decrypts_to_the_rows(small, B, first_block):
    """rows 1000 .. 1039 touch blocks 0 and 1: every ciphertext of both blocks opens, under the oracle's secret key, to the sparse
    diagonal image of the rows; c0 + a s equals NTT(m + e0) bit for bit; a is the public seed's expansion at the message's nonce"""
    P, K = small
    Or = O.Oracle(P, K)
    rows = np.random.default_rng(3).integers(-99, 100, size=(40, P.dim)).astype(np.float64)
    first = 1000
    touched, blocks = SD.seeded_blocks(P, K, B, first, rows, True, 50, A_SEED, first_block)
    assert touched == [0, 1] and np.allclose(np.linalg.norm(rows, axis=1), 1.0)
    U = UpdateRef(P, Or, babies=B)
    Z, _ = SD.placed(P, first, rows, False)
    s = K.s_ntt()
    seen = False
    for g, cts in zip(touched, blocks):
        assert cts.shape == (P.dim, 2, P.nQ, P.N)
        for i in (0, 1, P.dim // 2 + 3, P.dim - 1):
            image = U.image(Z, g * P.dim + i)
            seen = seen or np.abs(image).max() > 0
            ct = as_oracle_cts(P, Or, [cts[i]])[0]
            assert np.abs(Or.decrypt(ct) - image).max() < TOL, (g, i)
            nonce = (first_block + g) * P.dim + i
            want = SD.noisy_plaintext(P, image, 50, DB_NONCE_BASE + nonce)
            for j in range(P.nQ):
                q = int(P.moduli[j])
                assert np.array_equal((cts[i, 0, j] + SR.mulmod(cts[i, 1, j], s[j], q)) % np.uint64(q), want[j]), (g, i, j)
                assert np.array_equal(cts[i, 1, j], O.sample_uniform(A_SEED, (9 << 56) | (nonce << 16) | j, q, P.N))
    assert seen  # the images looked at are not all empty


def test_agrees_with_the_seeded_query_on_a_shared_stream(small):
    """the same (a_seed, nonce) and the same (seed, nonce) give the query of tests/seeded_ref.py: one stream domain, one expansion"""
    P, K = small
    query = np.random.default_rng(4).integers(-99, 100, size=P.dim).astype(np.float64)
    for nonce in (1, 3 * P.dim + 5, (1 << 40) - 1):
        c0, a = SR.seeded_query(P, K, query, SEED, A_SEED, nonce)
        assert np.array_equal(a, SD.expand_a(P, A_SEED, nonce))
        got0, got1 = SD.seeded_ct(P, K, SR.tiled_probe(P, query), SEED, A_SEED, nonce, nonce)
        assert np.array_equal(got0, c0) and np.array_equal(got1, a)
    # the two nonces are independent: the noise moves c0 and leaves a
    c0b, ab = SD.seeded_ct(P, K, SR.tiled_probe(P, query), SEED, A_SEED, 2, 1)
    c0, a = SR.seeded_query(P, K, query, SEED, A_SEED, 1)
    assert np.array_equal(ab, a) and not np.array_equal(c0b, c0)


def test_fold_is_addition_mod_q(small):
    P, _ = small
    rng = np.random.default_rng(5)
    old = np.stack([rng.integers(0, int(q), size=(2, P.N), dtype=np.uint64) for q in P.moduli[:P.nQ]], axis=1)
    E = np.stack([rng.integers(0, int(q), size=(2, P.N), dtype=np.uint64) for q in P.moduli[:P.nQ]], axis=1)
    for j in range(P.nQ):
        old[:, j, :3] = int(P.moduli[j]) - 1
        E[:, j, :3] = (int(P.moduli[j]) - 1, 1, 0)
    got = SD.fold(P, old, E)
    for j in (0, 1, P.nQ - 1):
        q = int(P.moduli[j])
        assert [int(v) for v in got[1, j, :40]] == [(int(x) + int(y)) % q for x, y in zip(old[1, j, :40], E[1, j, :40])]
    assert np.array_equal(SD.fold(P, None, E), E)


# ------------------------------------------------------------------------------------------------ 2. the container
MODS10 = [(1 << 59) + 1025, (1 << 45) + 7, (1 << 44) + 3]
DIM, N, SLOTS = 4, 1024, 512
SCALE = 2.0 ** 45
ASEED32 = bytes(range(100, 132))


def random_blocks(count, seed=1):
    rng = np.random.default_rng(seed)
    return [np.stack([rng.integers(0, q, size=(DIM, 2, N), dtype=np.uint64) for q in MODS10], axis=2) for _ in range(count)]


def test_container_round_trip():
    blocks = random_blocks(3)
    data = SD.build(blocks, [0, 1, 2], MODS10, SCALE, babies=2, first_vector=500, n_rows=2 * SLOTS, a_seed=ASEED32, first_block=7)
    assert len(data) == SD.total_bytes(N, DIM, MODS10, 500, 2 * SLOTS) == DR.HEADER_BYTES + 3 * SD.message_bytes(N, DIM, MODS10)
    assert data[:8] == b"HYDDELS1" and len(data) % 8 == 0
    # half the unseeded delta's payload
    assert 2 * (len(data) - 64 - 3 * 360) == DR.total_bytes(N, DIM, MODS10, 500, 2 * SLOTS) - 64 - 3 * 360
    h, messages = SD.split(data)
    assert h == dict(magic=SD.MAGIC, version=1, vector_dim=DIM, babies=2, first_vector=500, n_rows=2 * SLOTS, first_block=7, n_blocks=3, reserved=0)
    for g, (m, want) in enumerate(zip(messages, blocks)):
        wh, rows = WR.unpack_message(m)
        assert (wh["type"], wh["count"], wh["n_polys"], wh["n_limbs"], wh["scale"], wh["log_n"]) == (2, DIM, 1, 3, SCALE, 10)
        assert wh["a_seed"] == ASEED32 and wh["nonce0"] == (7 + g) * DIM
        assert np.array_equal(rows[:, 0], want[:, 0])
    # the header has the unseeded delta's fields at its offsets
    assert data[8:64] == DR.header(DIM, 2, 500, 2 * SLOTS, 7, 3)[8:]


# ------------------------------------------------------------------------------------------------ 3. hydia_db_delta_seeded_peek without a GPU
def peek_code(im, data, length=None, seeded=True):
    L = im.load_library()
    info = im.hydia._DeltaInfo()
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    f = L.hydia_db_delta_seeded_peek if seeded else L.hydia_db_delta_peek
    return f(raw.ctypes.data_as(C.c_void_p) if raw.size else None, len(data) if length is None else length, C.byref(info))


def zero_message(nonce0, count=DIM, n_polys=1, moduli=MODS10, scale=SCALE, mtype=2, log_n=10, a_seed=ASEED32, **over):
    head = WR.header(mtype, log_n, count, n_polys, moduli, scale=scale, a_seed=a_seed, nonce0=nonce0, **over)
    return head + bytes(WR.parse_header(head)["payload_bytes"])


def test_peek_describes_a_seeded_delta(im):
    data = SD.build(random_blocks(2), [0, 1], MODS10, SCALE, babies=DIM, first_vector=SLOTS - 3, n_rows=10, a_seed=ASEED32, first_block=5)
    got = im.db_delta_seeded_peek(data)
    assert got == dict(version=1, vector_dim=DIM, babies=DIM, first_vector=SLOTS - 3, n_rows=10, first_block=5, n_blocks=2, total_bytes=len(data))
    for cut in (data[:-1], data[:DR.HEADER_BYTES + 100], data[:40], data + b"\0"):
        with pytest.raises(im.HydiaError) as e:
            im.db_delta_seeded_peek(cut)
        assert e.value.code == ERR_ARG and "len" in str(e.value)
    # each container is refused by the other's entry point, by its magic; the seeded one names where an unseeded delta goes
    with pytest.raises(im.HydiaError) as e:
        im.db_delta_peek(data)
    assert e.value.code == ERR_ARG and "magic" in str(e.value)
    whole = DR.build(random_blocks(2), MODS10, SCALE, babies=DIM, first_vector=SLOTS - 3, n_rows=10, first_block=5)
    assert im.db_delta_peek(whole)["n_blocks"] == 2
    with pytest.raises(im.HydiaError) as e:
        im.db_delta_seeded_peek(whole)
    assert e.value.code == ERR_ARG and "magic" in str(e.value) and "hydia_db_delta_apply" in str(e.value)


def test_peek_refusals(im):
    fb = 5
    good = [zero_message((fb + 0) * DIM), zero_message((fb + 1) * DIM)]
    base = dict(vector_dim=DIM, babies=DIM, first_vector=SLOTS - 3, n_rows=10, first_block=fb, messages=good)

    def delta(**over):
        return SD.container(**{**base, **over})

    assert peek_code(im, delta()) == 0
    other = bytes(range(32))
    bad = {
        "magic": delta(magic=b"HYDDELS2"), "the unseeded magic": delta(magic=b"HYDDELT1"), "version": delta(version=2), "reserved": delta(reserved=1),
        "vector_dim 3": delta(vector_dim=3), "babies 3": delta(babies=3), "n_rows 0": delta(n_rows=0), "n_blocks 0": delta(n_blocks=0, messages=[]),
        "rows in one block, two messages": delta(n_rows=3), "n_blocks 1, two messages": delta(n_blocks=1),
        "first_vector + n_rows wraps": delta(first_vector=(1 << 64) - 5, n_rows=10),
        "a ciphertext batch": delta(messages=[good[0], zero_message(0, mtype=1, n_polys=2, a_seed=bytes(32))]),
        "two polynomials": delta(messages=[zero_message(fb * DIM, n_polys=2), good[1]]),
        "two seeds": delta(messages=[good[0], zero_message((fb + 1) * DIM, a_seed=other)]),
        "nonce0 of message 0": delta(messages=[zero_message(fb * DIM + 1), good[1]]),
        "nonce0 of message 1": delta(messages=[good[0], zero_message(fb * DIM)]),
        "nonce0 without first_block": delta(messages=[zero_message(0), zero_message(DIM)]),
        "first_block out of step": delta(first_block=fb + 1),
        "nonces beyond 2^40": SD.container(DIM, DIM, 0, 1, (1 << 40) // DIM - 1, [zero_message((1 << 40) - DIM)]),
        "count": delta(messages=[good[0], zero_message((fb + 1) * DIM, count=DIM + 1)]),
        "a wire type 7": delta(messages=[zero_message(fb * DIM, mtype=7), good[1]]),
        "rings differ": delta(messages=[good[0], zero_message((fb + 1) * DIM, log_n=11)]),
        "trailing message": delta(messages=good + good[:1]), "one message": delta(messages=good[:1]),
    }
    L = im.load_library()
    for name, data in bad.items():
        assert peek_code(im, data) == ERR_ARG, name
        assert L.hydia_last_error().decode().startswith("hydia: seeded database delta refused"), name
    assert peek_code(im, SD.container(DIM, DIM, 0, 1, (1 << 40) // DIM - 2, [zero_message((1 << 40) - 2 * DIM)])) == 0  # the last block that fits
    assert L.hydia_db_delta_seeded_peek(None, 400, None) == ERR_ARG and peek_code(im, b"", 0) == ERR_ARG
    assert peek_code(im, delta(), seeded=False) == ERR_ARG  # hydia_db_delta_peek keeps refusing it


# ------------------------------------------------------------------------------------------------ 4. sizes, arguments, roles
def test_sizes_follow_from_the_parameters(im):
    info, moduli, _ = im.describe_params(im.default_params())
    n, nQ, dim = info["n"], info["n_q"], info["vector_dim"]
    mods = [int(q) for q in moduli[:nQ]]
    message = SD.message_bytes(n, dim, mods)
    assert message == 1176502632 == 360 + 512 * 2297856
    assert SD.total_bytes(n, dim, mods, 0, n // 2) == 64 + message and SD.total_bytes(n, dim, mods, n // 2 - 1, 2) == 64 + 2 * message
    assert message / DR.message_bytes(n, dim, mods) < 0.51
    for doc in ("README.md", os.path.join("include", "hydia.h")):
        text = re.sub(r"(?<=\d) (?=\d{3}\b)", "", open(os.path.join(ROOT, doc)).read())
        assert re.search(r"\b%d\b" % message, text), doc


def test_entry_points_refuse_null_arguments(im):
    """the refusals that come before the context is looked at; the arithmetic on a context is checked on the GPU
    (tests/test_gpu_db_delta_seeded.py), where contexts exist"""
    L = im.load_library()
    b = C.c_size_t(5)
    assert L.hydia_db_delta_seeded_bytes(None, 0, 1, C.byref(b)) == ERR_ARG
    assert L.hydia_db_delta_seeded_bytes(None, 0, 1, None) == ERR_ARG
    assert L.hydia_db_delta_apply_seeded(None, None, 0) == ERR_ARG
    assert L.hydia_db_delta_make_seeded(None, 0, None, 1, 1, None, None, 64, 0, None, 0, None) == ERR_ARG
    assert L.hydia_db_delta_make_seeded_device(None, 0, None, 1, None, None, 64, 0, None, 0, None) == ERR_ARG


def test_role_methods_refuse_a_sharded_context(im):
    group = object()
    rows = np.ones((2, 4))
    calls = [lambda: im.DiagonalEnroller(group, 0).updateToWireSeeded(0, rows), lambda: im.DiagonalEnroller(group, 0).appendToWireSeeded(rows, 0),
             lambda: list(im.DiagonalEnroller(group, 0).serializeDBToWireSeeded(rows)), lambda: im.DiagonalSender(group, 0).applyDBWireSeeded(b"")]
    for call in calls:
        with pytest.raises(im.HydiaError) as e:
            call()
        assert e.value.code == -2 and "sharded" in str(e.value)


def test_torch_is_not_imported_for_host_rows():
    """the seeded methods take host rows without importing torch (a child process: this one may have imported it already)"""
    code = ("import sys, numpy as np\nimport image_matching_amd as im\n"
            "try:\n    im.DiagonalEnroller(object(), 0).updateToWireSeeded(0, np.ones((2, 4)))\nexcept im.HydiaError:\n    pass\n"
            "try:\n    im.db_delta_seeded_peek(b'')\nexcept im.HydiaError:\n    pass\n"
            "assert 'torch' not in sys.modules\nprint('ok')\n")
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env={**os.environ, "PYTHONPATH": ROOT})
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


ROLES_DELTA_SEEDED = r"""
#include "hydia_roles.hpp"
using namespace std;
using hydia::CryptoContext; using hydia::Ciphertext; using hydia::GenCryptoContext;
using hydia::DiagonalReceiver; using hydia::DiagonalSender; using hydia::DiagonalEnroller; using hydia::DeviceRows;

int run(size_t numVectors, vector<double> queryVector, vector<vector<double>> plaintextVectors, vector<vector<double>> more, const void *devRows) {
    CryptoContext oc = GenCryptoContext(11, 45), sc = GenCryptoContext(11, 45);
    auto keyPair = oc->KeyGen();
    if (!keyPair) return -1;
    DiagonalReceiver receiver(oc, keyPair.publicKey, keyPair.secretKey, numVectors);
    DiagonalEnroller enroller(oc, keyPair.publicKey, 0);   // the owner: the secret key and the templates on one context
    DiagonalSender sender(sc, 0);                           // the database and nothing else
    vector<vector<uint8_t>> enrolment = enroller.serializeDBToWireSeeded(plaintextVectors);
    size_t n = 0;
    for (const vector<uint8_t> &m : enrolment) n = sender.applyDBWireSeeded(m);
    vector<uint8_t> appended = enroller.appendToWireSeeded(more, n);
    n = sender.applyDBWireSeeded(appended);
    vector<vector<double>> gone{plaintextVectors[3]};
    for (double &x : gone[0]) x = -x;
    uint8_t seed[32] = {1}, aseed[32] = {2};
    vector<uint8_t> removed = enroller.updateToWireSeeded(3, gone, true, seed, aseed, 8, 2);
    vector<uint8_t> dev = enroller.updateToWireSeeded(n, DeviceRows(devRows, HYDIA_F32, more.size(), 512), true);
    vector<uint8_t> dev2 = enroller.appendToWireSeeded(DeviceRows(devRows, HYDIA_F16, more.size(), 512), n, nullptr, nullptr, 8);
    hydia_db_delta_info info;
    if (hydia_db_delta_seeded_peek(removed.data(), removed.size(), &info) != HYDIA_OK) return -2;
    size_t bytes = 0;
    if (hydia_db_delta_seeded_bytes(oc->h, 0, 1, &bytes) != HYDIA_OK) return -3;
    return (int)sender.applyDBWireSeeded(removed) + (int)dev.size() + (int)dev2.size() + (int)info.n_blocks + (int)enroller.size() + (int)bytes;
}
int main() { return 0; }
"""


def test_roles_header_compiles_with_the_seeded_delta_methods(tmp_path):
    src = tmp_path / "roles_delta_seeded.cpp"
    src.write_text(ROLES_DELTA_SEEDED)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ 5. the validator under sanitizers
def test_container_validator_under_sanitizers(tmp_path):
    """tests/delta_seeded_header_check.cpp (own main, the three format headers alone) built with -fsanitize=address,undefined and run
    as a subprocess.  Nothing is loaded into Python, nothing is preloaded."""
    exe = tmp_path / "delta_seeded_header_check"
    flags = ["-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if can.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked on this machine: " + can.stderr[-200:])
    b = subprocess.run(["g++"] + flags + ["-I", os.path.join(ROOT, "image_matching_amd", "csrc"),
                        os.path.join(ROOT, "tests", "delta_seeded_header_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "delta_seeded_header_check ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
