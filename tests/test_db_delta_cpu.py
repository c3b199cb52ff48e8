"""CPU-only checks of the database delta (include/hydia.h, "database deltas"): the Python restatement of the container
(tests/db_delta_ref.py) round-trips, hydia_db_delta_bytes and hydia_db_delta_peek through ctypes without a GPU against it, the sizes the
documents quote, the C++ role header, and the container validator (image_matching_amd/csrc/delta_format.h) as a stand-alone program
under AddressSanitizer / UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import db_delta_ref as DR
import wire_ref as WR
from conftest import ROOT

ERR_ARG = -1


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    if not os.path.exists(im.lib_path()):
        from image_matching_amd.hydia import build_library
        build_library()
    return im


# ------------------------------------------------------------------------------------------------ 1. the restatement
MODS10 = [(1 << 59) + 1025, (1 << 45) + 7, (1 << 44) + 3]
DIM, N, SLOTS = 4, 1024, 512
SCALE = 2.0 ** 45


def random_blocks(count, seed=1):
    rng = np.random.default_rng(seed)
    return [np.stack([rng.integers(0, q, size=(DIM, 2, N), dtype=np.uint64) for q in MODS10], axis=2) for _ in range(count)]


def test_container_round_trip():
    assert DR.touched_blocks(0, 1, SLOTS) == [0] and DR.touched_blocks(0, SLOTS, SLOTS) == [0] and DR.touched_blocks(0, SLOTS + 1, SLOTS) == [0, 1]
    assert DR.touched_blocks(SLOTS - 1, 2, SLOTS) == [0, 1] and DR.touched_blocks(3 * SLOTS, 1, SLOTS) == [3]
    assert DR.touched_blocks(500, 2 * SLOTS, SLOTS) == [0, 1, 2]
    blocks = random_blocks(3)
    data = DR.build(blocks, MODS10, SCALE, babies=2, first_vector=500, n_rows=2 * SLOTS, first_block=7)
    assert len(data) == DR.total_bytes(N, DIM, MODS10, 500, 2 * SLOTS) == DR.HEADER_BYTES + 3 * DR.message_bytes(N, DIM, MODS10)
    assert data[:8] == b"HYDDELT1" and len(data) % 8 == 0
    h, messages = DR.split(data)
    assert h == dict(magic=DR.MAGIC, version=1, vector_dim=DIM, babies=2, first_vector=500, n_rows=2 * SLOTS, first_block=7, n_blocks=3, reserved=0)
    assert len(messages) == 3
    for m, want in zip(messages, blocks):
        wh, rows = WR.unpack_message(m)
        assert (wh["type"], wh["count"], wh["n_polys"], wh["n_limbs"], wh["scale"], wh["log_n"]) == (1, DIM, 2, 3, SCALE, 10)
        assert np.array_equal(rows, want)
    # the header's layout in the format's own words: offsets 0 / 8 / 12 / 16 / 24 / 32 / 40 / 48 / 56, little-endian
    raw = DR.header(DIM, 2, 500, 2 * SLOTS, 7, 3)
    assert len(raw) == 64 and raw[8:12] == (1).to_bytes(4, "little") and raw[12:16] == DIM.to_bytes(4, "little")
    for off, v in ((16, 2), (24, 500), (32, 2 * SLOTS), (40, 7), (48, 3), (56, 0)):
        assert raw[off:off + 8] == v.to_bytes(8, "little"), off


# ------------------------------------------------------------------------------------------------ 2. hydia_db_delta_peek without a GPU
def peek_code(im, data, length=None):
    L = im.load_library()
    info = im.hydia._DeltaInfo()
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    return L.hydia_db_delta_peek(raw.ctypes.data_as(C.c_void_p) if raw.size else None, len(data) if length is None else length, C.byref(info))


def zero_message(count=DIM, n_polys=2, moduli=MODS10, scale=SCALE, mtype=1, log_n=10, **over):
    head = WR.header(mtype, log_n, count, n_polys, moduli, scale=scale, **over)
    return head + bytes(WR.parse_header(head)["payload_bytes"])


def test_peek_describes_a_delta(im):
    data = DR.build(random_blocks(2), MODS10, SCALE, babies=DIM, first_vector=SLOTS - 3, n_rows=10, first_block=5)
    got = im.db_delta_peek(data)
    assert got == dict(version=1, vector_dim=DIM, babies=DIM, first_vector=SLOTS - 3, n_rows=10, first_block=5, n_blocks=2, total_bytes=len(data))
    for cut in (data[:-1], data[:DR.HEADER_BYTES + 100], data[:40], data + b"\0"):
        with pytest.raises(im.HydiaError) as e:
            im.db_delta_peek(cut)
        assert e.value.code == ERR_ARG and "len" in str(e.value)


def test_peek_refusals(im):
    good = [zero_message(), zero_message()]
    base = dict(vector_dim=DIM, babies=DIM, first_vector=SLOTS - 3, n_rows=10, first_block=0, messages=good)

    def delta(**over):
        return DR.container(**{**base, **over})

    assert peek_code(im, delta()) == 0
    bad = {
        "magic": delta(magic=b"HYDDELT2"), "version": delta(version=2), "reserved": delta(reserved=1),
        "vector_dim 0": delta(vector_dim=0), "vector_dim 3": delta(vector_dim=3),
        "babies 0": delta(babies=0), "babies 1": delta(babies=1), "babies 3": delta(babies=3), "babies 8": delta(babies=8),
        "n_rows 0": delta(n_rows=0), "n_blocks 0": delta(n_blocks=0, messages=[]),
        "rows in one block, two messages": delta(n_rows=3), "rows in three blocks, two messages": delta(n_rows=SLOTS + 4),
        "n_blocks 1, two messages": delta(n_blocks=1), "n_blocks 3, two messages": delta(n_blocks=3, n_rows=SLOTS + 4),
        "first_vector + n_rows wraps": delta(first_vector=(1 << 64) - 5, n_rows=10),
        "count": delta(messages=[good[0], zero_message(count=DIM + 1)]), "three polynomials": delta(messages=[zero_message(n_polys=3), good[1]]),
        "a seeded query": delta(messages=[good[0], zero_message(mtype=2, n_polys=1, a_seed=bytes(range(32)))]),
        "a wire type 7": delta(messages=[zero_message(mtype=7), good[1]]), "scale 0": delta(messages=[zero_message(scale=0.0), good[1]]),
        "rings differ": delta(messages=[good[0], zero_message(log_n=11)]),
        "vector_dim exceeds the slots": DR.container(1024, 1024, 0, 1, 0, [zero_message(count=1024, moduli=MODS10[:1])]),
        "trailing message": delta(messages=good + good[:1]), "no messages": delta(messages=[]), "one message": delta(messages=good[:1]),
    }
    L = im.load_library()
    for name, data in bad.items():
        assert peek_code(im, data) == ERR_ARG, name
        assert L.hydia_last_error().decode().startswith("hydia: database delta refused"), name
    assert L.hydia_db_delta_peek(None, 400, None) == ERR_ARG and peek_code(im, b"", 0) == ERR_ARG


# ------------------------------------------------------------------------------------------------ 3. hydia_db_delta_bytes and the documents' sizes
def delta_bytes_code(im, cc, first, n):
    b = C.c_size_t(123)
    return im.load_library().hydia_db_delta_bytes(cc, first, n, C.byref(b)), b.value


def test_sizes_follow_from_the_parameters(im):
    info, moduli, _ = im.describe_params(im.default_params())
    n, nQ, dim = info["n"], info["n_q"], info["vector_dim"]
    mods = [int(q) for q in moduli[:nQ]]
    message = DR.message_bytes(n, dim, mods)
    resident = dim * 2 * (n * 8 + (nQ - 1) * (n // 128) * 736)  # the group-sequential 46-bit layout: limb 0 in 8 bytes, 128 residues in 736
    assert (message, resident) == (2353004904, 2390753280)
    assert DR.total_bytes(n, dim, mods, 0, 1) == 64 + message and DR.total_bytes(n, dim, mods, n // 2 - 1, 2) == 64 + 2 * message
    for doc in ("README.md", os.path.join("include", "hydia.h")):
        text = re.sub(r"(?<=\d) (?=\d{3}\b)", "", open(os.path.join(ROOT, doc)).read())
        for figure in (message, resident):
            assert re.search(r"\b%d\b" % figure, text), (doc, figure)


def test_delta_bytes_needs_no_gpu_arguments(im):
    """the refusals that come before the context is looked at; the arithmetic on a context is checked on the GPU
    (tests/test_gpu_db_delta.py), where contexts exist"""
    L = im.load_library()
    b = C.c_size_t(5)
    assert L.hydia_db_delta_bytes(None, 0, 1, C.byref(b)) == ERR_ARG
    assert L.hydia_db_delta_bytes(None, 0, 1, None) == ERR_ARG
    assert L.hydia_db_delta_apply(None, None, 0) == ERR_ARG
    assert L.hydia_db_delta_make(None, 0, None, 1, 1, None, 64, 0, None, 0, None) == ERR_ARG
    assert L.hydia_db_delta_make_device(None, 0, None, 1, None, 64, 0, None, 0, None) == ERR_ARG


def test_role_methods_refuse_a_sharded_context(im):
    """anything that is not ONE Context (a ShardGroup) is refused before the library is called, as the wire methods refuse it"""
    group = object()
    rows = np.ones((2, 4))
    calls = [lambda: im.DiagonalEnroller(group, 0).updateToWire(0, rows), lambda: im.DiagonalEnroller(group, 0).appendToWire(rows, 0),
             lambda: list(im.DiagonalEnroller(group, 0).serializeDBToWire(rows)), lambda: im.DiagonalSender(group, 0).applyDBWire(b"")]
    for call in calls:
        with pytest.raises(im.HydiaError) as e:
            call()
        assert e.value.code == -2 and "sharded" in str(e.value)


# ------------------------------------------------------------------------------------------------ 4. the C++ roles
ROLES_DELTA = r"""
#include "hydia_roles.hpp"
using namespace std;
using hydia::CryptoContext; using hydia::Ciphertext; using hydia::GenCryptoContext;
using hydia::DiagonalReceiver; using hydia::DiagonalSender; using hydia::DiagonalEnroller; using hydia::DeviceRows;

int run(size_t numVectors, vector<double> queryVector, vector<vector<double>> plaintextVectors, vector<vector<double>> more, const void *devRows) {
    CryptoContext rc = GenCryptoContext(11, 45), ec = GenCryptoContext(11, 45), sc = GenCryptoContext(11, 45);
    auto keyPair = rc->KeyGen();
    if (!keyPair) return -1;
    DiagonalReceiver receiver(rc, keyPair.publicKey, keyPair.secretKey, numVectors);
    DiagonalEnroller enroller(ec, keyPair.publicKey, 0);   // the public key and nothing else
    DiagonalSender sender(sc, 0);                           // the database and nothing else
    vector<vector<uint8_t>> enrolment = enroller.serializeDBToWire(plaintextVectors);
    size_t n = 0;
    for (const vector<uint8_t> &m : enrolment) n = sender.applyDBWire(m);
    vector<uint8_t> appended = enroller.appendToWire(more, n);
    n = sender.applyDBWire(appended);
    vector<vector<double>> gone{plaintextVectors[3]};
    for (double &x : gone[0]) x = -x;
    uint8_t seed[32] = {1};
    vector<uint8_t> removed = enroller.updateToWire(3, gone, true, seed, 8, 2);
    vector<uint8_t> dev = enroller.updateToWire(n, DeviceRows(devRows, HYDIA_F32, more.size(), 512), true);
    vector<uint8_t> dev2 = enroller.appendToWire(DeviceRows(devRows, HYDIA_F16, more.size(), 512), n, nullptr, 8);
    hydia_db_delta_info info;
    if (hydia_db_delta_peek(removed.data(), removed.size(), &info) != HYDIA_OK) return -2;
    size_t bytes = 0;
    if (hydia_db_delta_bytes(ec->h, 0, 1, &bytes) != HYDIA_OK) return -3;
    return (int)sender.applyDBWire(removed) + (int)dev.size() + (int)dev2.size() + (int)info.n_blocks + (int)enroller.size() + (int)bytes;
}
int main() { return 0; }
"""


def test_roles_header_compiles_with_the_delta_methods(tmp_path):
    src = tmp_path / "roles_delta.cpp"
    src.write_text(ROLES_DELTA)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ 5. the validator under sanitizers
def test_container_validator_under_sanitizers(tmp_path):
    """tests/delta_header_check.cpp (own main, delta_format.h and wire_format.h alone) built with -fsanitize=address,undefined and run
    as a subprocess: every refusal of the container check, every prefix of the headers, every single-byte mutation, the wrap-around
    cases.  Nothing is loaded into Python, nothing is preloaded."""
    exe = tmp_path / "delta_header_check"
    flags = ["-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if can.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked on this machine: " + can.stderr[-200:])
    b = subprocess.run(["g++"] + flags + ["-I", os.path.join(ROOT, "image_matching_amd", "csrc"), os.path.join(ROOT, "tests", "delta_header_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "delta_header_check ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
