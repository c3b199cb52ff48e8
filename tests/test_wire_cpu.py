"""CPU-only checks of the wire format (include/hydia.h, "wire messages"): the numpy restatement tests/wire_ref.py against Python
integers, the byte counts the README quotes, hydia_wire_peek through ctypes without a GPU, the C++ role header, and the header validator
(image_matching_amd/csrc/wire_format.h) as a stand-alone program under AddressSanitizer / UndefinedBehaviorSanitizer."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

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
def int_pack(residues, w):
    """the format's sentence in Python integers: residue c in bits [c w, (c + 1) w) of one little-endian bit string"""
    big = 0
    for c, r in enumerate(residues):
        big |= (int(r) & ((1 << w) - 1)) << (c * w)
    return big.to_bytes(len(residues) * w // 8, "little")


@pytest.mark.parametrize("w", [33, 45, 46, 47, 59, 60, 64])
def test_restatement_against_python_integers(w):
    n = 128
    rng = np.random.default_rng(w)
    for q in ((1 << (w - 1)) + 12345, (1 << w) - 1):
        assert WR.width(q) == w
        alt = np.zeros(n, dtype=np.uint64)
        alt[0::2] = q - 1
        patterns = [np.zeros(n, dtype=np.uint64), np.ones(n, dtype=np.uint64), np.full(n, q - 1, dtype=np.uint64), alt, np.uint64(q - 1) - alt,
                    rng.integers(0, q, size=n, dtype=np.uint64, endpoint=False)]
        for r in patterns:
            packed = WR.pack_row(r, w)
            assert len(packed) == n * w // 8 == WR.row_bytes(n, q)
            assert packed == int_pack(r, w)
            assert np.array_equal(WR.unpack_row(packed, w, n), r)
        # a neighbour's bits do not bleed: the alternating row's odd residues are exactly zero after the round trip
        assert not WR.unpack_row(WR.pack_row(alt, w), w, n)[1::2].any()
    # 64 consecutive residues make exactly w 64-bit words
    assert len(WR.pack_row(np.zeros(64, dtype=np.uint64), w)) == 8 * w


def test_message_round_trip():
    rng = np.random.default_rng(1)
    mods = [(1 << 59) + 3, (1 << 45) + 9, (1 << 44) + 5]
    rows = np.stack([rng.integers(0, q, size=(2, 3, 1024), dtype=np.uint64) for q in mods], axis=2)
    msg = WR.ct_message(rows, mods, 2.0 ** 45)
    assert len(msg) == WR.HEADER_BYTES + WR.payload_bytes(1024, 2, 3, mods)
    h, back = WR.unpack_message(msg)
    assert (h["type"], h["count"], h["n_polys"], h["n_limbs"], h["scale"], h["log_n"]) == (1, 2, 3, 3, 2.0 ** 45, 10)
    assert np.array_equal(back, rows)


# ------------------------------------------------------------------------------------------------ 2. the README's byte counts
def test_readme_byte_counts_follow_from_the_parameters(im):
    info, moduli, _ = im.describe_params(im.default_params())
    N, nQ, nT, dnum, dim, slots = info["n"], info["n_q"], info["n_q"] + info["n_p"], info["dnum"], info["vector_dim"], info["slots"]
    mods = [int(q) for q in moduli]
    assert [WR.width(q) for q in mods[:nQ]] == [60] + [46, 45] * 5 + [46] and [WR.width(q) for q in mods[nQ:]] == [60] * 4
    H = WR.HEADER_BYTES
    query = H + WR.payload_bytes(N, 1, 1, mods[:nQ])          # one seeded query
    result = H + WR.payload_bytes(N, 1, 2, mods[:nQ])         # a ciphertext of two polynomials on all n_q limbs
    half_key = H + WR.payload_bytes(N, dnum, 1, mods)         # a seeded evaluation key
    key = H + WR.payload_bytes(N, dnum, 2, mods)              # a whole one
    n_keys, r = 1 + (dim - 1), dim
    while r < slots:
        n_keys, r = n_keys + 1, r * 2
    assert (query, half_key, key, n_keys) == (2298216, 9843048, 19685736, 517)
    pk_half = H + WR.payload_bytes(N, 1, 1, mods[:nQ])
    key_set = WR.FILE_HEADER_BYTES + pk_half + n_keys * half_key
    text = re.sub(r"(?<=\d) (?=\d{3}\b)", "", open(os.path.join(ROOT, "README.md")).read())
    for figure in (query, half_key, key, result):
        assert re.search(r"\b%d\b" % figure, text), figure
    assert "%.1f GB" % (key_set / 1e9) in text, key_set
    header = re.sub(r"(?<=\d) (?=\d{3}\b)", "", open(os.path.join(ROOT, "include", "hydia.h")).read())
    for figure in (query, half_key, key):
        assert str(figure) in header, figure


# ------------------------------------------------------------------------------------------------ 3. hydia_wire_peek without a GPU
MODS10 = [(1 << 59) + 1025, (1 << 45) + 7, (1 << 44) + 3, (1 << 46) + 1, (1 << 47) + 5]
SEED = bytes(range(1, 33))


def zeros_message(head):
    return head + bytes(WR.parse_header(head)["payload_bytes"])


def peek_code(im, data, length=None):
    L = im.load_library()
    info = im.hydia._WireInfo()
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    return L.hydia_wire_peek(raw.ctypes.data_as(C.c_void_p) if raw.size else None, len(data) if length is None else length, C.byref(info))


def test_peek_describes_every_type(im):
    cases = [
        (WR.header(1, 10, 3, 2, MODS10[:3], scale=2.0 ** 45), dict(type=1, count=3, n_polys=2, n_limbs=3, rot=0, scale=2.0 ** 45, nonce0=0)),
        (WR.header(1, 10, 1, 3, MODS10[:1], scale=7.5), dict(type=1, count=1, n_polys=3, n_limbs=1, scale=7.5)),
        (WR.header(2, 10, 4, 1, MODS10[:4], scale=2.0 ** 45, a_seed=SEED, nonce0=(1 << 40) - 4), dict(type=2, count=4, nonce0=(1 << 40) - 4, a_seed=SEED)),
        (WR.header(3, 10, 3, 2, MODS10, rot=511), dict(type=3, count=3, n_polys=2, n_limbs=5, rot=511, scale=0.0, a_seed=bytes(32))),
        (WR.header(4, 10, 2, 1, MODS10, rot=0, a_seed=SEED), dict(type=4, count=2, n_polys=1, rot=0, a_seed=SEED)),
        (WR.header(5, 10, 1, 2, MODS10[:4]), dict(type=5, count=1, n_polys=2, n_limbs=4)),
        (WR.header(6, 10, 1, 1, MODS10[:4], a_seed=SEED), dict(type=6, n_polys=1, a_seed=SEED)),
    ]
    for head, want in cases:
        msg = zeros_message(head)
        got = im.wire_peek(msg)
        assert got["log_n"] == 10 and got["header_bytes"] == WR.HEADER_BYTES and got["payload_bytes"] == len(msg) - WR.HEADER_BYTES
        for k, v in want.items():
            assert got[k] == v, (k, got[k], v)
        with pytest.raises(im.HydiaError) as e:
            im.wire_peek(msg[:-1])
        assert e.value.code == ERR_ARG and "len" in str(e.value)


def test_peek_refusals(im):
    good = WR.header(1, 10, 2, 2, MODS10[:3], scale=4.0)
    body = bytes(WR.parse_header(good)["payload_bytes"])
    assert peek_code(im, good + body) == 0
    ct = dict(mtype=1, log_n=10, count=2, n_polys=2, moduli=MODS10[:3], scale=4.0)

    def head(**over):
        return WR.header(**{**ct, **over})

    rows = sum(WR.row_bytes(1024, q) for q in MODS10[:3]) * 2
    wrap = (1 << 64) // rows + 1  # count x n_polys x sum_j N w_j / 8 wraps 64 bits
    assert wrap * rows >= 1 << 64 and wrap < 1 << 64
    bad = {
        "magic": head(magic=b"HYDWIRE2"), "version": head(version=2), "type 0": head(mtype=0), "type 7": head(mtype=7),
        "count 0": head(count=0, payload=0), "n_polys 4": head(n_polys=4), "n_polys 1": head(n_polys=1),
        "n_limbs 0": head(moduli=[], payload=0), "n_limbs 33": head(n_limbs=33), "log_n 9": head(log_n=9), "log_n 17": head(log_n=17),
        "rot on a ciphertext": head(rot=1), "scale nan": head(scale=math.nan), "scale inf": head(scale=math.inf), "scale 0": head(scale=0.0),
        "scale negative": head(scale=-4.0), "reserved": head(reserved=1), "payload_bytes + 8": head(payload=len(body) + 8),
        "payload_bytes - 8": head(payload=len(body) - 8), "seed on an unseeded type": head(a_seed=SEED), "nonce on a batch": head(nonce0=1),
        "modulus 0": head(moduli=[MODS10[0], 0, MODS10[2]]), "modulus past n_limbs": head(moduli=MODS10[:4], n_limbs=3, payload=len(body)),
        "count wraps": head(count=wrap, payload=(wrap * rows) % (1 << 64)),
        "rot = slots": WR.header(3, 10, 3, 2, MODS10, rot=512), "key with a scale": WR.header(3, 10, 3, 2, MODS10, scale=1.0),
        "nonce0 + count > 2^40": WR.header(2, 10, 4, 1, MODS10[:4], scale=4.0, a_seed=SEED, nonce0=(1 << 40) - 3),
        "public key of two": WR.header(5, 10, 2, 2, MODS10[:4]), "whole key with one polynomial": WR.header(3, 10, 3, 1, MODS10),
    }
    for name, h in bad.items():
        claimed = WR.parse_header(h)["payload_bytes"]
        data = h + bytes(min(claimed, 1 << 20))
        assert peek_code(im, data, WR.HEADER_BYTES + claimed if claimed < 1 << 62 else len(data)) == ERR_ARG, name
        assert im.load_library().hydia_last_error().decode().startswith("hydia: wire message refused"), name
    # the length: shorter than a header, truncated, trailing bytes, no buffer
    for data, length in ((good[:100], None), (good + body[:-1], None), (good + body + b"\0", None), (b"", 0)):
        assert peek_code(im, data, length) == ERR_ARG
    assert im.load_library().hydia_wire_peek(None, 400, None) == ERR_ARG
    # and the nonce space's last message is fine
    last = WR.header(2, 10, 3, 1, MODS10[:4], scale=4.0, a_seed=SEED, nonce0=(1 << 40) - 3)
    assert peek_code(im, zeros_message(last)) == 0


# ------------------------------------------------------------------------------------------------ 4. the C++ roles
ROLES_WIRE = r"""
#include "hydia_roles.hpp"
using namespace std;
using hydia::CryptoContext; using hydia::Ciphertext; using hydia::GenCryptoContext;
using hydia::DiagonalReceiver; using hydia::DiagonalSender; using hydia::DiagonalEnroller; using hydia::DeviceRows;

int run(size_t numVectors, vector<double> queryVector, vector<vector<double>> probes, vector<vector<double>> plaintextVectors, const void *devRows) {
    CryptoContext rc = GenCryptoContext(11, 45), sc = GenCryptoContext(11, 45);
    auto keyPair = rc->KeyGenSeeded();
    if (!keyPair) return -1;
    DiagonalReceiver receiver(rc, keyPair.publicKey, keyPair.secretKey, numVectors);
    DiagonalSender sender(sc, numVectors);
    if (!receiver.exportKeysWire("keys.bin") || !receiver.exportKeysWire("keys_whole.bin", false, vector<int>{1, 2})) return -2;
    if (!sender.importKeysWire("keys.bin")) return -3;
    DiagonalEnroller enroller(sc, numVectors);
    enroller.serializeDB(plaintextVectors);
    vector<uint8_t> one = receiver.encryptQueryWire(queryVector);
    vector<uint8_t> many = receiver.encryptQueriesWire(probes);
    vector<uint8_t> dev = receiver.encryptQueriesWire(DeviceRows(devRows, HYDIA_F32, probes.size(), 512));
    hydia_wire_info info;
    if (hydia_wire_peek(one.data(), one.size(), &info) != HYDIA_OK) return -4;
    vector<Ciphertext> queryCipher = sender.queryFromWire(one);
    vector<vector<Ciphertext>> queryCiphers = sender.queriesFromWire(many);
    auto indexCiphers = sender.indexScenarioMulti(queryCiphers);
    vector<Ciphertext> indexCipher = sender.indexScenario(queryCipher);
    vector<uint8_t> back = sender.resultToWire(indexCipher);
    vector<Ciphertext> result = receiver.resultFromWire(back);
    vector<size_t> found = receiver.decryptIndex(result);
    vector<uint8_t> raw = hydia::toWire(rc, queryCipher);
    vector<Ciphertext> again = hydia::fromWire(sc, raw);
    return (int)found.size() + (int)dev.size() + (int)indexCiphers.size() + (int)again.size() + (int)info.count;
}
int main() { return 0; }
"""


def test_roles_header_compiles_with_the_wire_methods(tmp_path):
    src = tmp_path / "roles_wire.cpp"
    src.write_text(ROLES_WIRE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ 5. the validator under sanitizers
def test_header_validator_under_sanitizers(tmp_path):
    """tests/wire_header_check.cpp (own main, wire_format.h alone) built with -fsanitize=address,undefined and run as a subprocess: every
    prefix of a valid header, every single-byte mutation, the wrap-around shapes.  Nothing is loaded into Python, nothing is preloaded."""
    exe = tmp_path / "wire_header_check"
    flags = ["-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if can.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked on this machine: " + can.stderr[-200:])
    b = subprocess.run(["g++"] + flags + ["-I", os.path.join(ROOT, "image_matching_amd", "csrc"), os.path.join(ROOT, "tests", "wire_header_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wire_header_check ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
