"""Seeded database deltas on the GPU (include/hydia.h, "seeded database deltas"; run with -m gpu): a context that holds the SECRET key
makes the message (c0 halves alone), a context that holds NO key applies it.  Every resident ciphertext is compared bit for bit, through
hydia_db_export_ct, with the restatement on the CPU oracle (tests/db_delta_seeded_ref.py): the blocks of a fresh enrolment are the
reference's E, the blocks of an update are old + E mod q_j.  Ring: N = 2^11, 64-dim vectors (1024 slots, 64 ciphertexts per block)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # (imported before the library is loaded: torch and libhydia.so then share one HIP runtime in the process)

import db_delta_ref as DR
import db_delta_seeded_ref as SD
import oracle_lib as O
import wire_ref as WR
from conftest import ROOT

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -2
KEY_SEED, A_SEED = 7, 1007
N0 = 10 * 1024 - 3  # the resident database of the update and append cases: ten blocks, the last ragged


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def bare_ctx(im):
    return im.Context(im.default_params(log_n=11, vector_dim=64), 0)


@pytest.fixture(scope="module")
def small(im):
    """the owner's context: the secret key (and every other key: it is also the sender of the end-to-end test)"""
    P = O.Params(log_n=11, depth=11, dim=64)
    K = O.Keys(P, KEY_SEED)
    cc = bare_ctx(im)
    cc.keygen(KEY_SEED)
    yield P, K, cc
    cc.close()


@pytest.fixture(scope="module")
def rows10():
    """ten blocks - 3 rows of random templates and 300 more (shared, never modified)"""
    rng = np.random.default_rng(2026)
    db = rng.integers(-99, 100, size=(N0 + 300, 64)).astype(np.float64)
    db.setflags(write=False)
    return db


def moduli(P):
    return [int(q) for q in P.moduli[:P.nQ]]


def form(c):
    return c.db_stats(), c.db_kind(), c.db_babies(), c.db_group(), c.db_residue_bits()


def snapshot(c, ts):
    return form(c), [c.db_export_ct(t) for t in ts]


def unchanged(c, ts, before):
    after = snapshot(c, ts)
    return after[0] == before[0] and all(np.array_equal(a, b) for a, b in zip(after[1], before[1]))


def block(P, g):
    return range(g * P.dim, (g + 1) * P.dim)


# the three cases: (first_vector, rows, seed of the noise).  Their references are computed once per form and shared
CASES = {"enrol": (0, slice(0, 1024 + 300), 61), "update": (900, slice(N0, N0 + 300), 62), "append": (N0, slice(N0, N0 + 300), 63)}
_REF, _BASE = {}, {}


def reference(P, K, rows10, case, B):
    """(normalised rows, touched blocks, [per block the reference's E [dim][2][nQ][N]], the reference's container bytes)"""
    if (case, B) not in _REF:
        first, sl, seed = CASES[case]
        rows = rows10[sl].copy()
        touched, blocks = SD.seeded_blocks(P, K, B, first, rows, True, seed, A_SEED)
        data = SD.build(blocks, touched, moduli(P), P.delta, B, first, rows.shape[0], A_SEED)
        _REF[case, B] = (rows, touched, blocks, data)
    return _REF[case, B]


def base_messages(im, cc, rows10, B):
    """the ten-block database under the PUBLIC key, as unseeded deltas (one per block), made once per form"""
    if B not in _BASE:
        _BASE[B] = list(im.DiagonalEnroller(cc, 0).serializeDBToWire(rows10[:N0].copy(), seed=41, babies=B))
    return _BASE[B]


def sender_with_base(im, cc, rows10, B, env, monkeypatch):
    """a context of its own that holds NO key, created under `env` (the layout is fixed by the context that allocates the database)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    snd = bare_ctx(im)
    for k in env:
        monkeypatch.delenv(k)
    return snd


LAYOUTS = [({}, 46), ({"HYDIA_DB_48BIT": "1"}, 48), ({"HYDIA_DB_UNPACKED": "1"}, 64)]


# ------------------------------------------------------------------------------------------------ 1. make with the key, apply without
@pytest.mark.parametrize("env,bits", LAYOUTS)
@pytest.mark.parametrize("B", [64, 8])
@pytest.mark.parametrize("case", ["enrol", "update", "append"])
def test_apply_equals_the_reference(im, small, rows10, case, B, env, bits, monkeypatch):
    """8-byte residues (HYDIA_DB_UNPACKED), 6-byte residues (HYDIA_DB_48BIT; and ciphertext-major in the two-block hoisted enrolment)
    and the 46-bit granules of the group-sequential layout, in the hoisted form and at babies = 8"""
    P, K, cc = small
    first, sl, seed = CASES[case]
    want_rows, touched, E, want_bytes = reference(P, K, rows10, case, B)
    rows = rows10[sl].copy()
    message = cc.db_delta_make_seeded(first, rows, True, seed=seed, a_seed=A_SEED, babies=B)
    assert np.array_equal(rows, want_rows)  # normalised in place, as the oracle normalises
    assert len(message) == cc.db_delta_seeded_bytes(first, rows.shape[0]) == SD.total_bytes(P.N, P.dim, moduli(P), first, rows.shape[0])
    assert message == want_bytes  # c0 of every ciphertext, the headers, a_seed and the nonces: byte for byte the reference's container
    snd = sender_with_base(im, cc, rows10, B, env, monkeypatch)
    try:
        old = {}
        if case != "enrol":
            for m in base_messages(im, cc, rows10, B):
                snd.db_delta_apply(m)
            assert snd.db_stats()[:2] == (N0, 10 * P.dim) and snd.db_residue_bits() == bits
            assert (snd.db_group() > 0) == (bits != 64)
            for g in touched:
                if g < 10:
                    old[g] = np.stack([snd.db_export_ct(t) for t in block(P, g)])
        untouched = [t for t in (0, 2 * P.dim + 5, 9 * P.dim - 1) if t // P.dim not in touched and case != "enrol"]
        keep = [snd.db_export_ct(t) for t in untouched]
        assert snd.db_kind() == (0 if case == "enrol" else (5 if B == P.dim else 6))
        snd.db_delta_apply_seeded(message)
        n_new = max(N0 if case != "enrol" else 0, first + rows.shape[0])
        assert snd.db_stats()[:2] == (n_new, -(-n_new // P.slots) * P.dim)
        assert snd.db_kind() == (5 if B == P.dim else 6) and snd.db_babies() == B
        if case == "enrol":  # two blocks: hoisted stays ciphertext-major, babies = 8 makes 16 loop-B blocks and goes group-sequential
            assert snd.db_residue_bits() == (64 if bits == 64 else (48 if B == P.dim else bits)) and (snd.db_group() > 0) == (B == 8 and bits != 64)
        else:
            assert snd.db_residue_bits() == bits
        for g, e in zip(touched, E):
            want = SD.fold(P, old.get(g), e)
            for i, t in enumerate(block(P, g)):
                assert np.array_equal(snd.db_export_ct(t), want[i]), (g, i)
        for t, k in zip(untouched, keep):
            assert np.array_equal(snd.db_export_ct(t), k), t
    finally:
        snd.close()


# ------------------------------------------------------------------------------------------------ 2. equivalence with the shipped path
@pytest.mark.parametrize("B", [64, 8])
def test_equals_the_unseeded_delta_of_the_expanded_ciphertexts(im, small, rows10, B):
    """every block message through Context.ct_from_wire (an ordinary type 2 message), the HYDDELT1 delta of those ciphertexts through
    hydia_db_delta_apply on a copy of the database: the same database, the same hydia_db_stats"""
    P, K, cc = small
    first, sl, seed = CASES["update"]
    message = cc.db_delta_make_seeded(first, rows10[sl].copy(), True, seed=seed, a_seed=A_SEED, babies=B)
    h, msgs = SD.split(message)
    a, b = bare_ctx(im), bare_ctx(im)
    try:
        for m in base_messages(im, cc, rows10, B):
            a.db_delta_apply(m)
            b.db_delta_apply(m)
        blocks = []
        for m in msgs:
            cts = b.ct_from_wire(m)
            assert len(cts) == P.dim
            blocks.append(np.stack([c.export()[0] for c in cts]))
            del cts
        whole = DR.build(blocks, moduli(P), P.delta, B, first, 300, 0)
        assert len(message) - 64 - 2 * 360 == (len(whole) - 64 - 2 * 360) // 2
        a.db_delta_apply_seeded(message)
        b.db_delta_apply(whole)
        assert form(a) == form(b) and a.db_stats() == b.db_stats()
        for t in list(range(2 * P.dim)) + [2 * P.dim, 10 * P.dim - 1]:
            assert np.array_equal(a.db_export_ct(t), b.db_export_ct(t)), t
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 3. end to end
def test_a_match_appended_by_seeded_delta_is_found_and_removed(im, small):
    """the owner's context holds every key and, here, the database too.  A planted match appended by a seeded delta is found at its
    index; removed by a seeded negated update it no longer matches"""
    P, K, cc = small
    rng = np.random.default_rng(13)
    n0 = 1000
    db = rng.integers(-99, 100, size=(n0 + 40, P.dim)).astype(np.float64)
    db[n0 + 30] = rng.integers(1, 4, size=P.dim)  # matches the all-ones query, in the block the delta opens
    cc.set_matvec("hoisted")
    try:
        im.DiagonalEnroller(cc, n0).serializeDB(db[:n0].copy(), seed=41)
    finally:
        cc.set_matvec("auto")
    sender, receiver = im.DiagonalSender(cc, n0), im.DiagonalReceiver(cc, n0)
    qc = receiver.encryptQuery(np.ones(P.dim), seed=5, nonce=1)
    assert n0 + 30 not in receiver.decryptIndex(sender.indexScenario(qc))
    enroller = im.DiagonalEnroller(cc, n0)
    more = db[n0:].copy()
    message = enroller.appendToWireSeeded(more, sender.numVectors, seed=42, babies=cc.db_babies())  # a_seed: a fresh hydia_random_seed
    assert enroller.numVectors == n0 + 40 and WR.parse_header(SD.split(message)[1][0])["a_seed"] != bytes(32)
    assert sender.applyDBWireSeeded(message) == n0 + 40 == sender.numVectors == cc.db_stats()[0]
    receiver = im.DiagonalReceiver(cc, n0 + 40)  # rebuilt for the new vector count
    assert n0 + 30 in receiver.decryptIndex(sender.indexScenario(qc))
    gone = -more[30:31]  # `more` was normalised in place: the negated template
    sender.applyDBWireSeeded(enroller.updateToWireSeeded(n0 + 30, gone, True, seed=43, babies=cc.db_babies()))
    assert n0 + 30 not in receiver.decryptIndex(sender.indexScenario(qc))


# ------------------------------------------------------------------------------------------------ 4. refusals
def apply_code(c, data, seeded=True):
    raw = np.frombuffer(b"" if data is None else bytes(data), dtype=np.uint8)
    f = c.L.hydia_db_delta_apply_seeded if seeded else c.L.hydia_db_delta_apply
    return f(c.h, raw.ctypes.data_as(C.c_void_p) if raw.size else None, raw.size)


def refused(c, data, code, ts, before, word=None, seeded=True):
    assert apply_code(c, data, seeded) == code
    if word is not None:
        assert word in c.L.hydia_last_error().decode(), (word, c.L.hydia_last_error().decode())
    assert unchanged(c, ts, before)


def test_refused_deltas_change_nothing(im, small):
    P, K, cc = small
    rng = np.random.default_rng(9)
    n = 1500
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    snd = bare_ctx(im)
    try:
        for m in im.DiagonalEnroller(cc, 0).serializeDBToWireSeeded(db.copy(), seed=3, a_seed=A_SEED + 1):
            snd.db_delta_apply_seeded(m)
        ts = (0, P.dim - 1, P.dim, 2 * P.dim - 1)
        before = snapshot(snd, ts)
        assert before[0][0][:2] == (n, 2 * P.dim)
        rows = rng.integers(-99, 100, size=(30, P.dim)).astype(np.float64)
        first = P.slots - 10
        good = cc.db_delta_make_seeded(first, rows.copy(), True, seed=5, a_seed=A_SEED)  # blocks 0 and 1, both resident
        hdr, messages = SD.split(good)
        assert hdr["n_blocks"] == 2
        mods = moduli(P)
        # ONE bad c0 residue (= q_j): the last residue of the last limb of the last ciphertext of the LAST block.  Block 0 passed its
        # check before it was seen, and nothing of block 0 may have been added
        w, q = WR.width(mods[-1]), mods[-1]
        tail = int.from_bytes(good[-8:], "little")
        bad = good[:-8] + ((tail & ((1 << (64 - w)) - 1)) | (q << (64 - w))).to_bytes(8, "little")
        _, bad_rows = WR.unpack_message(SD.split(bad)[1][1])
        _, good_rows = WR.unpack_message(messages[1])
        assert np.argwhere(bad_rows != good_rows).tolist() == [[P.dim - 1, 0, P.nQ - 1, P.N - 1]] and int(bad_rows[-1, -1, -1, -1]) == q
        refused(snd, bad, ERR_ARG, ts, before, "at or above its modulus")
        # a buffer truncated by one byte, trailing bytes
        refused(snd, good[:-1], ERR_ARG, ts, before, "truncated")
        refused(snd, good + b"\0", ERR_ARG, ts, before, "bytes after the last message")
        # each container at the other's entry point
        whole = cc.db_delta_make(first, rows.copy(), True, seed=5)
        refused(snd, whole, ERR_ARG, ts, before, "hydia_db_delta_apply")
        refused(snd, good, ERR_ARG, ts, before, "magic", seeded=False)

        def delta(msgs=messages, **over):
            return SD.container(**{**dict(vector_dim=P.dim, babies=P.dim, first_vector=first, n_rows=30, first_block=0, messages=msgs), **over})

        assert delta() == good

        def retag(m, **over):
            hd = WR.parse_header(m)
            args = dict(mtype=hd["type"], log_n=hd["log_n"], count=hd["count"], n_polys=hd["n_polys"], moduli=mods, scale=hd["scale"],
                        a_seed=hd["a_seed"], nonce0=hd["nonce0"])
            return WR.header(**{**args, **over}) + m[WR.HEADER_BYTES:]

        refused(snd, delta(msgs=[messages[0], retag(messages[1], a_seed=bytes(range(32)))]), ERR_ARG, ts, before, "a_seed differs")
        refused(snd, delta(msgs=[messages[0], retag(messages[1], nonce0=0)]), ERR_ARG, ts, before, "nonce0 is not")
        refused(snd, delta(first_block=1), ERR_ARG, ts, before, "nonce0 is not")
        refused(snd, delta(version=2), ERR_ARG, ts, before, "version")
        refused(snd, delta(n_blocks=1), ERR_ARG, ts, before, "n_blocks")
        refused(snd, delta(msgs=[messages[0], messages[1] + messages[1][WR.HEADER_BYTES:]]), ERR_ARG, ts, before)  # two polynomials' worth
        # the target
        refused(snd, cc.db_delta_make_seeded(first, rows.copy(), True, seed=5, a_seed=A_SEED, babies=8), ERR_ARG, ts, before, "babies")
        refused(snd, cc.db_delta_make_seeded(n + 1, rows.copy(), True, seed=5, a_seed=A_SEED), ERR_ARG, ts, before, "first_vector")
        assert apply_code(snd, None) == ERR_ARG and unchanged(snd, ts, before)
        # ... and the good delta still applies afterwards
        assert apply_code(snd, good) == 0 and snd.db_stats()[:2] == (n, 2 * P.dim) and not unchanged(snd, ts, before)
    finally:
        snd.close()


def test_refused_targets_and_makers(im, small):
    P, K, cc = small
    rng = np.random.default_rng(10)
    n = 300
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    rows = rng.integers(-99, 100, size=(4, P.dim)).astype(np.float64)
    good = cc.db_delta_make_seeded(0, rows.copy(), True, seed=5, a_seed=A_SEED)
    later = cc.db_delta_make_seeded(7, rows.copy(), True, seed=5, a_seed=A_SEED)
    snd = bare_ctx(im)
    try:
        # nothing resident and a nonzero first_vector; no key is needed to find that out
        assert apply_code(snd, later) == ERR_STATE and "first_vector = 0" in snd.L.hydia_last_error().decode()
        assert snd.db_kind() == 0 and snd.db_stats()[:2] == (0, 0)
        # no secret key on the maker: none at all, and the public key alone
        for with_pk in (False, True):
            if with_pk:
                snd.import_public_key(cc.export_public_key())
            with pytest.raises(im.HydiaError) as e:
                snd.db_delta_make_seeded(0, rows.copy(), True, seed=5, a_seed=A_SEED)
            assert e.value.code == ERR_STATE and "secret key" in str(e.value)
        # a plain gallery, and kind 4 (HERS), resident
        im.PlainEnroller(snd, n).serializeDB(db.copy())
        assert snd.db_kind() in (7, 8)
        stats, pt = snd.db_stats(), snd.plain_db_export_pt(1)
        assert apply_code(snd, good) == ERR_STATE and "hydia_plain_db_update" in snd.L.hydia_last_error().decode()
        assert snd.db_stats() == stats and snd.db_kind() in (7, 8) and np.array_equal(snd.plain_db_export_pt(1), pt)
        im.HersEnroller(snd, n).serializeDB(db.copy(), seed=3)
        assert snd.db_kind() == 4
        before = snapshot(snd, (0, 1))
        refused(snd, good, ERR_STATE, (0, 1), before, "kind 4")
    finally:
        snd.close()
    # the maker's arguments: nothing is written, not even the length of a refused call's message
    L = cc.L
    seed = np.frombuffer((5).to_bytes(32, "little"), dtype=np.uint8).copy()
    aseed = np.frombuffer(int(A_SEED).to_bytes(32, "little"), dtype=np.uint8).copy()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    need = cc.db_delta_seeded_bytes(0, 4)
    buf = np.full(need + 16, 0xA5, dtype=np.uint8)

    def make(r, cnt, babies, cap, sd=seed, ad=aseed, b=buf, first_block=0):
        ln = C.c_size_t(77)
        code = L.hydia_db_delta_make_seeded(cc.h, 0, None if r is None else vp(r), cnt, 1, None if sd is None else vp(sd),
                                            None if ad is None else vp(ad), babies, first_block, None if b is None else vp(b), cap, C.byref(ln))
        return code, ln.value

    keep = rows.copy()
    for babies in (0, 1, 3, 48, 128, -8):
        assert make(keep, 4, babies, buf.size) == (ERR_ARG, 0), babies
    assert make(keep, 0, P.dim, buf.size) == (ERR_ARG, 0)
    assert make(None, 4, P.dim, buf.size)[0] == ERR_ARG
    assert make(keep, 4, P.dim, buf.size, sd=None) == (ERR_ARG, 0) and make(keep, 4, P.dim, buf.size, ad=None) == (ERR_ARG, 0)
    assert make(keep, 4, P.dim, buf.size, ad=seed) == (ERR_ARG, 0) and "a_seed" in L.hydia_last_error().decode()  # a_seed == seed
    # cap one byte short: the bytes function's answer in *len, the buffer untouched
    assert make(keep, 4, P.dim, need - 1) == (ERR_ARG, need) and make(keep, 4, P.dim, need, b=None) == (ERR_ARG, need)
    # the nonce space: the a stream's nonces (first_block + blocks) * vector_dim, and the noise stream's 2^36 above them
    assert make(keep, 4, P.dim, buf.size, first_block=(1 << 40) // P.dim - 1)[0] == ERR_ARG
    assert make(keep, 4, P.dim, buf.size, first_block=((1 << 40) - (1 << 36)) // P.dim)[0] == ERR_ARG
    assert (buf == 0xA5).all() and np.array_equal(keep, rows)  # nothing written, the rows not normalised by a refused call
    assert L.hydia_db_delta_make_seeded(cc.h, 0, vp(keep), 4, 1, vp(seed), vp(aseed), P.dim, 0, vp(buf), buf.size, None) == ERR_ARG
    assert make(keep, 4, P.dim, need) == (0, need) and bytes(buf[:need]) == good and (buf[need:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ 5. bytes and calls
def test_bytes_and_the_device_rows_maker(im, small):
    P, K, cc = small
    rng = np.random.default_rng(11)
    rows32 = rng.integers(-99, 100, size=(30, P.dim)).astype(np.float32)
    first = 2 * P.slots - 7
    host = cc.db_delta_make_seeded(first, rows32.astype(np.float64), True, seed=70, a_seed=A_SEED, first_block=3)
    assert len(host) == cc.db_delta_seeded_bytes(first, 30) == SD.total_bytes(P.N, P.dim, moduli(P), first, 30)
    assert len(host) <= 0.51 * cc.db_delta_bytes(first, 30)
    assert im.db_delta_seeded_peek(host) == dict(version=1, vector_dim=P.dim, babies=P.dim, first_vector=first, n_rows=30, first_block=3, n_blocks=2,
                                                 total_bytes=len(host))
    heads = [WR.parse_header(m) for m in SD.split(host)[1]]
    assert [h["nonce0"] for h in heads] == [(3 + 1) * P.dim, (3 + 2) * P.dim] and all(h["a_seed"] == int(A_SEED).to_bytes(32, "little") for h in heads)
    t = torch.tensor(rows32, device="cuda:0")
    keep = t.clone()
    assert cc.db_delta_make_seeded(first, t, True, seed=70, a_seed=A_SEED, first_block=3) == host  # f32 rows widened on the device
    assert torch.equal(t, keep)
    assert cc.db_delta_make_seeded(5, t, True, seed=71, a_seed=A_SEED, babies=8) == \
        cc.db_delta_make_seeded(5, rows32.astype(np.float64), True, seed=71, a_seed=A_SEED, babies=8)
    # the size is host arithmetic
    for fv, n in ((0, 1), (0, P.slots), (0, P.slots + 1), (P.slots - 1, 2), (5 * P.slots + 1, 3 * P.slots)):
        assert cc.db_delta_seeded_bytes(fv, n) == SD.total_bytes(P.N, P.dim, moduli(P), fv, n)
    for fv, n in ((0, 0), ((1 << 64) - 1, 1), (0, (1 << 64) - 1)):
        with pytest.raises(im.HydiaError) as e:
            cc.db_delta_seeded_bytes(fv, n)
        assert e.value.code == ERR_ARG


ROLES_CALLS = r"""
#include <cstdio>
#include "hydia_roles.hpp"
using namespace std;
using hydia::CryptoContext; using hydia::GenCryptoContext; using hydia::DiagonalSender; using hydia::DiagonalEnroller;

int main() {
    CryptoContext oc = GenCryptoContext(11, 45, 64, 11), sc = GenCryptoContext(11, 45, 64, 11);
    auto keyPair = oc->KeyGen();
    if (!keyPair) return 1;
    DiagonalEnroller enroller(oc, keyPair.publicKey, 0);
    DiagonalSender sender(sc, 0);
    vector<vector<double>> db(1030, vector<double>(64));
    for (size_t i = 0; i < db.size(); i++)
        for (size_t j = 0; j < 64; j++) db[i][j] = (double)((i * 31 + j * 7) % 19) - 9.0 + (j == i % 64 ? 3.0 : 0.0);
    vector<vector<double>> more(db.begin() + 1000, db.end());
    db.resize(1000);
    size_t n = 0, bytes = 0, whole = 0;
    for (const vector<uint8_t> &m : enroller.serializeDBToWireSeeded(db)) n = sender.applyDBWireSeeded(m);
    if (n != 1000) return 2;
    vector<uint8_t> appended = enroller.appendToWireSeeded(more, n);
    if (hydia_db_delta_seeded_bytes(oc->h, 1000, 30, &bytes) != HYDIA_OK || bytes != appended.size()) return 3;
    if (hydia_db_delta_bytes(oc->h, 1000, 30, &whole) != HYDIA_OK || 100 * bytes > 51 * whole) return 4;
    hydia_db_delta_info info;
    if (hydia_db_delta_seeded_peek(appended.data(), appended.size(), &info) != HYDIA_OK || info.n_blocks != 2 || info.first_vector != 1000) return 5;
    if (sender.applyDBWireSeeded(appended) != 1030 || enroller.size() != 1030) return 6;
    if (sender.applyDBWire(appended) != 0 || sc->last_status != HYDIA_ERR_ARG) return 7;  // the unseeded entry refuses it
    std::puts("roles ok");
    return 0;
}
"""


def test_cpp_roles_make_the_same_calls(im, tmp_path):
    """the C++ role methods in a -Werror driver, run: seeded enrolment, append, sizes and peek through include/hydia_roles.hpp"""
    src, exe = tmp_path / "roles_calls.cpp", tmp_path / "roles_calls"
    src.write_text(ROLES_CALLS)
    libdir = os.path.dirname(im.lib_path())
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir, "-lhydia",
                        "-Wl,-rpath," + libdir, "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "roles ok" in r.stdout, (r.returncode, r.stderr[-2000:])
