"""Database deltas on the GPU (include/hydia.h, "database deltas"; run with -m gpu): the enroller's context (public key only) makes
the message, the sender's applies it.  The bytes are compared with the container built in Python (tests/db_delta_ref.py over
tests/wire_ref.py) from the oracle's fresh encryptions E; the database after an apply is compared bit for bit with a twin context that
ran hydia_db_update with the same arguments AND with the restatement on the CPU oracle (tests/db_update_ref.py).  Every refusal is
checked to leave the database, its layout, form and counts exactly as they were.  Ring: N = 2^11, 64-dim vectors (1024 slots, 64
ciphertexts per block, 45- and 46-bit limbs), the sizes of tests/test_gpu_db_update.py."""
import ctypes as C

import numpy as np
import pytest
import torch  # (imported before the library is loaded: torch and libhydia.so then share one HIP runtime in the process)

import db_delta_ref as DR
import oracle_lib as O
import wire_ref as WR
from db_update_ref import DB_NONCE_BASE, UpdateRef, saturated_ct

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def bare_ctx(im):
    return im.Context(im.default_params(log_n=11, vector_dim=64), 0)


@pytest.fixture(scope="module")
def small(im):
    """the fully keyed context: the twin that runs hydia_db_update, and the sender of the end-to-end test"""
    P = O.Params(log_n=11, depth=11, dim=64)
    K = O.Keys(P, 7)
    cc = bare_ctx(im)
    cc.keygen(7)
    yield P, K, O.Oracle(P, K), cc
    cc.close()


@pytest.fixture(scope="module")
def enr(im, small):
    """the enroller's context: the receiver's PUBLIC key, imported, and nothing else"""
    c = bare_ctx(im)
    c.import_public_key(small[3].export_public_key())
    yield c
    c.close()


@pytest.fixture(scope="module")
def snd(im, small):
    """the sender's context.  A delta needs no key on it; the public key is there only so that the tests can enrol its first database
    with the twin's arguments"""
    c = bare_ctx(im)
    c.import_public_key(small[3].export_public_key())
    yield c
    c.close()


@pytest.fixture(scope="module")
def rows10(small):
    """10 blocks - 3 rows of random templates (shared, never modified): tests/test_gpu_db_update.py's"""
    P = small[0]
    n = 10 * P.slots - 3
    rng = np.random.default_rng(2025)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for i in (5, 8 * P.slots + 100, n - 1):
        db[i] = rng.integers(1, 4, size=P.dim)
    db.setflags(write=False)
    return db


@pytest.fixture(scope="module")
def enrolled10(small, rows10):
    """the oracle's hoisted enrolment of rows10 with seed 41 (shared: UpdateRef.fork() never modifies a ciphertext in place)"""
    P, K, Or, cc = small
    return UpdateRef(P, Or).enroll(rows10.copy(), 41)


def moduli(P):
    return [int(q) for q in P.moduli[:P.nQ]]


def oracle_blocks(P, Or, B, first_vector, rows, normalise, seed, first_block=0):
    """the specification of hydia_db_delta_make on the oracle: per touched block the fresh encryptions E of the sparse diagonal image
    of `rows` (normalised in place when asked), [dim][2][n_q][N] each"""
    U = UpdateRef(P, Or, babies=B)
    n = rows.shape[0]
    if normalise:
        for v in range(n):
            P.L.hyo_normalize(O._ptr(rows[v]), P.dim)
    touched = DR.touched_blocks(first_vector, n, P.slots)
    Z = np.zeros(((touched[-1] + 1) * P.slots, P.dim), dtype=np.float64)
    Z[first_vector:first_vector + n] = rows
    out = []
    for g in touched:
        cts = [Or.encrypt(U.image(Z, g * P.dim + i), seed, DB_NONCE_BASE + (first_block + g) * P.dim + i) for i in range(P.dim)]
        assert all(c.scale == P.delta and c.nl == P.nQ for c in cts)
        out.append(np.stack([c.data().copy() for c in cts]))
    return out


def expected_delta(P, Or, B, first_vector, rows, normalise, seed, first_block=0):
    blocks = oracle_blocks(P, Or, B, first_vector, rows, normalise, seed, first_block)
    return DR.build(blocks, moduli(P), P.delta, B, first_vector, rows.shape[0], first_block)


def form(c):
    return c.db_stats(), c.db_kind(), c.db_babies(), c.db_group(), c.db_residue_bits()


def snapshot(c, ts):
    return form(c), [c.db_export_ct(t) for t in ts]


def unchanged(c, ts, before):
    after = snapshot(c, ts)
    return after[0] == before[0] and all(np.array_equal(a, b) for a, b in zip(after[1], before[1]))


def same3(snd, twin, ref, ts):
    """the sender after the delta, the twin after hydia_db_update and the oracle agree bit for bit"""
    for t in ts:
        got = snd.db_export_ct(t)
        assert np.array_equal(got, twin.db_export_ct(t)), t
        assert np.array_equal(got, ref.cts[t].data()), t
    assert form(snd) == form(twin)


def block(P, g):
    return range(g * P.dim, (g + 1) * P.dim)


def enrol_both(im, snd, twin, rows, seed, matvec):
    for c in (snd, twin):
        c.set_matvec(matvec)
        try:
            im.DiagonalEnroller(c, rows.shape[0]).serializeDB(rows.copy(), seed=seed)
        finally:
            c.set_matvec("auto")


def update_both(enr, snd, twin, ref, first, rows, normalise, seed, B=None):
    """the update three ways; returns the ciphertexts it touches"""
    a, b, c = rows.copy(), rows.copy(), rows.copy()
    touched = ref.update(first, a, 1 if normalise else 0, seed)
    twin.db_update(first, b, normalise, seed=seed)
    message = enr.db_delta_make(first, c, normalise, seed=seed, babies=B)
    assert np.array_equal(a, b) and np.array_equal(b, c)  # all three normalise the rows in place alike
    assert len(message) == enr.db_delta_bytes(first, rows.shape[0])
    snd.db_delta_apply(message)
    return touched


# ------------------------------------------------------------------------------------------------ bytes
def test_bytes_from_a_public_key_alone(im, small, enr):
    """rows that straddle blocks 1 and 2, with a nonce offset: the container built in Python from the oracle's E, byte for byte; the
    same bytes from a fully keyed context with a database resident (which stays what it was) and from the rows in device memory"""
    P, K, Or, cc = small
    rng = np.random.default_rng(11)
    rows = rng.integers(-99, 100, size=(30, P.dim)).astype(np.float64)
    first = 2 * P.slots - 7
    a, b, c = rows.copy(), rows.copy(), rows.copy()
    want = expected_delta(P, Or, P.dim, first, a, True, 70, first_block=3)
    assert enr.db_kind() == 0
    got = enr.db_delta_make(first, b, True, seed=70, first_block=3)
    assert np.array_equal(a, b) and not np.array_equal(b, rows)  # normalised in place, as the oracle normalises
    assert len(got) == len(want) == enr.db_delta_bytes(first, 30) == DR.total_bytes(P.N, P.dim, moduli(P), first, 30)
    assert got == want
    assert im.db_delta_peek(got) == dict(version=1, vector_dim=P.dim, babies=P.dim, first_vector=first, n_rows=30, first_block=3, n_blocks=2,
                                         total_bytes=len(want))
    assert enr.db_kind() == 0 and enr.db_stats()[:2] == (0, 0)  # making a delta allocates no database
    # a fully keyed context with a database resident: the same bytes, the database neither read nor written
    cc.db_fill_random(3 * P.slots, 9)
    ts = (0, 2 * P.dim - 1, 2 * P.dim, 3 * P.dim - 1)
    before = snapshot(cc, ts)
    assert cc.db_delta_make(first, c, True, seed=70, first_block=3) == want
    assert unchanged(cc, ts, before)
    # rows in device memory: never written, the same bytes for the same float64 rows
    t = torch.tensor(rows, dtype=torch.float64, device="cuda:0")
    keep = t.clone()
    assert enr.db_delta_make(first, t, True, seed=70, first_block=3) == want
    assert torch.equal(t, keep)
    # the pre-rotated form and rows taken as given
    a = rows * 0.01
    want8 = expected_delta(P, Or, 8, 5, a.copy(), False, 71)
    assert enr.db_delta_make(5, a, False, seed=71, babies=8) == want8
    assert enr.db_delta_make(5, torch.tensor(a, dtype=torch.float64, device="cuda:0"), False, seed=71, babies=8) == want8
    # the size is host arithmetic
    for fv, n in ((0, 1), (0, P.slots), (0, P.slots + 1), (P.slots - 1, 2), (5 * P.slots + 1, 3 * P.slots)):
        assert enr.db_delta_bytes(fv, n) == DR.total_bytes(P.N, P.dim, moduli(P), fv, n)
    for fv, n in ((0, 0), ((1 << 64) - 1, 1), (0, (1 << 64) - 1)):
        with pytest.raises(im.HydiaError) as e:
            enr.db_delta_bytes(fv, n)
        assert e.value.code == ERR_ARG


# ------------------------------------------------------------------------------------------------ apply equals update
def test_append_across_a_block_edge(im, small, enr, snd):
    """ciphertext-major, 48-bit, one block: + 30 rows at 1000 fill block 0 and open block 1 (one block added to, one created)"""
    P, K, Or, cc = small
    rng = np.random.default_rng(1)
    db = rng.integers(-99, 100, size=(1000 + 30 + 1200, P.dim)).astype(np.float64)
    enrol_both(im, snd, cc, db[:1000], 41, "hoisted")
    ref = UpdateRef(P, Or).enroll(db[:1000].copy(), 41)
    assert form(snd) == form(cc) and snd.db_kind() == 5 and snd.db_group() == 0 and snd.db_residue_bits() == 48
    touched = update_both(enr, snd, cc, ref, 1000, db[1000:1030], True, 42)
    assert touched == list(range(2 * P.dim)) and snd.db_stats()[:2] == (1030, 2 * P.dim)
    same3(snd, cc, ref, touched)
    touched = update_both(enr, snd, cc, ref, 1030, db[1030:], True, 43)  # blocks 1 (exists now) and 2 (new)
    assert touched == list(range(P.dim, 3 * P.dim)) and snd.db_stats()[:2] == (2230, 3 * P.dim)
    same3(snd, cc, ref, touched)
    same3(snd, cc, ref, (0, P.dim // 2, P.dim - 1))  # block 0 was not touched again


def test_remove_and_replace(im, small, enr, snd):
    """remove by the negated row (normalise = 1) and replace by new - old with normalise = 0, both in block 0 of two"""
    P, K, Or, cc = small
    rng = np.random.default_rng(2)
    n = 1500
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    gallery = db / np.linalg.norm(db, axis=1, keepdims=True)
    enrol_both(im, snd, cc, db, 41, "hoisted")
    ref = UpdateRef(P, Or).enroll(db.copy(), 41)
    touched = update_both(enr, snd, cc, ref, 700, -gallery[700:701], True, 50)
    assert touched == list(block(P, 0))
    same3(snd, cc, ref, touched)
    new = np.where(np.arange(P.dim) % 2 == 0, 1.0, -1.0)
    new /= np.linalg.norm(new)
    update_both(enr, snd, cc, ref, 300, (new - gallery[300])[None, :], False, 52)
    same3(snd, cc, ref, block(P, 0))
    same3(snd, cc, ref, (P.dim, 2 * P.dim - 1))  # block 1 was never touched
    assert snd.db_stats()[:2] == (n, 2 * P.dim)


@pytest.mark.parametrize("env,bits,group", [({}, 46, 2), ({"HYDIA_DB_48BIT": "1"}, 48, 2), ({"HYDIA_DB_UNPACKED": "1"}, 64, 0)])
def test_inside_a_ten_block_database(im, small, enr, snd, rows10, enrolled10, env, bits, group, monkeypatch):
    """10 blocks; rows that straddle the edge between blocks 3 and 4: the 46-bit granules of the group-sequential layout, 6-byte
    residues under HYDIA_DB_48BIT and 8-byte residues under HYDIA_DB_UNPACKED (contexts of their own: the layout is fixed by the
    context that allocates the database)"""
    P, K, Or, cc = small
    own = []
    twin = cc
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pk = cc.export_public_key()
        for _ in range(2):
            c = bare_ctx(im)
            c.import_public_key(pk)
            own.append(c)
        snd, twin = own
        for k in env:
            monkeypatch.delenv(k)
    try:
        n = rows10.shape[0]
        rng = np.random.default_rng(4)
        ref = enrolled10.fork()
        enrol_both(im, snd, twin, rows10, 41, "hoisted")
        assert form(snd) == form(twin) and snd.db_group() == group and snd.db_residue_bits() == bits and snd.db_kind() == 5
        first = 4 * P.slots - 10
        rows = rng.integers(-99, 100, size=(25, P.dim)).astype(np.float64)
        touched = update_both(enr, snd, twin, ref, first, rows, True, 90)
        assert touched == list(range(3 * P.dim, 5 * P.dim))
        update_both(enr, snd, twin, ref, first + 9, rng.uniform(-0.1, 0.1, size=(3, P.dim)), False, 91)
        assert snd.db_group() == group and snd.db_residue_bits() == bits and snd.db_stats()[:2] == (n, 10 * P.dim)
        same3(snd, twin, ref, touched)
        same3(snd, twin, ref, (0, 2 * P.dim + 31, 3 * P.dim - 1, 5 * P.dim, 10 * P.dim - 1))  # the neighbours and the ends: untouched
    finally:
        for c in own:
            c.close()


def test_growth_across_the_layout_change(im, small, enr, snd, rows10):
    """hoisted, 8 blocks (ciphertext-major, 48-bit) + a delta to 10 blocks - 3 rows: db_grow moves the database to the group-sequential
    46-bit layout, block 7 is added to and blocks 8 and 9 are created in the NEW layout"""
    P, K, Or, cc = small
    n0, n1 = 8 * P.slots - 5, rows10.shape[0]
    enrol_both(im, snd, cc, rows10[:n0], 41, "hoisted")
    ref = UpdateRef(P, Or).enroll(rows10[:n0].copy(), 41)
    assert snd.db_group() == 0 and snd.db_residue_bits() == 48 and snd.db_stats()[:2] == (n0, 8 * P.dim)
    touched = update_both(enr, snd, cc, ref, n0, rows10[n0:], True, 77)
    assert touched == list(range(7 * P.dim, 10 * P.dim))
    assert snd.db_group() == 2 and snd.db_residue_bits() == 46 and snd.db_kind() == 5 and snd.db_stats()[:2] == (n1, 10 * P.dim)
    same3(snd, cc, ref, touched)
    same3(snd, cc, ref, (0, P.dim + 7, 4 * P.dim, 7 * P.dim - 1))  # moved by db_grow, not touched by the delta


def test_pre_rotated_form(im, small, enr, snd):
    """set_matvec(8), kind 6: a delta that opens block 1 (the database becomes group-sequential) and one inside block 0; the delta
    declares babies = 8"""
    P, K, Or, cc = small
    rng = np.random.default_rng(7)
    n0, extra = 1000, 100
    db = rng.integers(-99, 100, size=(n0 + extra, P.dim)).astype(np.float64)
    enrol_both(im, snd, cc, db[:n0], 41, 8)
    ref = UpdateRef(P, Or, babies=8).enroll(db[:n0].copy(), 41)
    assert snd.db_kind() == 6 and snd.db_babies() == 8 and snd.db_group() == 0
    touched = update_both(enr, snd, cc, ref, n0, db[n0:], True, 42, B=8)
    assert touched == list(range(2 * P.dim)) and snd.db_kind() == 6 and snd.db_babies() == 8 and snd.db_group() > 0
    same3(snd, cc, ref, touched)
    touched = update_both(enr, snd, cc, ref, 10, rng.integers(-99, 100, size=(3, P.dim)).astype(np.float64), True, 43, B=8)
    assert touched == list(block(P, 0))
    same3(snd, cc, ref, range(2 * P.dim))


# ------------------------------------------------------------------------------------------------ enrol from nothing
@pytest.mark.parametrize("matvec,B,first_block", [("hoisted", 64, 0), (8, 8, 3)])
def test_enrol_from_nothing(im, small, enr, matvec, B, first_block):
    """ONE two-block delta with first_vector = 0 on an empty context that holds no key at all: bit for bit hydia_db_enroll_shard_ex of
    the same rows, seed, first_block and form — and, block by block through the roles, serializeDBToWire / applyDBWire"""
    P, K, Or, cc = small
    rng = np.random.default_rng(12)
    n = P.slots + 476
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    a, b, c = db.copy(), db.copy(), db.copy()
    im.DiagonalEnroller(cc, n).serializeDB(a, seed=61, first_block=first_block, matvec=matvec)
    want = [cc.db_export_ct(t) for t in range(2 * P.dim)]
    assert cc.db_kind() == (5 if B == P.dim else 6) and cc.db_babies() == B
    if first_block == 0:  # the oracle's own enrolment
        ref = UpdateRef(P, Or, babies=B).enroll(db.copy(), 61)
        for t in (0, P.dim - 1, P.dim, 2 * P.dim - 1):
            assert np.array_equal(want[t], ref.cts[t].data()), t
    empty = bare_ctx(im)
    try:
        assert empty.db_kind() == 0
        message = enr.db_delta_make(0, b, True, seed=61, babies=B, first_block=first_block)
        assert np.array_equal(a, b) and im.db_delta_peek(message)["n_blocks"] == 2
        empty.db_delta_apply(message)
        assert form(empty) == form(cc) and empty.db_stats()[:2] == (n, 2 * P.dim)
        for t in range(2 * P.dim):
            assert np.array_equal(empty.db_export_ct(t), want[t]), t
    finally:
        empty.close()
    empty = bare_ctx(im)
    try:
        sender = im.DiagonalSender(empty, 0)
        counts = [sender.applyDBWire(m) for m in im.DiagonalEnroller(enr, 0).serializeDBToWire(c, seed=61, babies=B, first_block=first_block)]
        assert counts == [P.slots, n] and sender.numVectors == n and np.array_equal(a, c)
        assert form(empty) == form(cc)
        for t in (0, P.dim - 1, P.dim, P.dim + 9, 2 * P.dim - 1):
            assert np.array_equal(empty.db_export_ct(t), want[t]), t
    finally:
        empty.close()


# ------------------------------------------------------------------------------------------------ saturated residues
def saturated_message(P):
    """a type 1 message of vector_dim ciphertexts whose every residue is q_j - 1, through wire_ref's own pack_row and header"""
    mods = moduli(P)
    poly = b"".join(WR.pack_row(np.full(P.N, q - 1, dtype=np.uint64), WR.width(q)) for q in mods)
    return WR.header(WR.CT_BATCH, P.log_n, P.dim, 2, mods, scale=P.delta) + poly * (2 * P.dim)


@pytest.mark.parametrize("blocks,bits", [(1, 48), (10, 46)])
def test_saturated_residues(im, small, snd, blocks, bits):
    """q_j - 1 in every residue of the delta, added to ciphertexts whose every residue is q_j - 1: q_j - 2 everywhere — the sum is
    reduced before it is packed, in the 6-byte fields and in the 46-bit ones (where an unreduced sum carries into the neighbour)"""
    P, K, Or, cc = small
    n = blocks * P.slots - 3
    sat = saturated_ct(P, Or)
    first = 500 if blocks == 1 else 4 * P.slots - 10
    touched_blocks = DR.touched_blocks(first, 25, P.slots)
    assert touched_blocks == ([0] if blocks == 1 else [3, 4])
    snd.db_alloc(n)
    assert snd.db_kind() == 5 and snd.db_residue_bits() == bits and snd.db_group() == (0 if blocks == 1 else 2)
    for g in touched_blocks:
        for t in block(P, g):
            snd.db_import_ct(t, sat.data())
    one = saturated_message(P)
    h, rows = WR.unpack_message(one)
    assert all((rows[:, :, j] == np.uint64(q - 1)).all() for j, q in enumerate(moduli(P)))
    snd.db_delta_apply(DR.container(P.dim, P.dim, first, 25, 0, [one] * len(touched_blocks)))
    want = sat.data().copy()
    for j, q in enumerate(moduli(P)):
        want[:, j, :] = np.uint64(q - 2)
    for g in touched_blocks:
        for t in block(P, g):
            assert np.array_equal(snd.db_export_ct(t), want), t
    assert snd.db_stats()[:2] == (n, blocks * P.dim) and snd.db_residue_bits() == bits


# ------------------------------------------------------------------------------------------------ refusals
def apply_code(c, data):
    raw = np.frombuffer(b"" if data is None else bytes(data), dtype=np.uint8)
    return c.L.hydia_db_delta_apply(c.h, raw.ctypes.data_as(C.c_void_p) if raw.size else None, raw.size)


def refused(c, data, code, ts, before, word=None):
    assert apply_code(c, data) == code
    if word is not None:
        assert word in c.L.hydia_last_error().decode(), (word, c.L.hydia_last_error().decode())
    assert unchanged(c, ts, before)


def test_refused_deltas_change_nothing(im, small, enr, snd):
    P, K, Or, cc = small
    rng = np.random.default_rng(9)
    n = 1500
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    snd.set_matvec("hoisted")
    try:
        im.DiagonalEnroller(snd, n).serializeDB(db.copy(), seed=3)
    finally:
        snd.set_matvec("auto")
    ts = (0, P.dim - 1, P.dim, 2 * P.dim - 1)
    before = snapshot(snd, ts)
    rows = rng.integers(-99, 100, size=(30, P.dim)).astype(np.float64)
    first = P.slots - 10
    good = enr.db_delta_make(first, rows.copy(), True, seed=5)  # blocks 0 and 1, both resident
    hdr, messages = DR.split(good)
    assert hdr["n_blocks"] == 2
    mods = moduli(P)
    # ONE bad residue (= q_j): the last residue of the last limb of the last ciphertext of the second block.  Block 0 passed its check
    # before it was seen, and nothing of block 0 may have been added
    w, q = WR.width(mods[-1]), mods[-1]
    tail = int.from_bytes(good[-8:], "little")
    bad = good[:-8] + ((tail & ((1 << (64 - w)) - 1)) | (q << (64 - w))).to_bytes(8, "little")
    _, bad_rows = WR.unpack_message(DR.split(bad)[1][1])
    _, good_rows = WR.unpack_message(messages[1])
    diff = np.argwhere(bad_rows != good_rows)
    assert diff.tolist() == [[P.dim - 1, 1, P.nQ - 1, P.N - 1]] and int(bad_rows[-1, -1, -1, -1]) == q
    refused(snd, bad, ERR_ARG, ts, before, "at or above its modulus")
    # the container
    refused(snd, good[:-1], ERR_ARG, ts, before, "truncated")
    refused(snd, good[:DR.HEADER_BYTES + len(messages[0])], ERR_ARG, ts, before, "truncated")
    refused(snd, good[:40], ERR_ARG, ts, before, "len")
    refused(snd, good + b"\0", ERR_ARG, ts, before, "bytes after the last message")
    refused(snd, b"HYDDELT2" + good[8:], ERR_ARG, ts, before, "magic")

    def delta(msgs=messages, **over):
        return DR.container(**{**dict(vector_dim=P.dim, babies=P.dim, first_vector=first, n_rows=30, first_block=0, messages=msgs), **over})

    assert delta() == good
    refused(snd, delta(version=2), ERR_ARG, ts, before, "version")
    refused(snd, delta(reserved=1), ERR_ARG, ts, before, "reserved")
    refused(snd, delta(n_rows=5), ERR_ARG, ts, before, "n_blocks")            # the rows touch one block, two messages follow
    refused(snd, delta(n_blocks=1), ERR_ARG, ts, before, "n_blocks")
    refused(snd, delta(n_rows=0), ERR_ARG, ts, before, "n_rows")
    refused(snd, delta(msgs=messages[:1]), ERR_ARG, ts, before, "n_blocks")
    refused(snd, delta(vector_dim=32, babies=32), ERR_ARG, ts, before, "vector_dim")
    # a message of another shape (headers alone are read: the payloads are zeros of the length each header implies)
    def zeros(**over):
        args = {**dict(mtype=WR.CT_BATCH, log_n=P.log_n, count=P.dim, n_polys=2, moduli=mods, scale=P.delta), **over}
        head = WR.header(**args)
        return head + bytes(WR.parse_header(head)["payload_bytes"])

    assert apply_code(snd, delta(msgs=[zeros(), zeros()])) == 0  # (zeros are canonical: E = 0 changes no residue)
    assert unchanged(snd, ts, before)
    refused(snd, delta(msgs=[messages[0], zeros(count=P.dim + 1)]), ERR_ARG, ts, before, "count is not vector_dim")
    refused(snd, delta(msgs=[messages[0], zeros(moduli=mods[:-1])]), ERR_ARG, ts, before, "n_limbs is not n_q")
    refused(snd, delta(msgs=[zeros(n_polys=3), messages[1]]), ERR_ARG, ts, before, "n_polys is not 2")
    refused(snd, delta(msgs=[messages[0], zeros(scale=P.delta * 2)]), ERR_ARG, ts, before, "scale")
    refused(snd, delta(msgs=[messages[0], zeros(log_n=12)]), ERR_ARG, ts, before, "log_n")
    # the target
    refused(snd, enr.db_delta_make(first, rows.copy(), True, seed=5, babies=8), ERR_ARG, ts, before, "babies")
    refused(snd, enr.db_delta_make(n + 1, rows.copy(), True, seed=5), ERR_ARG, ts, before, "first_vector")
    assert apply_code(snd, None) == ERR_ARG and unchanged(snd, ts, before)
    # ... and the good delta still applies afterwards
    assert apply_code(snd, good) == 0 and snd.db_stats()[:2] == (n, 2 * P.dim) and not unchanged(snd, ts, before)


def test_refused_targets_and_makers(im, small, enr, snd):
    P, K, Or, cc = small
    rng = np.random.default_rng(10)
    n = 300
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    rows = rng.integers(-99, 100, size=(4, P.dim)).astype(np.float64)
    good = enr.db_delta_make(0, rows.copy(), True, seed=5)
    later = enr.db_delta_make(7, rows.copy(), True, seed=5)
    # nothing resident and a nonzero first_vector; no key is needed to find that out
    empty = bare_ctx(im)
    try:
        assert apply_code(empty, later) == ERR_STATE and "first_vector = 0" in empty.L.hydia_last_error().decode()
        assert empty.db_kind() == 0 and empty.db_stats()[:2] == (0, 0)
        # make without a public key
        with pytest.raises(im.HydiaError) as e:
            empty.db_delta_make(0, rows.copy(), True, seed=5)
        assert e.value.code == ERR_STATE and "public key" in str(e.value)
    finally:
        empty.close()
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
    # the maker's arguments: nothing is written, not even the length of a refused call's message
    L = enr.L
    seed = np.frombuffer((5).to_bytes(32, "little"), dtype=np.uint8).copy()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    need = enr.db_delta_bytes(0, 4)
    buf = np.full(need + 16, 0xA5, dtype=np.uint8)

    def make(r, cnt, babies, cap, sd=seed, b=buf):
        ln = C.c_size_t(77)
        code = L.hydia_db_delta_make(enr.h, 0, None if r is None else vp(r), cnt, 1, None if sd is None else vp(sd), babies, 0,
                                     None if b is None else vp(b), cap, C.byref(ln))
        return code, ln.value

    keep = rows.copy()
    for babies in (0, 1, 3, 48, 128, -8):
        assert make(keep, 4, babies, buf.size) == (ERR_ARG, 0), babies
    assert make(keep, 0, P.dim, buf.size) == (ERR_ARG, 0)
    assert make(None, 4, P.dim, buf.size)[0] == ERR_ARG and make(keep, 4, P.dim, buf.size, sd=None) == (ERR_ARG, 0)
    assert make(keep, 4, P.dim, need - 1) == (ERR_ARG, need) and make(keep, 4, P.dim, need, b=None) == (ERR_ARG, need)
    assert (buf == 0xA5).all() and np.array_equal(keep, rows)  # nothing written, the rows not normalised by a refused call
    assert L.hydia_db_delta_make(enr.h, 0, vp(keep), 4, 1, vp(seed), P.dim, 0, vp(buf), buf.size, None) == ERR_ARG
    # the nonce space: first_block + blocks beyond 2^40 nonces
    assert L.hydia_db_delta_make(enr.h, 0, vp(keep), 4, 1, vp(seed), P.dim, (1 << 40) // P.dim, vp(buf), buf.size, C.byref(C.c_size_t())) == ERR_ARG
    assert (buf == 0xA5).all()
    assert make(keep, 4, P.dim, need) == (0, need) and bytes(buf[:need]) == good and (buf[need:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ end to end
def test_a_match_appended_by_delta_is_found(im, small, enr):
    """the three roles as three parties: the receiver's keys on `cc` (which is also the sender here: it holds the evaluation keys and
    the database), the enroller on a context with the public key alone.  A planted match appended by delta is found at its index"""
    P, K, Or, cc = small
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
    enroller = im.DiagonalEnroller(enr, n0)
    message = enroller.appendToWire(db[n0:].copy(), sender.numVectors, seed=42, babies=cc.db_babies())
    assert enroller.numVectors == n0 + 40
    assert sender.applyDBWire(message) == n0 + 40 == sender.numVectors == cc.db_stats()[0]
    receiver = im.DiagonalReceiver(cc, n0 + 40)  # rebuilt for the new vector count
    assert n0 + 30 in receiver.decryptIndex(sender.indexScenario(qc))
