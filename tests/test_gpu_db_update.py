"""In-place update of the resident database on the GPU (hydia_db_update; run with -m gpu): append, remove, replace, growth across
the layout change, updates inside a group-sequential 46-bit database, saturated residues, the pre-rotated form, the shard
equivalence, the refused calls and a growth that does not fit in device memory.  Every comparison of ciphertexts is np.array_equal of db_export_ct against the restatement of the
semantics on the CPU oracle (tests/db_update_ref.py) — bit for bit, never against the product itself.  Ring: N = 2^11, 64-dim
vectors (1024 slots, 64 ciphertexts per block), as in tests/test_gpu_client.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from db_update_ref import UpdateRef, saturated_ct

pytestmark = pytest.mark.gpu
TOL = 1e-4
ERR_ARG, ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def make_ctx(im):
    cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    cc.keygen(7)
    return cc


@pytest.fixture(scope="module")
def small(im):
    P = O.Params(log_n=11, depth=11, dim=64)
    K = O.Keys(P, 7)
    cc = make_ctx(im)
    yield P, K, O.Oracle(P, K), cc
    cc.close()


@pytest.fixture(scope="module")
def rows10(small):
    """10 blocks - 3 rows of random templates with a few planted matches of the all-ones query (shared, never modified)"""
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


def same(cc, ref, ts):
    for t in ts:
        assert np.array_equal(cc.db_export_ct(t), ref.cts[t].data()), t


def block(P, g):
    return range(g * P.dim, (g + 1) * P.dim)


def test_append_across_a_block_edge(im, small):
    """ciphertext-major, 48-bit: 1000 rows, + 24 (fills block 0 exactly), + 1 (opens block 1 with a single row), + 1500"""
    P, K, Or, cc = small
    rng = np.random.default_rng(1)
    total = 1000 + 24 + 1 + 1500
    db = rng.integers(-99, 100, size=(total, P.dim)).astype(np.float64)
    planted = [3, 1010, 1024, 2000]  # one enrolled, one in each appended batch
    for i in planted:
        db[i] = rng.integers(1, 4, size=P.dim)
    cc.set_matvec("hoisted")
    try:
        a, b = db[:1000].copy(), db[:1000].copy()
        ref = UpdateRef(P, Or).enroll(a, 41)
        enr = im.DiagonalEnroller(cc, 1000)
        enr.serializeDB(b, seed=41)
        assert cc.db_kind() == 5 and cc.db_group() == 0 and cc.db_residue_bits() == 48
        lo = 1000
        for step, (cnt, seed) in enumerate([(24, 42), (1, 43), (1500, 44)]):
            a, b = db[lo:lo + cnt].copy(), db[lo:lo + cnt].copy()
            touched = ref.update(lo, a, 1, seed)
            enr.appendDB(b, seed=seed)
            assert np.array_equal(a, b)  # both normalise the rows in place
            lo += cnt
            assert cc.db_stats()[:2] == (lo, len(ref.cts)) and enr.numVectors == lo
            assert len(ref.cts) == [64, 128, 192][step]
            same(cc, ref, touched)
            if step > 0:  # block 0 is no longer touched
                same(cc, ref, (0, P.dim // 2, P.dim - 1))
        assert cc.db_kind() == 5 and cc.db_babies() == P.dim and cc.db_group() == 0
        query = np.ones(P.dim)
        q = Or.encrypt_query(query, 5, 1)
        gq = cc.import_ct(q.data(), q.scale)
        sender, receiver = im.DiagonalSender(cc, lo), im.DiagonalReceiver(cc, lo)  # rebuilt for the new vector count
        want = Or.compute_similarity(q, ref.array(), lo)
        got = sender.computeSimilarity(gq).export()
        assert len(want) == 3
        for g in range(3):
            assert np.array_equal(got[g], want[g].data()), g
        assert set(planted) <= set(receiver.decryptIndex(sender.indexScenario(gq)))
    finally:
        cc.set_matvec("auto")


def test_remove_and_replace(im, small):
    """three updates of block 0: a removal (the negated template), a replacement by a matching template and a replacement of a
    matching template by another one (new - old, normalise = 0)"""
    P, K, Or, cc = small
    rng = np.random.default_rng(2)
    n = 1500
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for i in (300, 700, 1100):
        db[i] = rng.integers(1, 4, size=P.dim)
    gallery = db / np.linalg.norm(db, axis=1, keepdims=True)
    query = np.ones(P.dim)
    qn = query / np.linalg.norm(query)
    cc.set_matvec("hoisted")
    try:
        ref = UpdateRef(P, Or).enroll(db.copy(), 41)
        enr = im.DiagonalEnroller(cc, n)
        enr.serializeDB(db.copy(), seed=41)
        sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
        qc = receiver.encryptQuery(query, seed=5, nonce=1)
        assert {300, 700, 1100} <= set(receiver.decryptIndex(sender.indexScenario(qc)))
        # removal
        neg = -gallery[700:701]
        touched = ref.update(700, neg.copy(), 1, 50)
        enr.updateRows(700, neg.copy(), True, seed=50)
        same(cc, ref, touched)
        gallery[700] = 0.0
        scores = cc.decrypt(sender.computeSimilarity(qc)).reshape(-1)
        assert abs(scores[700]) < TOL
        assert np.abs(scores[:n] - gallery @ qn).max() < TOL
        hits = receiver.decryptIndex(sender.indexScenario(qc))
        assert 700 not in hits and {300, 1100} <= set(hits)
        # replacements: 9 becomes a matching template, 300 stops being one
        for idx, new, seed in ((9, rng.integers(1, 4, size=P.dim).astype(np.float64), 51),
                               (300, np.where(np.arange(P.dim) % 2 == 0, 1.0, -1.0), 52)):
            new = new / np.linalg.norm(new)
            delta = (new - gallery[idx])[None, :].copy()
            ref.update(idx, delta.copy(), 0, seed)
            enr.updateRows(idx, delta, False, seed=seed)
            gallery[idx] = new
        same(cc, ref, block(P, 0))                     # after three updates of one block
        same(cc, ref, (P.dim, 2 * P.dim - 1))          # block 1 was never touched
        assert cc.db_stats()[:2] == (n, 2 * P.dim) and enr.numVectors == n
        scores = cc.decrypt(sender.computeSimilarity(qc)).reshape(-1)
        assert np.abs(scores[:n] - gallery @ qn).max() < TOL
        hits = receiver.decryptIndex(sender.indexScenario(qc))
        assert {9, 1100} <= set(hits) and 300 not in hits and 700 not in hits
    finally:
        cc.set_matvec("auto")


def test_growth_across_the_layout_change(im, small, rows10, enrolled10, tmp_path):
    """hoisted, 8 blocks (ciphertext-major, 48-bit) + an append to 10 blocks - 3 rows: the database moves to the group-sequential
    46-bit layout; every ciphertext equals the expected one, and the file round-trips"""
    P, K, Or, cc = small
    n0, n1 = 8 * P.slots - 5, rows10.shape[0]
    cc.set_matvec("hoisted")
    try:
        # blocks 0..6 are those of the 10-block enrolment; the ragged block 7 is its own
        ref = UpdateRef(P, Or).enroll(rows10[:n0].copy(), 41)
        for t in (0, 7 * P.dim - 1):
            assert np.array_equal(ref.cts[t].data(), enrolled10.cts[t].data())
        enr = im.DiagonalEnroller(cc, n0)
        enr.serializeDB(rows10[:n0].copy(), seed=41)
        assert cc.db_group() == 0 and cc.db_residue_bits() == 48 and cc.db_stats()[:2] == (n0, 8 * P.dim)
        touched = ref.update(n0, rows10[n0:].copy(), 1, 77)
        assert touched == list(range(7 * P.dim, 10 * P.dim))
        enr.appendDB(rows10[n0:].copy(), seed=77)
        assert cc.db_group() == 2 and cc.db_residue_bits() == 46 and cc.db_kind() == 5
        assert cc.db_stats()[:2] == (n1, 10 * P.dim)
        same(cc, ref, range(10 * P.dim))
        path = str(tmp_path / "grown.bin")
        cc.db_save(path)
        cc.db_fill_random(3 * P.slots, 1)  # something else resident in between
        cc.db_load(path)
        assert cc.db_group() == 2 and cc.db_stats()[:2] == (n1, 10 * P.dim) and cc.db_kind() == 5
        same(cc, ref, (0, P.dim, 7 * P.dim + 3, 8 * P.dim, 10 * P.dim - 1))
        # the grown database answers queries: the planted matches, one of them in an appended block
        query = np.ones(P.dim)
        q = Or.encrypt_query(query, 5, 1)
        gq = cc.import_ct(q.data(), q.scale)
        sender = im.DiagonalSender(cc, n1)
        assert {5, 8 * P.slots + 100, n1 - 1} <= set(im.DiagonalReceiver(cc, n1).decryptIndex(sender.indexScenario(gq)))
        want = Or.compute_similarity(q, ref.array(), n1)
        got = sender.computeSimilarity(gq).export()
        for g in (0, 7, 9):
            assert np.array_equal(got[g], want[g].data()), g
    finally:
        cc.set_matvec("auto")


@pytest.mark.parametrize("env,bits", [({}, 46), ({"HYDIA_DB_48BIT": "1"}, 48)])
def test_update_inside_a_group_sequential_database(im, small, rows10, enrolled10, env, bits, monkeypatch):
    """10 blocks, group-sequential; rows that straddle the edge between blocks 3 and 4 (46-bit granules, and 6-byte residues under
    HYDIA_DB_48BIT in a context of its own: the layout is fixed by the context that allocates the database)"""
    P, K, Or, cc = small
    own = None
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cc = own = make_ctx(im)
        for k in env:
            monkeypatch.delenv(k)
    n = rows10.shape[0]
    rng = np.random.default_rng(4)
    cc.set_matvec("hoisted")
    try:
        ref = enrolled10.fork()
        enr = im.DiagonalEnroller(cc, n)
        enr.serializeDB(rows10.copy(), seed=41)
        assert cc.db_group() == 2 and cc.db_residue_bits() == bits
        first = 4 * P.slots - 10
        rows = rng.integers(-99, 100, size=(25, P.dim)).astype(np.float64)
        touched = ref.update(first, rows.copy(), 1, 90)
        assert touched == list(range(3 * P.dim, 5 * P.dim))
        enr.updateRows(first, rows.copy(), True, seed=90)
        delta = rng.uniform(-0.1, 0.1, size=(3, P.dim))
        ref.update(first + 9, delta.copy(), 0, 91)
        enr.updateRows(first + 9, delta.copy(), False, seed=91)
        assert cc.db_group() == 2 and cc.db_residue_bits() == bits and cc.db_stats()[:2] == (n, 10 * P.dim)
        same(cc, ref, touched)
        same(cc, ref, (0, 2 * P.dim + 31, 3 * P.dim - 1, 5 * P.dim, 10 * P.dim - 1))  # the neighbours and the ends: untouched
    finally:
        cc.set_matvec("auto")
        if own is not None:
            own.close()


@pytest.mark.parametrize("blocks,bits", [(1, 48), (10, 46)])
def test_saturated_residues(im, small, blocks, bits):
    """every residue of the touched ciphertexts is q_j - 1 (planted through hydia_db_import_ct): the smallest input at which a
    missing reduction, or a carry into the neighbouring 46-bit field, shows.  Expected: the oracle's hyo_add_inplace."""
    P, K, Or, cc = small
    n = blocks * P.slots - 3
    sat = saturated_ct(P, Or)
    g0 = 0 if blocks == 1 else 3
    first = 500 if blocks == 1 else 4 * P.slots - 10  # inside block 0 / across the edge of blocks 3 and 4
    touched_blocks = (0,) if blocks == 1 else (3, 4)
    cc.db_alloc(n)
    assert cc.db_kind() == 5 and cc.db_residue_bits() == bits and cc.db_group() == (0 if blocks == 1 else 2)
    cts = [None] * (blocks * P.dim)
    for g in touched_blocks:
        for t in block(P, g):
            cc.db_import_ct(t, sat.data())
            cts[t] = sat
    assert np.array_equal(cc.db_export_ct(g0 * P.dim + 1), sat.data())
    ref = UpdateRef(P, Or).planted(n, cts)
    rows = np.random.default_rng(6).integers(-99, 100, size=(25, P.dim)).astype(np.float64)
    touched = ref.update(first, rows.copy(), 1, 33)
    cc.db_update(first, rows.copy(), True, seed=33)
    assert len(touched) == len(touched_blocks) * P.dim
    same(cc, ref, touched)
    assert cc.db_stats()[:2] == (n, blocks * P.dim)


def test_pre_rotated_form(im, small):
    """set_matvec(8), kind 6: an append that opens block 1 (16 loop-B blocks of 8 ciphertexts: the database becomes
    group-sequential) and an update inside block 0, against hyo_enroll_layout_row_bsgs; the form stays"""
    P, K, Or, cc = small
    rng = np.random.default_rng(7)
    n0, extra = 1000, 100
    db = rng.integers(-99, 100, size=(n0 + extra, P.dim)).astype(np.float64)
    db[n0 + 50] = rng.integers(1, 4, size=P.dim)
    cc.set_matvec(8)
    try:
        ref = UpdateRef(P, Or, babies=8).enroll(db[:n0].copy(), 41)
        enr = im.DiagonalEnroller(cc, n0)
        enr.serializeDB(db[:n0].copy(), seed=41)
        assert cc.db_kind() == 6 and cc.db_babies() == 8 and cc.db_group() == 0
        same(cc, ref, (0, 9, P.dim - 1))
        touched = ref.update(n0, db[n0:].copy(), 1, 42)
        enr.appendDB(db[n0:].copy(), seed=42)
        assert cc.db_kind() == 6 and cc.db_babies() == 8 and cc.db_stats()[:2] == (n0 + extra, 2 * P.dim)
        assert cc.db_group() > 0
        same(cc, ref, touched)
        rows = rng.integers(-99, 100, size=(3, P.dim)).astype(np.float64)
        touched = ref.update(10, rows.copy(), 1, 43)
        enr.updateRows(10, rows.copy(), True, seed=43)
        assert touched == list(block(P, 0)) and cc.db_babies() == 8 and cc.db_kind() == 6
        same(cc, ref, range(2 * P.dim))
        n = n0 + extra
        query = np.ones(P.dim)
        q = Or.encrypt_query(query, 5, 1)
        gq = cc.import_ct(q.data(), q.scale)
        sender = im.DiagonalSender(cc, n)
        want = Or.compute_similarity(q, ref.array(), n)
        got = sender.computeSimilarity(gq).export()
        for g in range(2):
            assert np.array_equal(got[g], want[g].data()), g
        assert n0 + 50 in im.DiagonalReceiver(cc, n).decryptIndex(sender.indexScenario(gq))
    finally:
        cc.set_matvec("auto")


def test_new_blocks_equal_a_shard_enrolment(im, small):
    """blocks 2..3 made by a _shard update (first_block = 0) are the ciphertexts hydia_db_enroll_shard makes of the same rows with
    the same seed at first_block = 2 — and both are the oracle's"""
    P, K, Or, cc = small
    rng = np.random.default_rng(8)
    n0, extra = 2 * P.slots, 1500
    db = rng.integers(-99, 100, size=(n0 + extra, P.dim)).astype(np.float64)
    cc.set_matvec("hoisted")
    try:
        ref = UpdateRef(P, Or).enroll(db[:n0].copy(), 60)
        im.DiagonalEnroller(cc, n0).serializeDB(db[:n0].copy(), seed=60)
        touched = ref.update(n0, db[n0:].copy(), 1, 61, first_block=0)
        cc.db_update(n0, db[n0:].copy(), True, seed=61, first_block=0)
        assert touched == list(range(2 * P.dim, 4 * P.dim)) and cc.db_stats()[:2] == (n0 + extra, 4 * P.dim)
        by_update = [cc.db_export_ct(t) for t in touched]
        im.DiagonalEnroller(cc, extra).serializeDB(db[n0:].copy(), seed=61, first_block=2, matvec="hoisted")
        assert cc.db_stats()[:2] == (extra, 2 * P.dim)
        for k, t in enumerate(touched):
            got = cc.db_export_ct(k)
            assert np.array_equal(got, by_update[k]), t
            assert np.array_equal(got, ref.cts[t].data()), t
    finally:
        cc.set_matvec("auto")


def test_refused_calls_leave_the_database_alone(im, small):
    P, K, Or, cc = small
    L = cc.L
    rng = np.random.default_rng(9)
    rows = rng.integers(-99, 100, size=(4, P.dim)).astype(np.float64)
    seed = np.frombuffer((5).to_bytes(32, "little"), dtype=np.uint8).copy()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def update(c, first, r, n, shard=False):
        if shard:
            return L.hydia_db_update_shard(c.h, first, None if r is None else vp(r), n, 1, vp(seed), 0)
        return L.hydia_db_update(c.h, first, None if r is None else vp(r), n, 1, vp(seed))

    # no database
    fresh = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        assert update(fresh, 0, rows.copy(), 4) == ERR_STATE and update(fresh, 0, rows.copy(), 4, shard=True) == ERR_STATE
    finally:
        fresh.close()
    # kinds 4, 1 and 3
    n = 300
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for enroll in (lambda: im.HersEnroller(cc, n).serializeDB(db.copy(), seed=3),
                   lambda: im.BaseEnroller(cc, n).serializeDB(db.copy(), seed=3),
                   lambda: im.BlindEnroller(cc, n).serializeDB(db.copy(), chunk_length=16, seed=3)):
        enroll()
        assert cc.db_kind() in (1, 3, 4)
        before = cc.db_export_ct(1)
        assert update(cc, 0, rows.copy(), 4) == ERR_STATE
        with pytest.raises(im.HydiaError) as e:
            cc.db_update(0, rows.copy(), True, seed=5)
        assert e.value.code == ERR_STATE
        assert np.array_equal(cc.db_export_ct(1), before) and cc.db_stats()[0] == n
    # a diagonal database: argument errors, and the empty update
    im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=3)
    stats, before = cc.db_stats(), cc.db_export_ct(1)
    assert update(cc, n + 1, rows.copy(), 4) == ERR_ARG            # a hole
    assert update(cc, n + 1, rows.copy(), 4, shard=True) == ERR_ARG
    assert update(cc, 0, None, 4) == ERR_ARG                       # null rows with n > 0
    assert L.hydia_db_update(cc.h, 0, vp(rows), 4, 1, None) == ERR_ARG  # null seed
    assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(1), before)
    assert update(cc, 0, None, 0) == 0 and update(cc, n, rows.copy(), 0) == 0  # n == 0: nothing changes
    assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(1), before)
    assert update(cc, n, rows.copy(), 4) == 0 and cc.db_stats()[0] == n + 4  # first_vector == n_old is the append


def test_growth_without_room_fails_before_anything_is_touched(im):
    """an append that adds a block to a 2^20-vector database (142 GiB resident) needs a second buffer of 145 GiB, which a 288 GB GPU
    does not have: HYDIA_ERR_DEVICE, and vectors, ciphertexts, layout and form are what they were"""
    cc = im.Context()
    try:
        cc.set_matvec("hoisted")
        cc.db_fill_random(1 << 20, 5)
        stats, group = cc.db_stats(), cc.db_group()
        assert cc.db_kind() == 5 and stats[0] == 1 << 20 and stats[2] > 140 << 30
        before = {t: cc.db_export_ct(t) for t in (0, 777, stats[1] - 1)}
        rows = np.ones((1, 512))
        with pytest.raises(im.HydiaError) as e:
            cc.db_update(1 << 20, rows, True, seed=1)
        assert e.value.code == -3 and "second buffer" in str(e.value)  # HYDIA_ERR_DEVICE
        assert cc.db_stats() == stats and cc.db_group() == group and cc.db_kind() == 5 and cc.db_babies() == 512
        for t, want in before.items():
            assert np.array_equal(cc.db_export_ct(t), want), t
    finally:
        cc.set_matvec("auto")
        cc.close()
