"""Re-keying the resident database on the GPU (hydia_keygen_switch / hydia_db_rekey; run with -m gpu): the switching key, every
resident layout (ciphertext-major 48-bit, group-sequential 46- and 48-bit, the pre-rotated form, HERS columns), crafted ciphertexts
and keys at the lazy sums' bounds, a ragged last chunk, the hand-over end to end, shard contexts, the refused calls and the full ring.
Every comparison of ciphertexts is np.array_equal of db_export_ct against the restatement on the CPU oracle (tests/db_rekey_ref.py:
hyo_keyswitch of c1, c0 + ks0) applied to the ciphertexts the database held before — bit for bit, never against the product itself.
Ring: N = 2^11, 64-dim vectors (1024 slots, 64 ciphertexts per block) unless said."""
import ctypes as C

import numpy as np
import pytest

import keyswitch_ref as KS
import oracle_lib as O
from db_rekey_ref import rekey_ct, switch_key
from db_update_ref import UpdateRef

pytestmark = pytest.mark.gpu
TOL = 1e-4
ERR_ARG, ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def make_ctx(im, seed, log_n=11):
    cc = im.Context(im.default_params(log_n=log_n, vector_dim=64), 0)
    cc.keygen(seed)
    return cc


@pytest.fixture(scope="module")
def small(im):
    """the oracle's parameters and keys 7 / 8, the sender's context (key 7) and the new receiver's (key 8), and the restated
    switching key 7 -> 8 under seed 100 (shared, never modified)"""
    P = O.Params(log_n=11, depth=11, dim=64)
    K7, K8 = O.Keys(P, 7), O.Keys(P, 8)
    cc7, cc8 = make_ctx(im, 7), make_ctx(im, 8)
    key = switch_key(P, K7, K8, 100)
    key.setflags(write=False)
    yield P, K7, K8, cc7, cc8, key
    cc7.close()
    cc8.close()


def make_rows(P, n, seed, planted=()):
    rng = np.random.default_rng(seed)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for i in planted:
        db[i] = rng.integers(1, 4, size=P.dim)
    return db


def state(cc):
    return cc.db_kind(), cc.db_babies(), cc.db_group(), cc.db_residue_bits(), cc.db_stats()


def rekey_and_compare(P, cc, key, ts, chunk=0):
    """export ciphertexts ts, re-key the database, compare each of ts with the restatement applied to what it held"""
    ts = list(ts)
    before, st = {t: cc.db_export_ct(t) for t in ts}, state(cc)
    cc.db_rekey(key, chunk=chunk)
    assert state(cc) == st
    for t in ts:
        got = cc.db_export_ct(t)
        assert np.array_equal(got, rekey_ct(P, before[t], key)), (t, KS.first_difference(got, rekey_ct(P, before[t], key)))
    return before


def move(ct, dst):
    """a ciphertext batch of one context imported into another (same parameters)"""
    return dst.import_ct(ct.export(), ct.shape()[3])


def adopt_new_keys(cc_sender, cc_new):
    """what the caller does after a re-key: the NEW receiver's evaluation keys and public key go to the sender"""
    rots, r = list(range(cc_new.dim)), cc_new.dim  # 0 = relinearisation, 1 .. dim-1, then the powers of two below the slot count
    while r < cc_new.slots:
        rots.append(r)
        r *= 2
    for r in rots:
        cc_sender.import_eval_key(r, cc_new.export_eval_key(r))
    cc_sender.import_public_key(cc_new.export_public_key())


def test_switch_key_generation(im, small):
    """Context.keygen_switch on the key-8 context from the key-7 secret equals the restatement bit for bit; the context's own keys
    stay; another seed gives another key"""
    P, K7, K8, cc7, cc8, key = small
    assert np.array_equal(cc7.export_secret_key(), K7.s_ntt()) and np.array_equal(cc8.export_secret_key(), K8.s_ntt())
    relin, rot1 = cc8.export_eval_key(0), cc8.export_eval_key(1)
    got = cc8.keygen_switch(cc7.export_secret_key(), 100)
    assert got.shape == (P.dnum, 2, P.nT, P.N)
    assert np.array_equal(got, key), KS.first_difference(got, key)
    assert np.array_equal(cc8.export_eval_key(0), relin) and np.array_equal(cc8.export_eval_key(1), rot1)
    assert not np.array_equal(cc8.keygen_switch(cc7.export_secret_key(), 101), key)
    assert np.array_equal(im.DiagonalReceiver(cc8, 1).genSwitchKey(cc7.export_secret_key(), seed=100), key)


@pytest.mark.parametrize("n", [1024 - 3, 1536])
def test_ciphertext_major_48bit(im, small, n):
    """kind 5, one block and a ragged 1.5 blocks (two blocks of ciphertexts): every ciphertext; kind, form, layout and counts stay.
    The database before the re-key is the oracle's enrolment, so the comparison is anchored at the oracle on both ends."""
    P, K7, K8, cc7, cc8, key = small
    db = make_rows(P, n, 21)
    cc7.set_matvec("hoisted")
    try:
        ref = UpdateRef(P, O.Oracle(P, K7)).enroll(db.copy(), 41)
        enr = im.DiagonalEnroller(cc7, n)
        enr.serializeDB(db.copy(), seed=41)
        cts = cc7.db_stats()[1]
        assert cc7.db_kind() == 5 and cc7.db_group() == 0 and cc7.db_residue_bits() == 48 and cts == -(-n // P.slots) * P.dim
        before = rekey_and_compare(P, cc7, key, range(cts))
        for t in (0, cts - 1):
            assert np.array_equal(before[t], ref.cts[t].data())
        if n > P.slots:  # through the role method, a second time (8 -> 8 is not meaningful; the arithmetic is the same)
            st, b0 = state(cc7), cc7.db_export_ct(cts - 1)
            enr.rekeyDB(key)
            assert state(cc7) == st and np.array_equal(cc7.db_export_ct(cts - 1), rekey_ct(P, b0, key))
    finally:
        cc7.set_matvec("auto")


@pytest.mark.parametrize("env,bits", [({}, 46), ({"HYDIA_DB_48BIT": "1"}, 48)])
def test_group_sequential(im, small, env, bits, monkeypatch):
    """10 blocks, groups of 2, 46-bit granules and 6-byte residues (HYDIA_DB_48BIT in a context of its own): every ciphertext of blocks
    0, 1, 8 and 9 (first and last group, both positions in a group) and one diagonal of every other block"""
    P, K7, K8, cc7, cc8, key = small
    cc, own = cc7, None
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cc = own = make_ctx(im, 7)
        for k in env:
            monkeypatch.delenv(k)
    n = 10 * P.slots - 3
    cc.set_matvec("hoisted")
    try:
        im.DiagonalEnroller(cc, n).serializeDB(make_rows(P, n, 22), seed=41)
        assert cc.db_kind() == 5 and cc.db_group() == 2 and cc.db_residue_bits() == bits and cc.db_stats()[1] == 10 * P.dim
        ts = [g * P.dim + i for g in (0, 1, 8, 9) for i in range(P.dim)] + [g * P.dim + (7 * g + 3) % P.dim for g in range(2, 8)]
        rekey_and_compare(P, cc, key, ts)
    finally:
        cc.set_matvec("auto")
        if own is not None:
            own.close()


def test_pre_rotated_form_and_hers(im, small):
    """kind 6 with 8 babies, 3 blocks = 24 loop-B blocks (group-sequential); kind 4 (HERS columns), one block, ciphertext-major"""
    P, K7, K8, cc7, cc8, key = small
    n = 3 * P.slots - 3
    cc7.set_matvec(8)
    try:
        im.DiagonalEnroller(cc7, n).serializeDB(make_rows(P, n, 23), seed=41)
        assert cc7.db_kind() == 6 and cc7.db_babies() == 8 and cc7.db_group() > 0 and cc7.db_stats()[1] == 3 * P.dim
        rekey_and_compare(P, cc7, key, range(3 * P.dim))
    finally:
        cc7.set_matvec("auto")
    n = P.slots - 5
    im.HersEnroller(cc7, n).serializeDB(make_rows(P, n, 24), seed=3)
    assert cc7.db_kind() == 4 and cc7.db_stats()[1] == P.dim
    rekey_and_compare(P, cc7, key, range(P.dim))


KEY_CASES = [(1, "sat"), (1, "edge"), (1, "digit-0"), (1, "digit-2"), (10, "holes"), (10, "uniform"), (10, "digit-1"), (10, "sat")]


@pytest.mark.parametrize("blocks,pattern", KEY_CASES)
def test_edges_crafted_ciphertexts_and_keys(im, small, blocks, pattern):
    """Ciphertexts whose residues are `sat` (every residue q_j - 1) and `edge` (the cycle 0, 1, q_j - 2, q_j - 1) planted with
    db_import_ct among uniform ones, re-keyed with a crafted switching key.  The key patterns of keyswitch_ref.key_patterns(3) are
    rotated over the two databases instead of the full product — covered: 1 block (ciphertext-major, 48-bit pairs) x {sat, edge,
    digit-0, digit-2}, 10 blocks (group-sequential, 46-bit granules) x {holes, uniform, digit-1, sat}; every case holds BOTH
    ciphertext patterns, so each key pattern meets sat and edge operands, `sat` meets both layouts, and all three digits are used
    (n_q = 12: nothing is poisoned).  sat x sat is the largest inner product and, with c0 = q_j - 1, the largest sum the store
    reduces before it packs."""
    P, K7, K8, cc7, cc8, key = small
    assert KS.digits_in_use(P, P.nQ) == P.dnum and {p for _, p in KEY_CASES} == set(KS.key_patterns(P.dnum))
    rng = np.random.default_rng(31 + blocks)
    Or = O.Oracle(P, K7)
    cc7.set_matvec("hoisted")
    try:
        cc7.db_fill_random(blocks * P.slots - 3, 9)
    finally:
        cc7.set_matvec("auto")
    assert cc7.db_kind() == 5 and cc7.db_group() == (0 if blocks == 1 else 2) and cc7.db_residue_bits() == (48 if blocks == 1 else 46)
    last = blocks * P.dim - 1
    plant = {0: "sat", 1: "edge", P.dim // 2: "edge", last - 1: "edge", last: "sat"}
    if blocks > 1:
        plant.update({P.dim + 5: "sat", 4 * P.dim + 17: "edge", 8 * P.dim: "edge", 9 * P.dim + 1: "sat"})
    for k, (t, pat) in enumerate(plant.items()):
        ct = KS.craft_ct(P, Or.encrypt(np.zeros(P.slots), 1, 1), pat, rng, phase=k)
        cc7.db_import_ct(t, ct.data())
    crafted = KS.craft_key(P, np.zeros((P.dnum, 2, P.nT, P.N), dtype=np.uint64), pattern, rng, phase=blocks)
    rekey_and_compare(P, cc7, crafted, list(plant) + [2, last - 2])


def test_chunking_with_a_ragged_last_chunk(im, small):
    """1.5 blocks (128 ciphertexts) in chunks of 48: 48 + 48 + 32 — every ciphertext, so the first, the last and both boundaries;
    the three timers each saw three chunks"""
    P, K7, K8, cc7, cc8, key = small
    n = 1536
    cc7.set_matvec("hoisted")
    try:
        im.DiagonalEnroller(cc7, n).serializeDB(make_rows(P, n, 25), seed=41)
        cc7.kernel_time_reset()
        rekey_and_compare(P, cc7, key, range(2 * P.dim), chunk=48)
        for name in ("db_rekey_gather", "db_rekey_switch", "db_rekey_store"):
            ms, launches = cc7.kernel_time(name)
            assert launches == 3 and ms > 0, name
    finally:
        cc7.set_matvec("auto")


def test_end_to_end_hand_over(im, small):
    """enrol under key 7; the key-8 receiver makes the switching key; the sender re-keys and takes key 8's evaluation keys: the key-8
    receiver finds the planted rows, a no-match query gives false, the key-7 receiver no longer reads the scores, and an append under
    the new public key matches"""
    P, K7, K8, cc7, cc8, key = small
    n, planted = 1500, [3, 700, 1400]
    db = make_rows(P, n, 26, planted)
    gallery = db / np.linalg.norm(db, axis=1, keepdims=True)
    sender_cc = make_ctx(im, 7)  # a context of its own: its keys are replaced below
    try:
        enr = im.DiagonalEnroller(sender_cc, n)
        enr.serializeDB(db.copy(), seed=41)
        old_receiver, new_receiver = im.DiagonalReceiver(cc7, n), im.DiagonalReceiver(cc8, n)
        enr.rekeyDB(new_receiver.genSwitchKey(cc7.export_secret_key(), seed=100))
        adopt_new_keys(sender_cc, cc8)
        sender = im.DiagonalSender(sender_cc, n)
        query = np.ones(P.dim)
        qc = move(new_receiver.encryptQuery(query, seed=5, nonce=1), sender_cc)
        assert set(planted) <= set(new_receiver.decryptIndex(move(sender.indexScenario(qc), cc8)))
        assert new_receiver.decryptMembership(move(sender.membershipScenario(qc), cc8)) is True
        nomatch = np.where(np.arange(P.dim) % 2 == 0, 1.0, -1.0)
        qn = move(new_receiver.encryptQuery(nomatch, seed=5, nonce=2), sender_cc)
        assert new_receiver.decryptMembership(move(sender.membershipScenario(qn), cc8)) is False
        cos = gallery @ (query / np.linalg.norm(query))
        sim = sender.computeSimilarity(qc)
        assert np.abs(cc8.decrypt(move(sim, cc8)).reshape(-1)[:n] - cos).max() < TOL
        assert np.abs(cc7.decrypt(move(sim, cc7)).reshape(-1)[:n] - cos).max() > TOL  # no longer opens under the old key
        del old_receiver
        # a later append: encrypted under the NEW public key (imported above)
        extra = make_rows(P, 40, 27, [20])
        enr.appendDB(extra, seed=77)
        n2 = n + 40
        sender, new_receiver = im.DiagonalSender(sender_cc, n2), im.DiagonalReceiver(cc8, n2)
        assert set(planted + [n + 20]) <= set(new_receiver.decryptIndex(move(sender.indexScenario(qc), cc8)))
    finally:
        sender_cc.close()


def test_shard_contexts(im, small):
    """a hydia_group of 2 shards on one GPU (2 blocks each, keys shared): db_rekey on each shard context gives, on that shard's blocks,
    the restatement of what it held — and that is what the single context holds after its own re-key"""
    P, K7, K8, cc7, cc8, key = small
    n = 4 * P.slots - 3
    db = make_rows(P, n, 28)
    cc7.set_matvec("hoisted")
    grp = im.ShardGroup([0, 0], im.default_params(log_n=11, vector_dim=64))
    try:
        im.DiagonalEnroller(cc7, n).serializeDB(db.copy(), seed=41)
        assert cc7.db_stats()[1] == 4 * P.dim
        ts = [0, 5, P.dim - 1, P.dim, 2 * P.dim - 1, 2 * P.dim, 2 * P.dim + 9, 3 * P.dim + 1, 4 * P.dim - 1]
        before = rekey_and_compare(P, cc7, key, ts)
        grp.ctx0.set_matvec("hoisted")
        grp.keygen(7)
        im.ShardedDiagonalEnroller(grp, n).serializeDB(db.copy(), seed=41)
        shards = [grp.shard_ctx(r) for r in range(2)]
        states = [state(s) for s in shards]
        assert [s.db_stats()[1] for s in shards] == [2 * P.dim, 2 * P.dim]
        for t in ts:  # the shards hold the single context's ciphertexts (same keys, same nonces)
            r, local = divmod(t, 2 * P.dim)
            assert np.array_equal(shards[r].db_export_ct(local), before[t]), t
        for s in shards:
            s.db_rekey(key)
        assert [state(s) for s in shards] == states
        for t in ts:
            r, local = divmod(t, 2 * P.dim)
            assert np.array_equal(shards[r].db_export_ct(local), rekey_ct(P, before[t], key)), t
    finally:
        cc7.set_matvec("auto")
        grp.close()


def test_refused_calls_leave_everything_alone(im, small):
    P, K7, K8, cc7, cc8, key = small
    L = cc7.L
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    k = np.ascontiguousarray(key)

    def refused(fn, code, *words):
        with pytest.raises(im.HydiaError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    # no database, and a key generation without a secret
    fresh = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        refused(lambda: fresh.db_rekey(k), ERR_STATE, "no database")
        assert L.hydia_db_rekey(fresh.h, vp(k)) == ERR_STATE
        refused(lambda: fresh.keygen_switch(cc7.export_secret_key(), 1), ERR_STATE, "secret")
        assert fresh.db_stats()[:2] == (0, 0) and fresh.db_kind() == 0
    finally:
        fresh.close()
    refused(lambda: cc8.keygen_switch(None, 1), ERR_ARG)
    # kinds 1 and 3
    n = 300
    db = make_rows(P, n, 29)
    for kind, enroll in ((1, lambda: im.BaseEnroller(cc7, n).serializeDB(db.copy(), seed=3)),
                         (3, lambda: im.BlindEnroller(cc7, n).serializeDB(db.copy(), chunk_length=16, seed=3))):
        enroll()
        assert cc7.db_kind() == kind
        st, before = state(cc7), cc7.db_export_ct(1)
        refused(lambda: cc7.db_rekey(k), ERR_STATE, "kind %d" % kind)
        assert L.hydia_db_rekey(cc7.h, vp(k)) == ERR_STATE
        assert state(cc7) == st and np.array_equal(cc7.db_export_ct(1), before)
    # a plain gallery, hoisted (7) and pre-rotated (8): nothing is encrypted
    for kind, mv in ((7, "hoisted"), (8, 8)):
        cc7.set_matvec(mv)
        try:
            im.PlainEnroller(cc7, n).serializeDB(db.copy())
        finally:
            cc7.set_matvec("auto")
        assert cc7.db_kind() == kind
        st, before = state(cc7), cc7.plain_db_export_pt(1)
        refused(lambda: cc7.db_rekey(k), ERR_STATE, "kind %d" % kind, "nothing is encrypted")
        assert state(cc7) == st and np.array_equal(cc7.plain_db_export_pt(1), before)
    # a diagonal database: a null key
    im.DiagonalEnroller(cc7, n).serializeDB(db.copy(), seed=3)
    st, before = state(cc7), cc7.db_export_ct(1)
    refused(lambda: cc7.db_rekey(None), ERR_ARG, "null")
    assert L.hydia_db_rekey(cc7.h, None) == ERR_ARG
    assert state(cc7) == st and np.array_equal(cc7.db_export_ct(1), before)


def test_full_ring_once(im):
    """N = 2^15, 64-dim vectors, one block (64 ciphertexts) through the fused key-switching pipeline: the switching key and every
    ciphertext bit for bit, and the hand-over's query finds its row"""
    P = O.Params(log_n=15, depth=11, dim=64)
    K7, K8 = O.Keys(P, 7, rotations=[]), O.Keys(P, 8, rotations=[])  # the secrets are all the restatement reads
    key = switch_key(P, K7, K8, 100)
    cc7, cc8 = make_ctx(im, 7, 15), make_ctx(im, 8, 15)
    try:
        got = cc8.keygen_switch(cc7.export_secret_key(), 100)
        assert np.array_equal(got, key), KS.first_difference(got, key)
        n, row = P.dim * 4, 77  # a few vectors per diagonal are enough: the block is 64 ciphertexts whatever n
        cc7.set_matvec("hoisted")
        im.DiagonalEnroller(cc7, n).serializeDB(make_rows(P, n, 30, [row]), seed=41)
        assert cc7.db_kind() == 5 and cc7.db_stats()[1] == P.dim
        cc7.kernel_time_reset()
        rekey_and_compare(P, cc7, key, range(P.dim))
        assert cc7.kernel_time("db_rekey_switch")[1] == 1 and cc7.kernel_time("ks_inner_product")[1] == 1
        adopt_new_keys(cc7, cc8)
        receiver, sender = im.DiagonalReceiver(cc8, n), im.DiagonalSender(cc7, n)
        qc = move(receiver.encryptQuery(np.ones(P.dim), seed=5, nonce=1), cc7)
        assert row in receiver.decryptIndex(move(sender.indexScenario(qc), cc8))
    finally:
        cc7.close()
        cc8.close()
