"""Seeded keys and seeded secret-key queries on the GPU (include/hydia.h, hydia_keygen_seeded .. hydia_ct_expand_seeded; run with
-m gpu): the seeded key set, half keys out and in, the fused encryption kernel k_enc_sym and the sender's expansion, two contexts end
to end, and the refusals.  Every comparison of residues is np.array_equal against the restatement on the CPU oracle's primitives
(tests/seeded_ref.py), never against the product itself.
Ring: N = 2^11, 64-dim vectors (1024 slots, n_q 12, n_p 4, dnum 3: N / 4 ChaCha blocks fill two workgroups) unless said."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import seeded_ref as SR
from db_rekey_ref import as_oracle_cts

pytestmark = pytest.mark.gpu
TOL = 1e-4
ERR_ARG, ERR_STATE = -1, -2
SEED, A_SEED = 7, 1007


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def new_ctx(im, log_n=11, dim=64):
    return im.Context(im.default_params(log_n=log_n, vector_dim=dim), 0)


@pytest.fixture(scope="module")
def torch():
    """torch where it is installed (else None), imported before this module's first context is created — the order in which
    tests/test_gpu_device_rows.py gets its tensors"""
    try:
        import torch
    except ImportError:
        return None
    return torch


@pytest.fixture(scope="module")
def small(im, torch):
    """the oracle's parameters, its own key set under SEED (never modified), a second one with the restated seeded keys installed, the
    restated keys themselves, and the receiver's context after keygen_seeded(SEED, A_SEED) — shared, never re-keyed"""
    P = O.Params(log_n=11, depth=11, dim=64)
    K0, K = O.Keys(P, SEED), O.Keys(P, SEED)
    keys, pk = SR.install(K, P, SEED, A_SEED)
    R = new_ctx(im)
    R.keygen_seeded(SEED, A_SEED)
    yield P, K0, K, keys, pk, R
    R.close()
    P.close()


def probe(P, seed):
    return np.random.default_rng(seed).integers(-99, 100, size=P.dim).astype(np.float64)


def raises(im, code, fn, *args, **kw):
    with pytest.raises(im.HydiaError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value


def move(ct, dst):
    return dst.import_ct(ct.export(), ct.shape()[3])


# ------------------------------------------------------------------------------------------------ 1. keys
def test_seeded_key_set(im, small):
    P, K0, K, keys, pk, R = small
    assert np.array_equal(R.export_secret_key(), K0.s_ntt())
    assert np.array_equal(R.export_public_key(), pk)
    for r in (0, 1, P.dim - 1, P.dim, P.slots // 2):
        assert np.array_equal(R.export_eval_key(r), keys[r]), r
    assert R.key_seed() == O.seed_bytes(A_SEED).tobytes()
    cc = new_ctx(im)
    try:
        raises(im, ERR_STATE, cc.key_seed)
        cc.keygen_rotations_seeded([1, P.slots - 1], SEED, A_SEED)
        assert np.array_equal(cc.export_eval_key(1), keys[1]) and np.array_equal(cc.export_eval_key(0), keys[0])
        assert cc.has_eval_key(P.slots - 1) and not cc.has_eval_key(2)
        # a_seed == seed would publish the secret's seed: refused before anything is touched
        raises(im, ERR_ARG, cc.keygen_seeded, 5, 5)
        raises(im, ERR_ARG, cc.keygen_rotations_seeded, [1], 5, 5)
        assert np.array_equal(cc.export_eval_key(1), keys[1]) and np.array_equal(cc.export_public_key(), pk)
        assert np.array_equal(cc.export_secret_key(), K0.s_ntt()) and cc.has_eval_key(P.slots - 1)
        assert cc.key_seed() == O.seed_bytes(A_SEED).tobytes()
    finally:
        cc.close()


def test_plain_keygen_did_not_change(im, small):
    """hydia_keygen / hydia_keygen_rotations still make the oracle's own keys (gen_evk and keygen_impl gained an argument)"""
    P, K0, K, keys, pk, R = small
    cc = new_ctx(im)
    try:
        cc.keygen(SEED)
        assert np.array_equal(cc.export_public_key(), K0.pk()) and np.array_equal(cc.export_eval_key(0), K0.relin())
        for r in (1, P.dim - 1, P.slots // 2):
            assert np.array_equal(cc.export_eval_key(r), K0.rot_key(r)), r
        cc.keygen_rotations([1], SEED)
        assert np.array_equal(cc.export_eval_key(1), K0.rot_key(1)) and np.array_equal(cc.export_eval_key(0), K0.relin())
    finally:
        cc.close()


# ------------------------------------------------------------------------------------------------ 2. halves
def test_half_keys_out_and_in(im, small):
    P, K0, K, keys, pk, R = small
    a_seed = R.key_seed()
    S = new_ctx(im)  # no secret, no keys
    try:
        for r in (0, 1, P.dim - 1, P.slots // 2):
            b = R.export_eval_key_seeded(r)
            assert b.shape == (P.dnum, P.nT, P.N) and np.array_equal(b, keys[r][:, 0]), r
            S.import_eval_key_seeded(r, b, a_seed)
            assert np.array_equal(S.export_eval_key(r), keys[r]), r
        b = R.export_public_key_seeded()
        assert np.array_equal(b, pk[0])
        S.import_public_key_seeded(b, a_seed)
        assert np.array_equal(S.export_public_key(), pk)
        # a wrong public seed: the same b, another a
        S.import_eval_key_seeded(1, keys[1][:, 0], A_SEED + 1)
        got = S.export_eval_key(1)
        assert np.array_equal(got[:, 0], keys[1][:, 0]) and not np.array_equal(got[:, 1], keys[1][:, 1])
        # the importing context holds no seeded key set
        raises(im, ERR_STATE, S.export_eval_key_seeded, 1)
        raises(im, ERR_STATE, S.export_public_key_seeded)
        raises(im, ERR_STATE, S.key_seed)
    finally:
        S.close()


def test_marks_follow_the_writers(im, small):
    P, K0, K, keys, pk, R = small
    cc = new_ctx(im)
    try:
        cc.keygen(SEED)  # a plain key set: nothing is marked
        raises(im, ERR_STATE, cc.export_eval_key_seeded, 0)
        raises(im, ERR_STATE, cc.export_public_key_seeded)
        cc.keygen_rotations_seeded([1, 2], SEED, A_SEED)
        assert np.array_equal(cc.export_eval_key_seeded(2), SR.seeded_rot(P, K0, SEED, A_SEED, 2)[:, 0])
        cc.import_eval_key(1, keys[1])  # an imported key is whatever the caller sent: that key only loses its mark
        raises(im, ERR_STATE, cc.export_eval_key_seeded, 1)
        assert np.array_equal(cc.export_eval_key_seeded(0), keys[0][:, 0]) and np.array_equal(cc.export_eval_key_seeded(2)[0], cc.export_eval_key(2)[0, 0])
        cc.import_public_key(pk)
        raises(im, ERR_STATE, cc.export_public_key_seeded)
        raises(im, ERR_STATE, cc.export_eval_key_seeded, 3)  # no such key
    finally:
        cc.close()


# ------------------------------------------------------------------------------------------------ 3. queries
def test_seeded_queries_against_the_restatement(im, small):
    P, K0, K, keys, pk, R = small
    rec = im.DiagonalReceiver(R, 1)
    query = probe(P, 1)
    sq = rec.encryptQuerySeeded(query, seed=SEED, a_seed=A_SEED, nonce=3)
    c0, a = SR.seeded_query(P, K0, query, SEED, A_SEED, 3)
    assert sq.c0.shape == (1, P.nQ, P.N) and np.array_equal(sq.c0[0], c0)
    assert (sq.a_seed, sq.nonce0, sq.nbytes) == (O.seed_bytes(A_SEED).tobytes(), 3, P.nQ * P.N * 8 + 40)
    zero = rec.encryptQuerySeeded(np.zeros(P.dim), seed=SEED, a_seed=A_SEED, nonce=4)
    assert np.array_equal(zero.c0[0], SR.seeded_query(P, K0, np.zeros(P.dim), SEED, A_SEED, 4)[0])
    rows = np.stack([probe(P, s) for s in (2, 3, 4)])
    batch = rec.encryptQueriesSeeded(rows, seed=SEED, a_seed=A_SEED, nonce0=5)
    assert len(batch) == 3 and rows.flags.writeable
    for i in range(3):
        assert np.array_equal(batch.c0[i], SR.seeded_query(P, K0, rows[i], SEED, A_SEED, 5 + i)[0]), i
    # the sender's expansion on a context without any key: c1 is the public seed's stream, bit for bit the a the fused kernel used
    S = new_ctx(im)
    try:
        ct = im.DiagonalSender(S, 1).expandQuery(sq)
        assert ct.shape() == (1, 2, P.nQ, P.delta)
        got = ct.export()[0]
        assert np.array_equal(got[0], c0)
        for j in range(P.nQ):
            assert np.array_equal(got[1, j], O.sample_uniform(A_SEED, SR.stream(SR.DOM_SYM_A, 3, 0, j), int(P.moduli[j]), P.N)), j
        assert np.array_equal(got[1], a)
    finally:
        S.close()
    # on the receiver the expanded handle decrypts as the oracle decrypts the restated ciphertext, and to the probe
    Or = O.Oracle(P, K0)
    want = Or.decrypt(as_oracle_cts(P, Or, [np.stack([c0, a])])[0])
    got = R.decrypt(im.DiagonalSender(R, 1).expandQuery(sq))[0]
    assert np.array_equal(got, want)
    assert np.abs(got - SR.tiled_probe(P, query)).max() < TOL


def test_seeded_queries_from_device_rows(im, small, torch):
    if torch is None:
        pytest.skip("torch is not installed")
    P, K0, K, keys, pk, R = small
    rows32 = np.stack([probe(P, s) for s in (6, 7)]).astype(np.float32) / np.float32(7)
    t = torch.from_numpy(rows32).to("cuda:0")
    rec = im.DiagonalReceiver(R, 1)
    batch = rec.encryptQueriesSeeded(t, seed=SEED, a_seed=A_SEED, nonce0=20)
    for i in range(2):
        assert np.array_equal(batch.c0[i], SR.seeded_query(P, K0, rows32[i].astype(np.float64), SEED, A_SEED, 20 + i)[0]), i
    one = rec.encryptQuerySeeded(t[1], seed=SEED, a_seed=A_SEED, nonce=21)
    assert len(one) == 1 and np.array_equal(one.c0[0], batch.c0[1])


@pytest.mark.parametrize("log_n,dim", [(10, 64), (15, 512)])
def test_ring_edges(im, log_n, dim):
    """N = 2^10: the ChaCha blocks of a limb are exactly one workgroup.  N = 2^15, 512-dim: the full ring, under the single rotation
    key 1 (no 13 GB key set).  The 2^10 ring is the receiver's side only (the transform's contiguous pass takes 1024-coefficient
    chunks there): the secret, the public key and the key it generates are held against the oracle's too, and key switching and a
    resident database are refused on it"""
    P = O.Params(log_n=log_n, depth=11, dim=dim)
    K0 = O.Keys(P, SEED, rotations=[1])
    cc = None
    try:
        cc = new_ctx(im, log_n, dim)
        cc.keygen_rotations_seeded([1], SEED, A_SEED)
        query = probe(P, 9)
        sq = im.DiagonalReceiver(cc, 1).encryptQuerySeeded(query, seed=SEED, a_seed=A_SEED, nonce=(1 << 40) - 1)
        c0, a = SR.seeded_query(P, K0, query, SEED, A_SEED, (1 << 40) - 1)
        assert np.array_equal(sq.c0[0], c0)
        ct = im.DiagonalSender(cc, 1).expandQuery(sq)
        assert np.array_equal(ct.export()[0, 1], a)
        assert np.abs(cc.decrypt(ct)[0] - SR.tiled_probe(P, query)).max() < TOL
        if log_n == 10:
            assert np.array_equal(cc.export_secret_key(), K0.s_ntt())
            assert np.array_equal(cc.export_public_key(), SR.seeded_pk(P, K0, SEED, A_SEED))
            assert np.array_equal(cc.export_eval_key(1), SR.seeded_rot(P, K0, SEED, A_SEED, 1))
            raises(im, ERR_ARG, cc.eval_rotate, ct, 1)
            raises(im, ERR_ARG, cc.db_alloc, 10)
    finally:
        if cc is not None:
            cc.close()
        P.close()


# ------------------------------------------------------------------------------------------------ 4. end to end, two contexts
def test_end_to_end_two_contexts(im, small):
    """receiver R (seeded key set) and sender S (no secret; half keys in, half queries in): the three scenarios equal the oracle's under
    the installed restated keys on the restated query and its own enrolment under the same seed, bit for bit"""
    P, K0, K, keys, pk, R = small
    n, planted = 1536, 1100
    rng = np.random.default_rng(31)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    db[planted] = rng.integers(1, 4, size=P.dim)
    query = np.ones(P.dim)
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))
    assert [int(i) for i in np.nonzero(cos >= 0.44)[0]] == [planted] and np.sort(cos)[-2] < 0.40  # (a property of the data)
    receiver = im.DiagonalReceiver(R, n)
    S = new_ctx(im)
    try:
        sender = im.DiagonalSender(S, n)
        shipped = receiver.exportKeysSeeded()
        assert shipped.a_seed == R.key_seed() and sorted(shipped.eval_keys) == sorted([0] + O.default_rotations(P))
        assert shipped.nbytes == 32 + P.nQ * P.N * 8 + len(shipped.eval_keys) * P.dnum * P.nT * P.N * 8
        sender.importKeysSeeded(shipped)
        raises(im, ERR_STATE, S.export_secret_key)
        im.DiagonalEnroller(S, n).serializeDB(db.copy(), seed=41)
        sq = receiver.encryptQuerySeeded(query, seed=SEED, a_seed=A_SEED, nonce=1)
        q = sender.expandQuery(sq)
        Or = O.Oracle(P, K)
        c0, a = SR.seeded_query(P, K0, query, SEED, A_SEED, 1)
        oq = as_oracle_cts(P, Or, [np.stack([c0, a])])[0]
        dbc = Or.enroll(db.copy(), 41)
        idx, gidx = Or.index_scenario(oq, dbc, n), sender.indexScenario(q)
        sim, gsim = Or.compute_similarity(oq, dbc, n), sender.computeSimilarity(q).export()
        gi = gidx.export()
        assert len(idx) == len(sim) == 2
        for g in range(2):
            assert np.array_equal(gi[g], idx[g].data()) and np.array_equal(gsim[g], sim[g].data()), g
        mem, gmem = Or.membership_scenario(oq, dbc, n), sender.membershipScenario(q)
        assert np.array_equal(gmem.export()[0], mem.data())
        assert receiver.decryptIndex(move(gidx, R)) == [planted]
        assert receiver.decryptMembership(move(gmem, R)) is True
        # the expanded handles are ordinary: a batch of two equals the two single calls
        second = probe(P, 12)
        two = receiver.encryptQueriesSeeded(np.stack([query, second]), seed=SEED, a_seed=A_SEED, nonce0=1)
        qs = sender.expandQueries(two)
        assert np.array_equal(qs[0].export(), q.export())
        multi = sender.indexScenarioMulti(qs)
        assert np.array_equal(multi[0].export(), gi) and np.array_equal(multi[1].export(), sender.indexScenario(qs[1]).export())
    finally:
        S.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(im, small):
    P, K0, K, keys, pk, R = small
    L = R.L
    seed, a_seed = O.seed_bytes(SEED), O.seed_bytes(A_SEED)
    query = probe(P, 1)
    guard = np.full((P.nQ, P.N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    out, vp = guard.copy(), lambda x: x.ctypes.data_as(C.c_void_p)
    enc1, encn = L.hydia_encrypt_query_seeded, L.hydia_encrypt_queries_seeded
    # no secret key on the encrypting context
    S = new_ctx(im)
    try:
        S.import_public_key(pk)
        assert enc1(S.h, vp(query), vp(seed), vp(a_seed), 1, vp(out)) == ERR_STATE
        raises(im, ERR_STATE, im.DiagonalReceiver(S, 1).encryptQuerySeeded, query, seed=SEED, a_seed=A_SEED)
        # the expansion needs no key at all, and refuses its own bad arguments
        hs = (C.c_void_p * 1)()
        assert L.hydia_ct_expand_seeded(S.h, vp(out), 1, vp(a_seed), 1 << 40, hs) == ERR_ARG
        assert L.hydia_ct_expand_seeded(S.h, None, 1, vp(a_seed), 1, hs) == ERR_ARG
        assert L.hydia_ct_expand_seeded(S.h, vp(out), 1, None, 1, hs) == ERR_ARG
        assert L.hydia_ct_expand_seeded(S.h, None, 0, vp(a_seed), 1, None) == 0 and not hs[0]
    finally:
        S.close()
    # the nonce space: nonce0 + count <= 2^40
    assert enc1(R.h, vp(query), vp(seed), vp(a_seed), 1 << 40, vp(out)) == ERR_ARG
    two = np.stack([query, query])
    assert encn(R.h, vp(two), 2, vp(seed), vp(a_seed), (1 << 40) - 1, vp(out)) == ERR_ARG
    # null arguments, a_seed == seed
    for args in ((None, vp(query), vp(seed), vp(a_seed), 1, vp(out)), (R.h, None, vp(seed), vp(a_seed), 1, vp(out)),
                 (R.h, vp(query), None, vp(a_seed), 1, vp(out)), (R.h, vp(query), vp(seed), None, 1, vp(out)),
                 (R.h, vp(query), vp(seed), vp(a_seed), 1, None), (R.h, vp(query), vp(seed), vp(seed.copy()), 1, vp(out))):
        assert enc1(*args) == ERR_ARG, args
    # count == 0: nothing to do, nothing written
    assert encn(R.h, None, 0, vp(seed), vp(a_seed), 1, None) == 0
    assert encn(R.h, vp(two), 0, vp(seed), vp(a_seed), 1 << 40, vp(out)) == 0
    assert np.array_equal(out, guard)
    # and the context still encrypts
    assert enc1(R.h, vp(query), vp(seed), vp(a_seed), 3, vp(out)) == 0
    assert np.array_equal(out, SR.seeded_query(P, K0, query, SEED, A_SEED, 3)[0])
