"""A batch of queries in one pass over the encrypted database (hydia_*_multi, DiagonalSender.*Multi), on an MI355X: every result
of a batch equals the single-query call on that query, ciphertext for ciphertext and limb for limb — for the ciphertext-major
layout (at most 8 blocks), the group-sequential 46-bit layout (more than 8), the BSGS output order, the two non-default layouts —
and, for three queries, the CPU oracle's index scenario.  Errors leave every output NULL."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def make_ctx(im, P, env=None):
    prm = im.default_params(log_n=P.log_n, mult_depth=P.nQ - 1, vector_dim=P.dim, dnum=P.dnum)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        cc = im.Context(prm, 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert np.array_equal(cc.moduli, P.moduli)
    return cc


def load_keys(cc, K):
    cc.import_eval_key(0, K.relin())
    for r in K.rotations:
        cc.import_eval_key(r, K.rot_key(r))
    cc.import_public_key(K.pk())
    cc.import_secret_key(K.s_ntt())


def load_db(cc, dbc, n, form):
    cc.set_matvec(form)
    cc.db_alloc(n)
    for t in range(len(dbc)):
        cc.db_import_ct(t, dbc[t].data())
    if getattr(dbc, "bsgs", False):
        cc.db_set_babies(dbc.babies)


def planted_db(P, n, seed):
    rng = np.random.default_rng(seed)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    for i in (0, n // 2, n - 1):
        db[i] = rng.integers(1, 4, size=P.dim)
    return db


def query_vectors(P, db, count, seed):
    """query 0 repeats database row 0, query 1 row n // 2, the rest are random"""
    rng = np.random.default_rng(seed)
    out = [db[0].copy(), db[len(db) // 2].copy()]
    while len(out) < count:
        out.append(rng.integers(-9, 10, size=P.dim).astype(np.float64))
    return out[:count]


def assert_multi_equals_single(sender, gqs, counts=(1, 2, 3, 5)):
    single = {
        "sim": [sender.computeSimilarity(q).export() for q in gqs],
        "idx": [sender.indexScenario(q).export() for q in gqs],
        "mem": [sender.membershipScenario(q).export() for q in gqs],
    }
    calls = {"sim": sender.computeSimilarityMulti, "idx": sender.indexScenarioMulti, "mem": sender.membershipScenarioMulti}
    got3 = None
    for Q in counts:
        for key, fn in calls.items():
            out = fn(gqs[:Q])
            assert len(out) == Q
            for q in range(Q):
                e = out[q].export()
                assert e.shape == single[key][q].shape, (key, Q, q)
                assert np.array_equal(e, single[key][q]), (key, Q, q)
            if key == "idx" and Q == 3:
                got3 = [o.export() for o in out]
    return single, got3


@pytest.fixture(scope="module")
def small(im):
    P = O.Params(log_n=11, depth=11, dim=64)
    K = O.Keys(P, 7)
    cc = make_ctx(im, P)
    load_keys(cc, K)
    yield P, K, O.Oracle(P, K), cc
    cc.close()


@pytest.mark.parametrize("form", ["hoisted", "bsgs"])
@pytest.mark.parametrize("blocks", [1, 3, 10])
def test_small_ring_multi_equals_single_and_oracle(im, small, blocks, form):
    P, K, Or, cc = small
    n = blocks * P.slots - 3
    db = planted_db(P, n, blocks)
    dbc = Or.enroll(db.copy(), 41, matvec=form)
    load_db(cc, dbc, n, form)
    assert cc.db_kind() == (5 if form == "hoisted" else 6)
    if blocks == 10 and form == "hoisted":
        assert cc.db_group() > 0 and cc.db_residue_bits() == 46  # group-sequential, 46-bit residues
    qs = [Or.encrypt_query(v, 5, 1 + i) for i, v in enumerate(query_vectors(P, db, 5, blocks))]
    gqs = [cc.import_ct(q.data(), q.scale) for q in qs]
    sender = im.DiagonalSender(cc, n)
    _, got3 = assert_multi_equals_single(sender, gqs)
    for q in range(3):  # the oracle's index scenario, composed on the CPU
        want = Or.index_scenario(qs[q], dbc, n)
        assert len(want) == got3[q].shape[0]
        for g in range(len(want)):
            assert np.array_equal(got3[q][g], want[g].data()), (q, g)


@pytest.mark.parametrize("env", [{"HYDIA_DB_UNPACKED": "1"}, {"HYDIA_DB_48BIT": "1"}])
def test_small_ring_fallback_layouts(im, small, env):
    P, K, Or, _ = small
    cc = make_ctx(im, P, env)
    load_keys(cc, K)
    try:
        for blocks, form in ((1, "hoisted"), (10, "hoisted"), (10, "bsgs")):
            n = blocks * P.slots - 3
            db = planted_db(P, n, 100 + blocks)
            dbc = Or.enroll(db.copy(), 43, matvec=form)
            load_db(cc, dbc, n, form)
            assert cc.db_residue_bits() == (64 if "HYDIA_DB_UNPACKED" in env else 48)
            qs = [Or.encrypt_query(v, 6, 1 + i) for i, v in enumerate(query_vectors(P, db, 5, blocks))]
            gqs = [cc.import_ct(q.data(), q.scale) for q in qs]
            assert_multi_equals_single(im.DiagonalSender(cc, n), gqs)
    finally:
        cc.close()


@pytest.mark.parametrize("form", ["hoisted", "bsgs"])
def test_full_ring_three_blocks(im, form):
    """Q = 3 on N = 2^15: a query equal to database row 777, one with no match, and the first again under another nonce"""
    cc = im.Context(im.default_params(), 0)
    try:
        cc.keygen(11)
        n = 3 * cc.slots - 5
        rng = np.random.default_rng(3)
        db = rng.integers(-99, 100, size=(n, cc.dim)).astype(np.float64)
        db[777] = rng.integers(1, 4, size=cc.dim)
        cc.set_matvec(form)
        im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=12)
        assert cc.db_kind() == (5 if form == "hoisted" else 6)
        receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
        match = db[777].copy()
        nomatch = np.zeros(cc.dim)
        nomatch[::2], nomatch[1::2] = 1.0, -1.0
        nomatch *= np.sign(rng.standard_normal(cc.dim))  # far from every planted row
        gqs = [receiver.encryptQuery(match, seed=1, nonce=1), receiver.encryptQuery(nomatch, seed=1, nonce=2),
               receiver.encryptQuery(match, seed=1, nonce=3)]
        single, _ = assert_multi_equals_single(sender, gqs, counts=(3,))
        idx = sender.indexScenarioMulti(gqs)
        assert receiver.decryptIndex(idx[0]) == [777]
        assert receiver.decryptIndex(idx[2]) == [777]
        assert 777 not in receiver.decryptIndex(idx[1])
    finally:
        cc.close()


def test_full_ring_ten_blocks_group_sequential(im):
    cc = im.Context(im.default_params(), 0)
    try:
        cc.keygen(13)
        cc.set_matvec("hoisted")
        n = 10 * cc.slots
        cc.db_fill_random(n, seed=5)
        assert cc.db_kind() == 5 and cc.db_group() > 0 and cc.db_residue_bits() == 46
        receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
        rng = np.random.default_rng(10)
        gqs = [receiver.encryptQuery(rng.standard_normal(cc.dim), seed=2, nonce=1 + i) for i in range(2)]
        for q, (a, b) in enumerate(zip(sender.computeSimilarityMulti(gqs), gqs)):
            assert np.array_equal(a.export(), sender.computeSimilarity(b).export()), q
        for q, (a, b) in enumerate(zip(sender.indexScenarioMulti(gqs), gqs)):
            assert np.array_equal(a.export(), sender.indexScenario(b).export()), q
    finally:
        cc.close()


def test_reference_fixture_2_10(im):
    """test/2_10.dat with Q = 2 (the fixture query and another): the fixture query's index is [0], its membership true"""
    g = np.load(os.path.join(GOLDEN, "dataset_2_10.npz"))
    n, query, db = int(g["n"]), g["query"].astype(np.float64), g["db"].astype(np.float64)
    cc = im.Context(im.default_params(), 0)
    try:
        cc.keygen(20250725)
        im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=99)
        receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
        other = np.random.default_rng(1).standard_normal(query.shape[0])
        gqs = [receiver.encryptQuery(query, seed=5, nonce=1), receiver.encryptQuery(other, seed=5, nonce=2)]
        idx = sender.indexScenarioMulti(gqs)
        mem = sender.membershipScenarioMulti(gqs)
        assert receiver.decryptIndex(idx[0]) == [0]
        assert receiver.decryptMembership(mem[0]) is True
        for q in range(2):
            assert np.array_equal(idx[q].export(), sender.indexScenario(gqs[q]).export())
            assert np.array_equal(mem[q].export(), sender.membershipScenario(gqs[q]).export())
    finally:
        cc.close()


def test_errors_leave_every_output_null(im, small):
    P, K, Or, _ = small
    cc = make_ctx(im, P)
    load_keys(cc, K)
    L = cc.L
    try:
        receiver = im.DiagonalReceiver(cc, 100)
        q1 = receiver.encryptQuery(np.ones(P.dim), seed=1, nonce=1)
        q2 = receiver.encryptQuery(np.ones(P.dim), seed=1, nonce=2)
        fns = (L.hydia_compute_similarity_multi, L.hydia_index_scenario_multi, L.hydia_membership_scenario_multi)

        def call(fn, hs, n):
            arr = (C.c_void_p * max(len(hs), 1))(*hs)
            out = (C.c_void_p * 4)(*([C.c_void_p(0x1234).value] * 4))
            code = fn(cc.h, arr, n, out)
            return code, [out[i] for i in range(4)]

        # no database resident: HYDIA_ERR_STATE
        for fn in fns:
            code, out = call(fn, [q1.h, q2.h], 2)
            assert code == -2 and out[:2] == [None, None]
        db = planted_db(P, 300, 1)
        im.DiagonalEnroller(cc, 300).serializeDB(db, seed=3)
        hers = im.HersReceiver(cc, 300).encryptQuery(np.ones(P.dim), seed=1)
        rescaled = receiver.encryptQuery(np.ones(P.dim), seed=1, nonce=3)
        assert L.hydia_rescale(cc.h, rescaled.h) == 0
        for fn in fns:
            code, _ = call(fn, [q1.h], 0)  # n_queries = 0
            assert code == -1
            code, out = call(fn, [q1.h, None, q2.h], 3)
            assert code == -1 and out[:3] == [None, None, None]
            code, out = call(fn, [q1.h, hers.h], 2)
            assert code == -1 and out[:2] == [None, None]
            code, out = call(fn, [rescaled.h, q2.h], 2)
            assert code == -1 and out[:2] == [None, None]
            code, out = call(fn, [q1.h, q2.h], 2)  # and the batch itself works
            assert code == 0 and all(out[:2])
            for h in out[:2]:
                L.hydia_ct_free(C.c_void_p(h))
    finally:
        cc.close()
