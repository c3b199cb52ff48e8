"""A plain gallery on the GPU (database kinds 7 / 8: an encrypted query against unencrypted templates; run with -m gpu).  Every
comparison of ciphertexts and plaintexts is np.array_equal against the restatement of the specification on the CPU oracle
(tests/plain_gallery_ref.py: the oracle's own sender path over TRIVIAL ciphertexts (encode(image_t), 0)) — bit for bit, never
against the product itself.  Ring: N = 2^11, 64-dim vectors (1024 slots, 64 plaintexts per block), as in tests/test_gpu_db_update.py;
one context at dim 512 for the 24-bit path over many diagonals, one at N = 2^15 without an oracle run."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from plain_gallery_ref import PlainRef, pattern_array, pattern_ct, pattern_poly

pytestmark = pytest.mark.gpu
TOL = 1e-4  # the reference's own bound on decrypted scores
ERR_ARG, ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


# ---- contexts, one per (prime chain, vector_dim), shared by the module
_CTX = {}


def chain_moduli(name):
    if name == "default":
        return None
    from test_gpu_loop_b_edges import chain  # the 47/48-bit chain ("evaluator") and the one with 59/60-bit scaling primes ("transform")
    return np.array([int(x) for x in chain(name).split(",")], dtype=np.uint64)


def world(im, chain="default", dim=64, seed=7):
    key = (chain, dim)
    if key not in _CTX:
        moduli = chain_moduli(chain)
        if moduli is None:
            P = O.Params(log_n=11, depth=11, dim=dim)
            cc = im.Context(im.default_params(log_n=11, vector_dim=dim), 0)
        else:
            P = O.Params(log_n=11, depth=11, dim=dim, moduli=moduli, n_p=4)
            cc = im.Context(im.default_params(log_n=11, vector_dim=dim), 0, moduli=moduli, roots=P.roots, n_p=4)
        K = O.Keys(P, seed)
        cc.keygen(seed)
        _CTX[key] = (P, K, O.Oracle(P, K), cc)
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for P, K, Or, cc in _CTX.values():
        cc.close()
    _CTX.clear()


@functools.lru_cache(maxsize=None)
def raw_rows(dim, blocks, slots):
    """`blocks` blocks - 3 rows of random templates with planted matches of the all-ones query in the first, a middle and the last
    block (shared, never modified: every user takes a copy of a prefix)"""
    n = blocks * slots - 3
    rng = np.random.default_rng(100 + dim)
    db = rng.integers(-99, 100, size=(n, dim)).astype(np.float64)
    for i in (5, (blocks // 2) * slots + 100, n - 1):
        db[i] = rng.integers(1, 4, size=dim)
    for g in range(blocks):  # one planted row in every block, so every prefix of whole blocks has some
        db[g * slots + 17] = rng.integers(1, 4, size=dim)
    db.setflags(write=False)
    return db


def cosines(rows):
    return (rows / np.maximum(np.linalg.norm(rows, axis=1, keepdims=True), 1e-300)) @ (np.ones(rows.shape[1]) / np.sqrt(rows.shape[1]))


def planted_in(rows):
    """the planted rows: their cosine with the all-ones query (about 0.93) clears the 0.44 threshold with room.  Random rows may lie
    near the threshold, so the index list is asked to CONTAIN these, as in tests/test_gpu_db_update.py"""
    return {int(i) for i in np.nonzero(cosines(rows) > 0.8)[0]}


def take(dim, slots, blocks, ragged):
    """a copy of the first `blocks` blocks of the shared rows (whole blocks, so that they share plaintexts with the larger galleries;
    ragged: the last 3 rows dropped)"""
    src = raw_rows(dim, 16, slots)
    n = blocks * slots - (3 if ragged else 0)
    return src[:n].copy()


def loop_b_kernels(chain, G):
    """the loop-B launches of a plain gallery of G loop-B blocks (blocks, or (block, giant step) pairs), as the byte ledger names
    them: tensor_split's blocks per wave / waves per workgroup, the split-diagonal kernel on limb 0 of <= 8 ciphertext-major blocks,
    one 8-byte launch over all limbs on the unpacked transform chain, the 24-bit halves on a group-sequential layout"""
    B = 2 if G % 2 == 0 else 1
    W = 4 if (G // B) % 4 == 0 else 2 if (G // B) % 2 == 0 else 1
    stream = lambda policy: "k_hydia_plain<%s, %d, %d>" % (policy, B, W)  # noqa: E731
    if chain == "transform":
        return {stream("Sums128<false>")}
    if G <= 8:
        return {"k_hydia_plain_sk<%d>" % (8 if G <= 2 else 4), stream("Sums128<true>")}
    return {stream("Sums128<false>"), stream("Halves24<true>" if chain == "default" else "Halves24<false>")}


def with_ledger(im, call):
    """call() and the loop-B kernels the byte ledger saw meanwhile"""
    im.byte_ledger(1)
    try:
        out = call()
    finally:
        led = im.byte_ledger(0)
    return out, {k for k in led if k.startswith("k_hydia_")}


def enrol_plain(im, cc, rows, matvec):
    cc.set_matvec(matvec)
    try:
        im.PlainEnroller(cc, rows.shape[0]).serializeDB(rows)
    finally:
        cc.set_matvec("auto")


# ------------------------------------------------------------------ enrolment
@pytest.mark.parametrize("blocks,ragged,matvec", [(0, False, "hoisted"), (2, True, "hoisted"), (10, False, "hoisted"), (16, True, "hoisted"),
                                                  (2, True, 8), (2, True, "auto"), (0, False, 8)],
                         ids=["n1", "ragged2", "blocks10", "blocks16", "ragged2-B8", "ragged2-auto", "n1-B8"])
def test_enrolment_matches_the_encoded_images(im, blocks, ragged, matvec):
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, blocks, ragged) if blocks else raw_rows(P.dim, 16, P.slots)[5:6].copy()
    n, G = rows.shape[0], max(blocks, 1)
    B = {"hoisted": P.dim, "auto": O.auto_babies(P.dim, G)}.get(matvec, matvec)
    # what an ENCRYPTED enrolment of the same rows takes: the gallery lies where it would, with one polynomial per entry
    cc.set_matvec(matvec)
    im.DiagonalEnroller(cc, n).serializeDB(rows.copy(), seed=3)
    cc.set_matvec("auto")
    enc = (cc.db_kind(), cc.db_babies(), cc.db_group(), cc.db_residue_bits(), cc.db_stats())
    assert enc[0] == (6 if B < P.dim else 5) and enc[1] == B
    a, b = rows.copy(), rows.copy()
    ref = PlainRef(P, Or, a, B)
    enrol_plain(im, cc, b, matvec)
    assert np.array_equal(a, b)  # both normalise the rows in place
    assert cc.db_kind() == enc[0] + 2 and cc.db_babies() == B
    assert cc.db_group() == enc[2] and cc.db_residue_bits() == enc[3]
    if matvec == "hoisted":
        assert (cc.db_group(), cc.db_residue_bits()) == ((8, 46) if G == 16 else (2, 46) if G == 10 else (0, 48))
    assert cc.db_stats() == (n, G * P.dim, enc[4][2] // 2) and enc[4][2] % 2 == 0 and enc[4][:2] == (n, G * P.dim)
    for g in range(G):
        for i in (0, P.dim // 2 - 1, P.dim - 1):
            t = g * P.dim + i
            assert np.array_equal(cc.plain_db_export_pt(t), ref.encode(t)), t


# ------------------------------------------------------------------ scenarios, bit for bit, and what they decrypt to
def check_scenarios(im, P, Or, cc, rows, matvec, none_match=False):
    n, G = rows.shape[0], -(-rows.shape[0] // P.slots)
    B = P.dim if matvec == "hoisted" else matvec
    a, b = rows.copy(), rows.copy()
    ref = PlainRef(P, Or, a, B)
    enrol_plain(im, cc, b, matvec)
    assert cc.db_kind() == (8 if B < P.dim else 7)
    query = np.ones(P.dim)
    q = Or.encrypt_query(query, 5, 1)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    gq = receiver.encryptQuery(query, seed=5, nonce=1)
    assert np.array_equal(gq.export()[0], q.data())
    arr = ref.array()
    want = Or.compute_similarity(q, arr, n)
    sim, ran = with_ledger(im, lambda: sender.computeSimilarity(gq))
    assert ran == loop_b_kernels("default", G * (P.dim // B)), sorted(ran)  # the plain kernels, and no encrypted one
    got = sim.export()
    assert len(want) == G == len(got)
    for g in range(G):
        assert np.array_equal(got[g], want[g].data()), g
    scores = cc.decrypt(sim).reshape(-1)[:n]
    assert np.abs(scores - a @ (query / np.linalg.norm(query))).max() < TOL
    want = Or.index_scenario(q, arr, n)
    idx = sender.indexScenario(gq)
    got = idx.export()
    for g in range(G):
        assert np.array_equal(got[g], want[g].data()), g
    hits, planted = set(receiver.decryptIndex(idx)), planted_in(a)
    assert hits == set(Or.decrypt_index(want))
    assert (not hits and not planted) if none_match else (planted and planted <= hits)
    want = Or.membership_scenario(q, arr, n)
    mem = sender.membershipScenario(gq)
    assert np.array_equal(mem.export()[0], want.data())
    assert receiver.decryptMembership(mem) is (not none_match)


@pytest.mark.parametrize("blocks,matvec", [(1, "hoisted"), (3, "hoisted"), (8, "hoisted"), (10, "hoisted"), (16, "hoisted"), (1, 8), (3, 8)],
                         ids=["1", "3", "8", "10", "16", "1-B8", "3-B8"])
def test_scenarios_equal_the_oracle_on_the_trivial_database(im, blocks, matvec):
    """1 .. 8 blocks: ciphertext-major (k_hydia_plain_sk on limb 0); 10 and 16: group-sequential, 46-bit (Halves24<true>, groups of
    2 and 8); B = 8: kind 8, the giant steps start at their key switch.  The last block is ragged where the gallery is the 16-block one."""
    P, K, Or, cc = world(im)
    check_scenarios(im, P, Or, cc, take(P.dim, P.slots, blocks, blocks == 16), matvec)


def test_membership_is_false_without_a_planted_row(im):
    P, K, Or, cc = world(im)
    rng = np.random.default_rng(9)
    rows = rng.integers(-99, 100, size=(700, P.dim)).astype(np.float64)
    rows[cosines(rows) > 0.2] *= -1.0  # no row anywhere near the 0.44 threshold
    assert cosines(rows).max() <= 0.2
    check_scenarios(im, P, Or, cc, rows, "hoisted", none_match=True)


def test_sixteen_blocks_at_dim_512(im):
    """the 24-bit halves over 512 diagonals per block (group-sequential, 46-bit): two distinct blocks of rows in an irregular order"""
    P, K, Or, cc = world(im, dim=512)
    rng = np.random.default_rng(21)
    A = rng.integers(-99, 100, size=(P.slots, P.dim)).astype(np.float64)
    Bk = rng.integers(-99, 100, size=(P.slots, P.dim)).astype(np.float64)
    A[3] = rng.integers(1, 4, size=P.dim)
    Bk[1000] = rng.integers(1, 4, size=P.dim)
    rows = np.ascontiguousarray(np.concatenate([A if c == "a" else Bk for c in "abbaaabababbbaab"]))
    check_scenarios(im, P, Or, cc, rows, "hoisted")
    assert cc.db_group() == 8 and cc.db_residue_bits() == 46


# ------------------------------------------------------------------ edges: imported plaintexts and a query at the residues' bounds
EDGE_SHAPES = [(1, 1024), (8, 64), (16, 64), (16, 512)]


EDGE_PAIRS = ["sat/sat", "holes/holes", "sat/uniform", "uniform/sat", "edge/edge"]  # query / gallery, as tests/test_gpu_loop_b_edges.py pairs them


@pytest.mark.parametrize("pair", EDGE_PAIRS, ids=[p.replace("/", "-") for p in EDGE_PAIRS])
@pytest.mark.parametrize("blocks,dim", EDGE_SHAPES, ids=["%dx%d" % s for s in EDGE_SHAPES])
@pytest.mark.parametrize("chain", ["default", "evaluator", "transform"])
def test_saturated_and_edge_residues(im, chain, blocks, dim, pair):
    """every plaintext residue and every residue of the query at q_j - 1 (and the holes, uniform and 0, 1, q - 2, q - 1 patterns),
    through plain_db_alloc / plain_db_import_pt / import_ct, against Or.compute_similarity on the same trivial ciphertexts.  default
    chain: 48-bit ciphertext-major up to 8 blocks, 46-bit group-sequential at 16; evaluator chain: 48-bit residues; transform chain:
    unpacked, folding sums on the 59/60-bit limbs.  The byte ledger says which instantiations ran."""
    check_edge_case(im, chain, blocks, dim, pair)


def check_edge_case(im, chain, blocks, dim, pair):
    P, K, Or, cc = world(im, chain, dim)
    qname, mname = pair.split("/")
    n = blocks * P.slots
    m = pattern_poly(P, mname)
    cc.plain_db_alloc(n, P.dim)
    for t in range(blocks * P.dim):
        cc.plain_db_import_pt(t, m)
    bits = {"default": 46 if blocks > 8 else 48, "evaluator": 48, "transform": 64}[chain]
    assert cc.db_kind() == 7 and cc.db_residue_bits() == bits and cc.db_stats()[:2] == (n, blocks * P.dim)
    for t in (0, blocks * P.dim - 1):
        assert np.array_equal(cc.plain_db_export_pt(t), m)
    q = pattern_ct(P, qname)
    gq = cc.import_ct(q.data(), q.scale)
    want = Or.compute_similarity(q, pattern_array(P, mname, blocks * P.dim), n)
    sender = im.DiagonalSender(cc, n)
    sim, ran = with_ledger(im, lambda: sender.computeSimilarity(gq))
    assert ran == loop_b_kernels(chain, blocks), sorted(ran)
    got = sim.export()
    assert len(want) == blocks
    for g in range(blocks):
        assert np.array_equal(got[g], want[g].data()), g


# the splits EDGE_SHAPES does not take (tensor_split picks blocks per wave and waves per workgroup from the block count alone), at dim 16:
# 2 and 4 blocks (<., 2, 1> and <., 2, 2>, the latter also unpacked), 9 (groups of one block: <., 1, 1> on 46- and 48-bit halves), 10
# (Halves24<false> at <., 2, 1>) and 12 (<., 2, 2> on both halves).  With them every k_hydia_plain / k_hydia_plain_sk instantiation the
# library ships is run by this file, except <., 1, 2> and <., 1, 4>: a gallery's cap is two blocks per wave (hk::PLAIN_BPP), so one block
# per wave means an odd block count, and that has no two waves
OTHER_SPLITS = [("default", 2), ("default", 4), ("transform", 4), ("default", 9), ("evaluator", 9), ("evaluator", 10), ("default", 12),
                ("evaluator", 12)]


@pytest.mark.parametrize("chain,blocks", OTHER_SPLITS, ids=["%s-%d" % c for c in OTHER_SPLITS])
def test_saturated_residues_on_the_other_splits(im, chain, blocks):
    check_edge_case(im, chain, blocks, 16, "sat/sat")


# ------------------------------------------------------------------ the full ring
def test_full_ring_two_blocks(im):
    """N = 2^15, dim 512, 2 blocks: enrol, query, planted indices found and scores within 1e-4 of numpy (no oracle run at this size)"""
    cc = im.Context(im.default_params(), 0)
    try:
        cc.keygen(11)
        slots, dim = cc.N // 2, cc.dim
        n = 2 * slots - 5
        rng = np.random.default_rng(4)
        rows = rng.integers(-99, 100, size=(n, dim)).astype(np.float64)
        for i in (12, slots + 7, n - 1):
            rows[i] = rng.integers(1, 4, size=dim)
        want = planted_in(rows)
        im.PlainEnroller(cc, n).serializeDB(rows)
        assert cc.db_kind() in (7, 8) and cc.db_babies() == cc.auto_babies(2) and cc.db_stats()[:2] == (n, 2 * dim)
        sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
        qc = receiver.encryptQuery(np.ones(dim), seed=5, nonce=1)
        scores = cc.decrypt(sender.computeSimilarity(qc)).reshape(-1)[:n]
        assert np.abs(scores - rows @ (np.ones(dim) / np.sqrt(dim))).max() < TOL
        assert len(want) == 3 and want <= set(receiver.decryptIndex(sender.indexScenario(qc)))
    finally:
        cc.close()


# ------------------------------------------------------------------ refusals
def test_out_of_scope_entry_points_are_refused_and_leave_the_gallery_alone(im, tmp_path):
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, 2, True)
    n = rows.shape[0]
    enrol_plain(im, cc, rows, "hoisted")
    stats, sample = cc.db_stats(), cc.plain_db_export_pt(P.dim + 5)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    qc = receiver.encryptQuery(np.ones(P.dim), seed=5, nonce=1)
    rot = sender.rotateQuery(qc)  # served: loop A does not look at the database
    assert len(rot.export()) == P.dim
    one = np.zeros((1, P.dim))
    one[0, 0] = 1.0
    ct = np.zeros((2, P.nQ, P.N), dtype=np.uint64)
    dev = rot.device_ptr()[0]
    refused = {
        "compute_similarity_multi": lambda: sender.computeSimilarityMulti([qc, qc]),
        "index_scenario_multi": lambda: sender.indexScenarioMulti([qc]),
        "membership_scenario_multi": lambda: sender.membershipScenarioMulti([qc, qc, qc]),
        "compute_similarity_rotated": lambda: sender.computeSimilarityRotated(rot),
        "index_scenario_rotated": lambda: sender.indexScenarioRotated(rot),
        "rotate_query_range": lambda: sender.rotateQueryRange(qc, 0, 4),
        "rotate_query_range_into": lambda: sender.rotateQueryRangeInto(qc, 0, 4, dev),
        "db_update": lambda: cc.db_update(n, one.copy(), True, seed=77),
        "db_update (replace)": lambda: cc.db_update(3, one.copy(), False, seed=78),
        "db_save": lambda: cc.db_save(tmp_path / "gallery.db"),
        "db_import_ct": lambda: cc.db_import_ct(0, ct),
        "db_export_ct": lambda: cc.db_export_ct(0),
        "db_set_babies": lambda: cc.db_set_babies(8),
    }
    for name, call in refused.items():
        with pytest.raises(im.HydiaError) as e:
            call()
        assert e.value.code == ERR_STATE and "plain gallery" in str(e.value), (name, str(e.value))
        assert cc.db_stats() == stats and cc.db_kind() == 7, name
    assert np.array_equal(cc.plain_db_export_pt(P.dim + 5), sample)
    assert not (tmp_path / "gallery.db").exists()
    # an imported residue at or above its modulus
    for j, v in ((0, int(P.moduli[0])), (P.nQ - 1, int(P.moduli[P.nQ - 1]) + 5), (1, 2 ** 64 - 1)):
        bad = sample.copy()
        bad[j, 77] = v
        with pytest.raises(im.HydiaError) as e:
            cc.plain_db_import_pt(P.dim + 5, bad)
        assert e.value.code == ERR_ARG, j
    assert np.array_equal(cc.plain_db_export_pt(P.dim + 5), sample) and cc.db_stats() == stats
    # a declared form must be vector_dim or a power of two >= 2 dividing it; without a plain gallery the plaintext calls are refused
    for babies in (0, 1, 3, 48, 128):
        with pytest.raises(im.HydiaError) as e:
            cc.plain_db_alloc(n, babies)
        assert e.value.code == ERR_ARG and cc.db_stats() == stats
    im.DiagonalEnroller(cc, 5).serializeDB(take(P.dim, P.slots, 1, False)[:5], seed=1)
    for call in (lambda: cc.plain_db_export_pt(0), lambda: cc.plain_db_import_pt(0, sample)):
        with pytest.raises(im.HydiaError) as e:
            call()
        assert e.value.code == ERR_STATE


def test_a_sharded_context_refuses_a_plain_gallery(im):
    """there is no hydia_group_* enrolment of a plain gallery: the shard contexts of a group and the Python role refuse it"""
    prm = im.default_params(log_n=11, vector_dim=64)
    grp = im.ShardGroup([0, 0], prm)
    try:
        rows = take(64, 1024, 1, False)[:100]
        with pytest.raises(im.HydiaError) as e:
            im.PlainEnroller(grp, 100)
        assert e.value.code == ERR_STATE and "plain gallery" in str(e.value)
        for r in (0, 1):
            cc = grp.shard_ctx(r)
            for call in (lambda: im.PlainEnroller(cc, 100).serializeDB(rows.copy()), lambda: cc.plain_db_alloc(100)):
                with pytest.raises(im.HydiaError) as e:
                    call()
                assert e.value.code == ERR_STATE and "plain gallery" in str(e.value)
            assert cc.db_kind() == 0 and cc.db_stats() == (0, 0, 0)
    finally:
        grp.close()


def test_alloc_declares_the_form_and_a_ciphertext_file_replaces_the_gallery(im, tmp_path):
    P, K, Or, cc = world(im)
    n = 3 * P.slots
    cc.plain_db_alloc(n, 8)
    assert (cc.db_kind(), cc.db_babies()) == (8, 8) and cc.db_stats()[:2] == (n, 3 * P.dim)
    assert not cc.plain_db_export_pt(3 * P.dim - 1).any()  # never imported: the zero polynomial
    cc.plain_db_alloc(n)
    assert (cc.db_kind(), cc.db_babies(), cc.db_group()) == (7, P.dim, 0)
    # hydia_db_load of a ciphertext file afterwards still works: it replaces the database
    rows = take(P.dim, P.slots, 1, False)[:300]
    cc.set_matvec("hoisted")
    try:
        im.DiagonalEnroller(cc, 300).serializeDB(rows.copy(), seed=9)
        first = cc.db_export_ct(7)
        cc.db_save(tmp_path / "enc.db")
        enrol_plain(im, cc, rows.copy(), "hoisted")
        assert cc.db_kind() == 7
        cc.db_load(tmp_path / "enc.db")
        assert cc.db_kind() == 5 and np.array_equal(cc.db_export_ct(7), first)
    finally:
        cc.set_matvec("auto")


# ------------------------------------------------------------------ existing kinds untouched
def test_an_encrypted_enrolment_after_a_plain_one_is_what_it_was(im):
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, 1, False)[:900]
    n = rows.shape[0]
    enrol_plain(im, cc, rows.copy(), "hoisted")
    assert cc.db_kind() == 7
    for matvec in ("hoisted", 8):
        a, b = rows.copy(), rows.copy()
        dbc = Or.enroll(a, 41, matvec=matvec)
        cc.set_matvec(matvec)
        try:
            im.DiagonalEnroller(cc, n).serializeDB(b, seed=41)
        finally:
            cc.set_matvec("auto")
        assert cc.db_kind() == (5 if matvec == "hoisted" else 6)
        for t in (0, P.dim // 2, P.dim - 1):
            assert np.array_equal(cc.db_export_ct(t), dbc[t].data()), t
        q = Or.encrypt_query(np.ones(P.dim), 5, 1)
        gq = cc.import_ct(q.data(), q.scale)
        sender = im.DiagonalSender(cc, n)
        sim, idx, mem = Or.compute_similarity(q, dbc, n), Or.index_scenario(q, dbc, n), Or.membership_scenario(q, dbc, n)
        assert np.array_equal(sender.computeSimilarity(gq).export()[0], sim[0].data())
        assert np.array_equal(sender.indexScenario(gq).export()[0], idx[0].data())
        assert np.array_equal(sender.membershipScenario(gq).export()[0], mem.data())
        enrol_plain(im, cc, rows.copy(), matvec)  # and back: the next round starts from a plain gallery again
