"""A plain query on the GPU (a known probe against the ENCRYPTED database, kinds 5 / 6; run with -m gpu).  Every comparison of
ciphertexts and plaintexts is np.array_equal against the restatement of the specification on the CPU oracle
(tests/plain_query_ref.py: the oracle's own sender path on the TRIVIAL ciphertext (encode(tiled normalised query), 0)) — bit for
bit, never against the product itself.  Ring: N = 2^11, 64-dim vectors (1024 slots, 64 ciphertexts per block), as in
tests/test_gpu_plain_gallery.py; one context at dim 512 for the 24-bit path over many diagonals, one at N = 2^15 without an oracle
run.  The GPU contexts hold NO rotation key 1 .. vector_dim-1 beyond the powers of two (EvalSum) and, at dim 64, the multiples of 8
(the giant steps of B = 8): the oracle rotates the trivial ciphertext with its full key set and gets the same bits."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
from plain_query_ref import ct_list, pattern_ct, pattern_db, pattern_poly, pattern_query, query_poly, trivial_query

pytestmark = pytest.mark.gpu
TOL = 1e-4  # the reference's own bound on decrypted scores
ERR_ARG, ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


# ---- contexts, one per (prime chain, vector_dim, key set), shared by the module
_CTX, _ORACLE = {}, {}


def chain_moduli(name):
    if name == "default":
        return None
    from test_gpu_loop_b_edges import chain  # the 47/48-bit chain ("evaluator") and the one with 59/60-bit scaling primes ("transform")
    return np.array([int(x) for x in chain(name).split(",")], dtype=np.uint64)


def pow2_rotations(slots):
    return [1 << k for k in range(slots.bit_length() - 1)]


def oracle_world(chain, dim, seed):
    """the oracle's parameters and FULL key set for (chain, dim): it rotates the trivial ciphertext with real keys"""
    key = (chain, dim)
    if key not in _ORACLE:
        moduli = chain_moduli(chain)
        if moduli is None:
            P = O.Params(log_n=11, depth=11, dim=dim)
        else:
            P = O.Params(log_n=11, depth=11, dim=dim, moduli=moduli, n_p=4)
        K = O.Keys(P, seed)
        _ORACLE[key] = (P, K, O.Oracle(P, K))
    return _ORACLE[key]


def world(im, chain="default", dim=64, seed=7, giants=True, bpp=2):
    """oracle with its full key set; GPU context with the power-of-two rotation keys and (giants, dim 64) the multiples of 8 only.
    bpp = 1: the context is created under HYDIA_TENSOR_BPP=1 (it reads the cap once), one database block per wave"""
    key = (chain, dim, giants) if bpp == 2 else (chain, dim, giants, bpp)
    P, K, Or = oracle_world(chain, dim, seed)
    if key not in _CTX:
        moduli = chain_moduli(chain)
        before = os.environ.get("HYDIA_TENSOR_BPP")
        if bpp != 2:
            os.environ["HYDIA_TENSOR_BPP"] = str(bpp)
        try:
            if moduli is None:
                cc = im.Context(im.default_params(log_n=11, vector_dim=dim), 0)
            else:
                cc = im.Context(im.default_params(log_n=11, vector_dim=dim), 0, moduli=moduli, roots=P.roots, n_p=4)
        finally:
            if bpp != 2:
                if before is None:
                    del os.environ["HYDIA_TENSOR_BPP"]
                else:
                    os.environ["HYDIA_TENSOR_BPP"] = before
        rots = set(pow2_rotations(P.slots))
        if giants and dim == 64:
            rots |= set(range(8, dim, 8))
        cc.keygen_rotations(sorted(rots), seed)
        for r in (3, 5, dim - 1):
            assert not cc.has_eval_key(r), r
        _CTX[key] = cc
    return P, K, Or, _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for cc in _CTX.values():
        cc.close()
    _CTX.clear()
    _ORACLE.clear()


@functools.lru_cache(maxsize=None)
def raw_rows(dim, blocks, slots):
    """`blocks` blocks - 3 rows of random templates with planted matches of the all-ones query in the first, a middle and the last
    block and one in every block (shared, never modified: every user takes a copy of a prefix)"""
    n = blocks * slots - 3
    rng = np.random.default_rng(100 + dim)
    db = rng.integers(-99, 100, size=(n, dim)).astype(np.float64)
    for i in (5, (blocks // 2) * slots + 100, n - 1):
        db[i] = rng.integers(1, 4, size=dim)
    for g in range(blocks):
        db[g * slots + 17] = rng.integers(1, 4, size=dim)
    db.setflags(write=False)
    return db


def cosines(rows):
    return (rows / np.maximum(np.linalg.norm(rows, axis=1, keepdims=True), 1e-300)) @ (np.ones(rows.shape[1]) / np.sqrt(rows.shape[1]))


def planted_in(rows):
    """the planted rows: their cosine with the all-ones query (about 0.93) clears the 0.44 threshold with room.  Random rows may lie
    near the threshold, so the index list is asked to CONTAIN these"""
    return {int(i) for i in np.nonzero(cosines(rows) > 0.8)[0]}


def take(dim, slots, blocks, ragged):
    src = raw_rows(dim, 16, slots)
    return src[:blocks * slots - (3 if ragged else 0)].copy()


def pq_kernels(chain, G, bpp=2):
    """the loop-B launches of a plain query over G loop-B blocks (blocks, or (block, giant step) pairs), as the byte ledger names them:
    tensor_split's blocks per wave / waves per workgroup, the split-diagonal kernel on limb 0 of <= 8 ciphertext-major blocks, one
    8-byte launch over all limbs on the unpacked transform chain, the 24-bit halves on a group-sequential layout"""
    B = 2 if bpp >= 2 and G % 2 == 0 else 1
    W = 4 if (G // B) % 4 == 0 else 2 if (G // B) % 2 == 0 else 1
    stream = lambda policy: "k_hydia_pq<%s, %d, %d>" % (policy, B, W)  # noqa: E731
    if chain == "transform":
        return {stream("Sums128<false>")}
    if G <= 8:
        return {"k_hydia_pq_sk<%d>" % (8 if G <= 2 else 4), stream("Sums128<true>")}
    return {stream("Sums128<false>"), stream("Halves24<true>" if chain == "default" else "Halves24<false>")}


def with_ledger(im, call):
    """call() and the loop-B kernels (encrypted, plain-gallery and plain-query ones alike) the byte ledger saw meanwhile"""
    im.byte_ledger(1)
    try:
        out = call()
    finally:
        led = im.byte_ledger(0)
    return out, {k for k in led if k.startswith("k_hydia_")}, led


def enrol(im, cc, rows, matvec, seed=99):
    cc.set_matvec(matvec)
    try:
        im.DiagonalEnroller(cc, rows.shape[0]).serializeDB(rows, seed=seed)
    finally:
        cc.set_matvec("auto")


# ------------------------------------------------------------------ 1. the plaintext handle
def test_encode_query_is_the_oracles_encoding_and_import_export_round_trips(im):
    P, K, Or, cc = world(im)
    sender = im.DiagonalSender(cc, 1)
    for query in (np.ones(P.dim), np.random.default_rng(3).uniform(-5, 5, P.dim), np.zeros(P.dim)):
        pt = sender.encodeQuery(query)
        assert isinstance(pt, im.Plaintext)
        assert np.array_equal(pt.export(), query_poly(P, query))
    for name in ("sat", "edge", "uniform"):
        m = pattern_poly(P, name)
        assert np.array_equal(cc.pt_import(m).export(), m), name


# ------------------------------------------------------------------ 2. scenarios, bit for bit, and what they decrypt to
def check_scenarios(im, P, Or, cc, rows, matvec, none_match=False, scenarios=("index", "membership")):
    n, G = rows.shape[0], -(-rows.shape[0] // P.slots)
    B = P.dim if matvec == "hoisted" else matvec
    a, b = rows.copy(), rows.copy()
    dbc = Or.enroll(a, 99, matvec=matvec)
    enrol(im, cc, b, matvec)
    assert np.array_equal(a, b) and cc.db_kind() == (6 if B < P.dim else 5) and cc.db_babies() == B
    for t in (0, G * P.dim - 1):
        assert np.array_equal(cc.db_export_ct(t), dbc[t].data()), t
    stats = cc.db_stats()
    query = np.ones(P.dim)
    q = trivial_query(P, query)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    pt = sender.encodeQuery(query)
    want = Or.compute_similarity(q, dbc, n)
    cc.kernel_time_reset()
    sim, ran, led = with_ledger(im, lambda: sender.computeSimilarity(pt))
    assert ran == pq_kernels("default", G * (P.dim // B)), sorted(ran)  # the plain-query kernels, and no k_hydia_tensor* / k_hydia_plain*
    assert led["k_automorph_batch"][0] == 1  # all rotations in ONE launch
    if B == P.dim:
        assert cc.kernel_time("ks_inner_product")[1] == 0  # no key switch anywhere in a hoisted computeSimilarity
    assert cc.kernel_time("hydia_pq")[1] == 1 and cc.kernel_time("hydia_tensor")[1] == 0
    got = sim.export()
    assert len(want) == G == len(got) and sim.shape()[1:] == (2, P.nQ - 1, want[0].scale)
    for g in range(G):
        assert np.array_equal(got[g], want[g].data()), g
    scores = cc.decrypt(sim).reshape(-1)[:n]
    assert np.abs(scores - a @ (query / np.linalg.norm(query))).max() < TOL
    if "index" in scenarios:
        want = Or.index_scenario(q, dbc, n)
        idx = sender.indexScenario(pt)
        got = idx.export()
        assert len(got) == G
        for g in range(G):
            assert np.array_equal(got[g], want[g].data()), g
        hits, planted = set(receiver.decryptIndex(idx)), planted_in(a)
        assert hits == set(Or.decrypt_index(want))
        assert (not hits and not planted) if none_match else (planted and planted <= hits)
    if "membership" in scenarios:
        want = Or.membership_scenario(q, dbc, n)
        mem = sender.membershipScenario(pt)
        assert np.array_equal(mem.export()[0], want.data())
        assert receiver.decryptMembership(mem) is (not none_match)
    assert cc.db_stats() == stats


@pytest.mark.parametrize("blocks,matvec", [(1, "hoisted"), (3, "hoisted"), (8, "hoisted"), (10, "hoisted"), (16, "hoisted"), (1, 8), (3, 8)],
                         ids=["1", "3", "8", "10", "16", "1-B8", "3-B8"])
def test_scenarios_equal_the_oracle_on_the_trivial_query(im, blocks, matvec):
    """1 .. 8 blocks: ciphertext-major (k_hydia_pq_sk on limb 0); 10 and 16: group-sequential, 46-bit (Halves24<true>, groups of 2 and
    8); B = 8: kind 6, giant steps with their real keys.  The last block is ragged where the database is the 16-block one."""
    P, K, Or, cc = world(im)
    check_scenarios(im, P, Or, cc, take(P.dim, P.slots, blocks, blocks == 16), matvec)
    if matvec == "hoisted" and blocks >= 10:
        assert (cc.db_group(), cc.db_residue_bits()) == ((8, 46) if blocks == 16 else (2, 46))


def test_membership_is_false_without_a_match(im):
    P, K, Or, cc = world(im)
    rng = np.random.default_rng(9)
    rows = rng.integers(-99, 100, size=(700, P.dim)).astype(np.float64)
    rows[cosines(rows) > 0.2] *= -1.0  # no row anywhere near the 0.44 threshold
    assert cosines(rows).max() <= 0.2
    check_scenarios(im, P, Or, cc, rows, "hoisted", none_match=True)


# ------------------------------------------------------------------ 3. the 24-bit path over 512 diagonals
def test_sixteen_blocks_at_dim_512(im):
    """group-sequential, 46-bit, 512 diagonals per block: two distinct encrypted blocks (the oracle's enrolment of two sets of rows)
    laid out in an irregular order through db_alloc / db_import_ct, so the oracle holds 1024 ciphertexts and not 8192"""
    P, K, Or, cc = world(im, dim=512)
    rng = np.random.default_rng(21)
    A = rng.integers(-99, 100, size=(P.slots, P.dim)).astype(np.float64)
    Bk = rng.integers(-99, 100, size=(P.slots, P.dim)).astype(np.float64)
    A[3] = rng.integers(1, 4, size=P.dim)
    Bk[1000] = rng.integers(1, 4, size=P.dim)
    enc = {"a": Or.enroll(A, 31, matvec="hoisted"), "b": Or.enroll(Bk, 32, matvec="hoisted")}  # normalise A, Bk in place
    order = "abbaaabababbbaab"
    n = len(order) * P.slots
    rows = np.concatenate([A if c == "a" else Bk for c in order])
    cc.db_alloc(n)
    cts = []
    for g, c in enumerate(order):
        for i in range(P.dim):
            ct = enc[c][i]
            cts.append(ct)
            cc.db_import_ct(g * P.dim + i, ct.data())
    assert cc.db_kind() == 5 and cc.db_group() == 8 and cc.db_residue_bits() == 46
    dbc = ct_list(cts, P.dim)
    query = np.ones(P.dim)
    q = trivial_query(P, query)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    pt = sender.encodeQuery(query)
    want = Or.compute_similarity(q, dbc, n)
    sim, ran, _ = with_ledger(im, lambda: sender.computeSimilarity(pt))
    assert ran == pq_kernels("default", 16), sorted(ran)
    got = sim.export()
    for g in range(16):
        assert np.array_equal(got[g], want[g].data()), g
    scores = cc.decrypt(sim).reshape(-1)[:n]
    assert np.abs(scores - rows @ (query / np.linalg.norm(query))).max() < TOL
    want = Or.index_scenario(q, dbc, n)
    idx = sender.indexScenario(pt)
    got = idx.export()
    for g in range(16):
        assert np.array_equal(got[g], want[g].data()), g
    hits, planted = set(receiver.decryptIndex(idx)), planted_in(rows)
    assert len(planted) == 16 and planted <= hits and hits == set(Or.decrypt_index(want))


# ------------------------------------------------------------------ 4. edges: an imported plaintext and database at the residues' bounds
EDGE_SHAPES = [(1, 1024), (8, 64), (16, 64), (16, 512)]
EDGE_PAIRS = ["sat/sat", "holes/holes", "sat/uniform", "uniform/sat", "edge/edge"]  # query / database, as tests/test_gpu_loop_b_edges.py pairs them


@pytest.mark.parametrize("pair", EDGE_PAIRS, ids=[p.replace("/", "-") for p in EDGE_PAIRS])
@pytest.mark.parametrize("blocks,dim", EDGE_SHAPES, ids=["%dx%d" % s for s in EDGE_SHAPES])
@pytest.mark.parametrize("chain", ["default", "evaluator", "transform"])
def test_saturated_and_edge_residues(im, chain, blocks, dim, pair):
    """every residue of the probe's plaintext and of both database polynomials at q_j - 1 (and the holes, uniform and 0, 1, q - 2,
    q - 1 patterns), through pt_import and db_alloc / db_import_ct, against Or.compute_similarity on the trivial ciphertext of the
    same plaintext.  default chain: 48-bit ciphertext-major up to 8 blocks, 46-bit group-sequential at 16; evaluator chain: 48-bit
    residues; transform chain: unpacked, folding sums on the 59/60-bit limbs.  The byte ledger says which instantiations ran."""
    check_edge_case(im, chain, blocks, dim, pair)


def check_edge_case(im, chain, blocks, dim, pair, bpp=2):
    P, K, Or, cc = world(im, chain, dim, giants=False, bpp=bpp)
    qname, mname = pair.split("/")
    n = blocks * P.slots
    pc = pattern_ct(P, mname)
    ct = pc.data().copy()  # (pc stays alive until the copy is made: data() is a view of the oracle's memory)
    cc.db_alloc(n)
    for t in range(blocks * P.dim):
        cc.db_import_ct(t, ct)
    bits = {"default": 46 if blocks > 8 else 48, "evaluator": 48, "transform": 64}[chain]
    assert cc.db_kind() == 5 and cc.db_residue_bits() == bits and cc.db_stats()[:2] == (n, blocks * P.dim)
    for t in (0, blocks * P.dim - 1):
        assert np.array_equal(cc.db_export_ct(t), ct)
    m = pattern_poly(P, qname)
    pt = cc.pt_import(m)
    assert np.array_equal(pt.export(), m)
    want = Or.compute_similarity(pattern_query(P, qname), pattern_db(P, mname, blocks * P.dim), n)
    sender = im.DiagonalSender(cc, n)
    sim, ran, _ = with_ledger(im, lambda: sender.computeSimilarity(pt))
    assert ran == pq_kernels(chain, blocks, bpp), sorted(ran)
    got = sim.export()
    assert len(want) == blocks
    for g in range(blocks):
        assert np.array_equal(got[g], want[g].data()), g


# the splits EDGE_SHAPES does not take (tensor_split picks blocks per wave and waves per workgroup from the block count and the context's
# cap alone), at dim 16.  Cap 2: 4 blocks (<., 2, 2>, also unpacked), 9 (groups of one block: <., 1, 1> on 46- and 48-bit halves), 10
# (Halves24<false> at <., 2, 1>), 12 (<., 2, 2> on both halves).  Cap 1 (HYDIA_TENSOR_BPP=1): 2 / 4 / 10 / 12 blocks -> one block per
# wave and two / four waves, for every arithmetic.  With them every k_hydia_pq / k_hydia_pq_sk instantiation the library ships is run
# by this file
OTHER_SPLITS = [("default", 4, 2), ("transform", 4, 2), ("default", 9, 2), ("evaluator", 9, 2), ("evaluator", 10, 2), ("default", 12, 2),
                ("evaluator", 12, 2), ("default", 2, 1), ("default", 4, 1), ("transform", 2, 1), ("transform", 4, 1), ("default", 10, 1),
                ("default", 12, 1), ("evaluator", 10, 1), ("evaluator", 12, 1)]


@pytest.mark.parametrize("chain,blocks,bpp", OTHER_SPLITS, ids=["%s-%d-bpp%d" % c for c in OTHER_SPLITS])
def test_saturated_residues_on_the_other_splits(im, chain, blocks, bpp):
    check_edge_case(im, chain, blocks, 16, "sat/sat", bpp)


# ------------------------------------------------------------------ 5. keys
def test_only_the_power_of_two_keys_are_needed_and_a_missing_giant_key_is_named(im):
    """a context with the power-of-two rotation keys alone: the hoisted scenarios match the oracle (which rotates with its full key
    set); on a B = 8 database giant key 24 is absent — ERR_STATE naming it, before any work, the database untouched"""
    P, K, Or, cc = world(im, giants=False)
    assert cc.has_eval_key(0) and cc.has_eval_key(8) and cc.has_eval_key(16) and not cc.has_eval_key(24)
    rows = take(P.dim, P.slots, 2, True)
    check_scenarios(im, P, Or, cc, rows, "hoisted")
    b = rows.copy()
    enrol(im, cc, b, 8)
    assert cc.db_kind() == 6 and cc.db_babies() == 8
    stats, sample = cc.db_stats(), cc.db_export_ct(P.dim + 5)
    sender = im.DiagonalSender(cc, rows.shape[0])
    pt = sender.encodeQuery(np.ones(P.dim))
    for call in (sender.computeSimilarity, sender.indexScenario, sender.membershipScenario):
        im.byte_ledger(1)
        try:
            with pytest.raises(im.HydiaError) as e:
                call(pt)
        finally:
            led = im.byte_ledger(0)
        assert e.value.code == ERR_STATE and "rotation key 24" in str(e.value), str(e.value)
        assert not led, sorted(led)  # nothing was enqueued
        assert cc.db_stats() == stats and cc.db_kind() == 6
    assert np.array_equal(cc.db_export_ct(P.dim + 5), sample)


def test_missing_relinearisation_and_power_of_two_keys_are_named(im):
    cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        cc.keygen_rotations([1, 2, 4, 8, 16, 32, 64, 128, 512], 7)  # 256 is absent
        rows = take(64, 1024, 1, False)[:200]
        enrol(im, cc, rows, "hoisted")
        sender = im.DiagonalSender(cc, 200)
        pt = sender.encodeQuery(np.ones(64))
        assert len(sender.indexScenario(pt)) == 1
        with pytest.raises(im.HydiaError) as e:
            sender.membershipScenario(pt)
        assert e.value.code == ERR_STATE and "rotation key 256" in str(e.value)
        # no evaluation key at all (a sender that was only handed the database): similarity is served and equals the oracle's bits
        P, K, Or = oracle_world("default", 64, 7)
        a = rows.copy()
        dbc = Or.enroll(a, 99, matvec="hoisted")
        cc2 = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
        try:
            cc2.db_alloc(200)
            for t in range(64):
                cc2.db_import_ct(t, dbc[t].data())
            assert not cc2.has_eval_key(0) and not cc2.has_eval_key(1)
            s2 = im.DiagonalSender(cc2, 200)
            p2 = s2.encodeQuery(np.ones(64))
            want = Or.compute_similarity(trivial_query(P, np.ones(64)), dbc, 200)
            assert np.array_equal(s2.computeSimilarity(p2).export()[0], want[0].data())
            for call in (s2.indexScenario, s2.membershipScenario):
                with pytest.raises(im.HydiaError) as e:
                    call(p2)
                assert e.value.code == ERR_STATE and "relinearisation key" in str(e.value)
            del p2
        finally:
            cc2.close()
        del pt
    finally:
        cc.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_database_alone(im):
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, 2, True)
    n = rows.shape[0]
    sender = im.DiagonalSender(cc, n)
    pt = sender.encodeQuery(np.ones(P.dim))
    three = (sender.computeSimilarity, sender.indexScenario, sender.membershipScenario)
    # a plain gallery, both forms: nothing would be private
    for matvec, kind in (("hoisted", 7), (8, 8)):
        cc.set_matvec(matvec)
        try:
            im.PlainEnroller(cc, n).serializeDB(rows.copy())
        finally:
            cc.set_matvec("auto")
        stats, sample = cc.db_stats(), cc.plain_db_export_pt(P.dim + 5)
        assert cc.db_kind() == kind
        for call in three:
            with pytest.raises(im.HydiaError) as e:
                call(pt)
            assert e.value.code == ERR_STATE and "kind 7 / 8" in str(e.value), str(e.value)
            assert cc.db_stats() == stats and cc.db_kind() == kind
        assert np.array_equal(cc.plain_db_export_pt(P.dim + 5), sample)
    # HERS' column packing (kind 4)
    im.HersEnroller(cc, 100).serializeDB(rows[:100].copy(), seed=5)
    stats = cc.db_stats()
    assert cc.db_kind() == 4
    for call in three:
        with pytest.raises(im.HydiaError) as e:
            call(pt)
        assert e.value.code == ERR_STATE and cc.db_stats() == stats and cc.db_kind() == 4
    # no database at all
    fresh = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        p0 = fresh.pt_import(pt.export())
        s0 = im.DiagonalSender(fresh, n)
        for call in (s0.computeSimilarity, s0.indexScenario, s0.membershipScenario):
            with pytest.raises(im.HydiaError) as e:
                call(p0)
            assert e.value.code == ERR_STATE and fresh.db_kind() == 0
        del p0
    finally:
        fresh.close()
    # an imported residue at or above its modulus: nothing is created
    good = pt.export()
    for j, v in ((0, int(P.moduli[0])), (P.nQ - 1, int(P.moduli[P.nQ - 1]) + 5), (1, 2 ** 64 - 1)):
        bad = good.copy()
        bad[j, 77] = v
        with pytest.raises(im.HydiaError) as e:
            cc.pt_import(bad)
        assert e.value.code == ERR_ARG, j
    # the batch and rotation methods do not take a Plaintext
    enrol(im, cc, rows.copy(), "hoisted")
    stats, sample = cc.db_stats(), cc.db_export_ct(7)
    for call in (lambda: sender.computeSimilarityMulti([pt, pt]), lambda: sender.indexScenarioMulti([pt]),
                 lambda: sender.membershipScenarioMulti([pt]), lambda: sender.computeSimilarityRotated(pt),
                 lambda: sender.indexScenarioRotated(pt), lambda: sender.rotateQuery(pt), lambda: sender.rotateQueryRange(pt, 0, 4)):
        with pytest.raises(im.HydiaError) as e:
            call()
        assert e.value.code == ERR_ARG
    assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(7), sample)


def test_a_plaintext_handle_keeps_its_context_alive(im):
    cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    m = np.arange(cc.nQ * cc.N, dtype=np.uint64).reshape(cc.nQ, cc.N) % np.uint64(1000)
    pt = cc.pt_import(m)
    L, h = cc.L, cc.h
    cc.close()  # deferred: the handle pins the context
    out = np.zeros_like(m)
    assert L.hydia_pt_export(h, pt.h, out.ctypes.data_as(ctypes.c_void_p)) == 0 and np.array_equal(out, m)
    del pt  # the last handle completes the destruction


# ------------------------------------------------------------------ 7. the full ring
def test_full_ring_two_blocks(im):
    """N = 2^15, dim 512, 2 blocks, hoisted and the auto form (B = 64, giant keys 64 .. 448): planted indices found and scores
    within 1e-4 of numpy (no oracle run at this size).  Rotation keys: the powers of two and the multiples of 64 only"""
    cc = im.Context(im.default_params(), 0)
    try:
        slots, dim = cc.N // 2, cc.dim
        cc.keygen_rotations(sorted(set(pow2_rotations(slots)) | set(range(64, dim, 64))), 11)
        n = 2 * slots - 5
        rng = np.random.default_rng(4)
        rows = rng.integers(-99, 100, size=(n, dim)).astype(np.float64)
        for i in (12, slots + 7, n - 1):
            rows[i] = rng.integers(1, 4, size=dim)
        want = planted_in(rows)
        assert len(want) == 3
        sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
        pt = sender.encodeQuery(np.ones(dim))
        for matvec in ("hoisted", "auto"):
            b = rows.copy()
            enrol(im, cc, b, matvec, seed=3)
            assert cc.db_kind() == (5 if matvec == "hoisted" else 6) and cc.db_stats()[:2] == (n, 2 * dim)
            if matvec == "auto":
                assert cc.db_babies() == 64
            scores = cc.decrypt(sender.computeSimilarity(pt)).reshape(-1)[:n]
            assert np.abs(scores - b @ (np.ones(dim) / np.sqrt(dim))).max() < TOL
            assert want <= set(receiver.decryptIndex(sender.indexScenario(pt)))
        del pt
    finally:
        cc.close()
