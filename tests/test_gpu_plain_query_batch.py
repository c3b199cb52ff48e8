"""A BATCH of plain queries on the GPU (hydia_*_pq_multi, DiagonalSender.*PlainMulti; run with -m gpu): several known probes against the
ENCRYPTED database in one pass.  The contract is "per query exactly what the single call returns", so most comparisons here are
np.array_equal of every exported limb against the single calls (which tests/test_gpu_plain_query.py holds to the oracle), with queries
that are DISTINCT and have distinct answers; one batch per form is also held to the oracle directly.  Ring and helpers: those of
tests/test_gpu_plain_query.py (N = 2^11, dim 64, 1024 slots, the three prime chains).

Loop B of a batch runs the k_hydia_pq_mq family.  Instantiated and launchable: k_hydia_pq_mq<A, QW, NW> for A in Sums128<false>,
Sums128<true>, Halves24<true>, QW in 1, 2, 4, NW in 1, 2, 4, 8, and k_hydia_pq_mq_sk<KS, QW> for KS in 4, 8, QW in 1, 2, 4 — 42 kernels,
every one of which test_every_instantiation_runs_once launches.  Never launched, and therefore not instantiated:
k_hydia_pq_mq<Halves24<false>, *, *> (a batch keeps the 128-bit sums on the 48-bit group-sequential layouts where a single query takes
the 24-bit halves, as the encrypted batch does).  The library's own width is 4, the measured choice
(profiles/plain_query_batch/README.md); Context.set_pq_batch_width narrows it for a measurement or a test."""
import ctypes

import numpy as np
import pytest

import test_gpu_plain_query as base
from plain_query_ref import pattern_ct, pattern_poly, trivial_query
from test_gpu_plain_query import ERR_ARG, ERR_STATE, TOL, enrol, pow2_rotations, take, with_ledger, world

pytestmark = pytest.mark.gpu
WIDTH = 4  # hydia_pq_mq_width: queries per database pass of a batch as shipped


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """world() keeps its contexts in the plain-query module's table: what this module opened there is closed here"""
    yield
    for cc in list(base._CTX.values()) + list(_OWN.values()):
        cc.close()
    base._CTX.clear()
    base._ORACLE.clear()
    _OWN.clear()


_OWN = {}
SCENARIOS = ("computeSimilarity", "indexScenario", "membershipScenario")


def multi_of(sender, name):
    return getattr(sender, name + "PlainMulti")


def exported(ct):
    return np.asarray(ct.export())


def schedule(Q, width):
    """the widths of a batch's passes: the widest power of two up to `width` that what is left still fills"""
    out, left, w = [], Q, width
    while left:
        while w > left:
            w //= 2
        out.append(w)
        left -= w
    return out


def mq_kernels(layout, G, Q, width):
    """{ledger name: launches} of a batch's loop B over G loop-B blocks on the resident layout, in the launcher's words: one block per
    wave; layout = resident(cc) or what the case expects; workgroup = the layout's group, else 4 / 2 / 1 waves by divisibility of G;
    8-byte layouts one launch over all limbs; packed ones limb 0 (split-diagonal for <= 8 ciphertext-major blocks) and the rest (46-bit
    halves, else the 128-bit sums) separately"""
    seq, bits = layout  # (blocks per group of a group-sequential layout or 0, bits per stored residue of limbs 1..)
    W = seq if seq else 4 if G % 4 == 0 else 2 if G % 2 == 0 else 1
    want = {}
    for qw in schedule(Q, width):
        stream = lambda policy: "k_hydia_pq_mq<%s, %d, %d>" % (policy, qw, W)  # noqa: E731
        if bits == 64:
            names = [stream("Sums128<false>")]
        else:
            first = "k_hydia_pq_mq_sk<%d, %d>" % (8 if G <= 2 else 4, qw) if not seq and G <= 8 else stream("Sums128<false>")
            names = [first, stream("Halves24<true>" if bits == 46 else "Sums128<true>")]
        for n in names:
            want[n] = want.get(n, 0) + 1
    return want


def resident(cc):
    return cc.db_group(), cc.db_residue_bits()


def launches(led):
    return {k: v[0] for k, v in led.items() if k.startswith("k_hydia_")}


def distinct_queries(P, rows, Q=5):
    """Q sign patterns, pairwise nearly orthogonal, and rows planted for each of them alone in the first and the last block: the
    match / no-match answers of those 2 Q rows differ between any two queries.  -> (queries [Q][dim], planted: list of row sets)"""
    rng = np.random.default_rng(77)
    while True:
        v = rng.choice([-1.0, 1.0], size=(Q, P.dim))
        c = np.abs(v @ v.T) / P.dim - np.eye(Q)
        if c.max() < 0.3 and np.abs(v.sum(axis=1)).max() / P.dim < 0.3:  # (nor near the all-ones rows the shared database carries)
            break
    n = rows.shape[0]
    planted = []
    for k in range(Q):
        mine = {11 * k + 3, n - 1 - k}
        for r in mine:
            rows[r] = v[k] * rng.integers(1, 4, size=P.dim)
        planted.append(mine)
    return v, planted


def assert_batches_equal_singles(im, P, cc, sender, pts, singles, sizes, G_loop, scenarios=SCENARIOS):
    for name in scenarios:
        for Q in sizes:
            cc.kernel_time_reset()
            res, _, led = with_ledger(im, lambda: multi_of(sender, name)(pts[:Q]))
            assert launches(led) == mq_kernels(resident(cc), G_loop, Q, WIDTH), (name, Q, sorted(launches(led).items()))
            assert led["k_automorph_batch"][0] == Q  # one launch per query
            assert cc.kernel_time("hydia_pq_multi")[1] == 1 and cc.kernel_time("hydia_pq")[1] == 0
            assert len(res) == Q
            for q in range(Q):
                got = exported(res[q])
                assert got.shape == singles[name][q].shape and np.array_equal(got, singles[name][q]), (name, Q, q)


def run_singles(im, sender, pts, scenarios=SCENARIOS):
    singles = {}
    for name in scenarios:
        singles[name] = []
        for pt in pts:
            r, ran, _ = with_ledger(im, lambda: getattr(sender, name)(pt))
            assert ran and all(k.startswith("k_hydia_pq<") or k.startswith("k_hydia_pq_sk<") for k in ran), sorted(ran)
            singles[name].append(exported(r))
        for a in range(len(pts)):
            for b in range(a):
                assert not np.array_equal(singles[name][a], singles[name][b]), (name, a, b)
    return singles


# ------------------------------------------------------------------ 1. a batch equals the single calls, bit for bit
@pytest.mark.parametrize("matvec", ["hoisted", 8], ids=["hoisted", "B8"])
@pytest.mark.parametrize("blocks", [1, 3, 10])
@pytest.mark.parametrize("chain", ["default", "evaluator", "transform"])
def test_batches_equal_single_calls(im, chain, blocks, matvec):
    """1 block: split kernel KS = 8 on limb 0 (hoisted); 3: KS = 4; 10: streaming on a group-sequential layout; B = 8 multiplies the
    loop-B blocks by 8 giants.  Q = 1, 2, 3, 5: passes of 1, of 2, of 2 + 1, of 4 + 1 — every width shipped, a remainder, more than one
    pass.  The last block is ragged"""
    P, K, Or, cc = world(im, chain)
    rows = take(P.dim, P.slots, blocks, True)
    vecs, planted = distinct_queries(P, rows)
    n = rows.shape[0]
    enrol(im, cc, rows, matvec)
    B = P.dim if matvec == "hoisted" else matvec
    assert cc.db_kind() == (6 if B < P.dim else 5)
    stats, sample = cc.db_stats(), cc.db_export_ct(5)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    pts = sender.encodeQueries(vecs)
    assert len(pts) == 5 and all(np.array_equal(pts[k].export(), sender.encodeQuery(vecs[k]).export()) for k in range(5))
    singles = run_singles(im, sender, pts)
    assert_batches_equal_singles(im, P, cc, sender, pts, singles, (1, 2, 3, 5), blocks * (P.dim // B))
    if chain == "default":  # what the batch decrypts to: every query finds its own planted rows and none of another query's
        idx = sender.indexScenarioPlainMulti(pts)
        mem = sender.membershipScenarioPlainMulti(pts)
        for k in range(5):
            hits = set(receiver.decryptIndex(idx[k]))
            assert planted[k] <= hits, k
            assert not any(hits & planted[j] for j in range(5) if j != k), k
            assert receiver.decryptMembership(mem[k]) is True
    assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(5), sample)


@pytest.mark.parametrize("env,bits", [("HYDIA_DB_UNPACKED", 64), ("HYDIA_DB_48BIT", 48)])
def test_fallback_layouts(im, env, bits, monkeypatch):
    """10 blocks under HYDIA_DB_UNPACKED (8-byte residues, ciphertext-major: one launch over all limbs) and HYDIA_DB_48BIT
    (group-sequential with 6-byte residues: the batch keeps the 128-bit sums where a single query takes Halves24<false>)"""
    P, K, Or, _ = world(im)
    if env not in _OWN:
        monkeypatch.setenv(env, "1")
        cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
        cc.keygen_rotations(pow2_rotations(P.slots), 7)
        _OWN[env] = cc
    cc = _OWN[env]
    rows = take(P.dim, P.slots, 10, True)
    vecs, planted = distinct_queries(P, rows, 3)
    enrol(im, cc, rows, "hoisted")
    assert cc.db_kind() == 5 and cc.db_residue_bits() == bits and cc.db_group() == (2 if bits == 48 else 0)
    sender = im.DiagonalSender(cc, rows.shape[0])
    pts = sender.encodeQueries(vecs)
    singles = run_singles(im, sender, pts, ("computeSimilarity", "indexScenario"))
    assert_batches_equal_singles(im, P, cc, sender, pts, singles, (3,), 10, ("computeSimilarity", "indexScenario"))


# ------------------------------------------------------------------ 2. a batch against the oracle on the trivial ciphertexts
@pytest.mark.parametrize("matvec", ["hoisted", 8], ids=["hoisted", "B8"])
def test_a_batch_of_three_equals_the_oracle(im, matvec):
    """the expectation is the reference path on (encode(q), 0) (tests/plain_query_ref.py), per query, bit for bit"""
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, 3, True)
    vecs, planted = distinct_queries(P, rows, 3)
    n = rows.shape[0]
    a, b = rows.copy(), rows.copy()
    dbc = Or.enroll(a, 99, matvec=matvec)
    enrol(im, cc, b, matvec)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    pts = sender.encodeQueries(vecs)
    qs = [trivial_query(P, v) for v in vecs]
    sim, idx, mem = sender.computeSimilarityPlainMulti(pts), sender.indexScenarioPlainMulti(pts), sender.membershipScenarioPlainMulti(pts)
    for k in range(3):
        want = Or.compute_similarity(qs[k], dbc, n)
        got = sim[k].export()
        assert len(got) == len(want) == 3
        for g in range(3):
            assert np.array_equal(got[g], want[g].data()), (k, g)
        scores = cc.decrypt(sim[k]).reshape(-1)[:n]
        assert np.abs(scores - a @ (vecs[k] / np.linalg.norm(vecs[k]))).max() < TOL
        want = Or.index_scenario(qs[k], dbc, n)
        got = idx[k].export()
        for g in range(3):
            assert np.array_equal(got[g], want[g].data()), (k, g)
        hits = set(receiver.decryptIndex(idx[k]))
        assert planted[k] <= hits and hits == set(Or.decrypt_index(want))
        want = Or.membership_scenario(qs[k], dbc, n)
        assert np.array_equal(mem[k].export()[0], want.data()), k
        assert receiver.decryptMembership(mem[k]) is True


# ------------------------------------------------------------------ 3. saturated operands
SAT_SHAPES = [(8, 64), (16, 64), (1, 1024)]  # dim 1024 = every slot: the largest the ring allows; the 59/60-bit limbs fold every 128 / 32 diagonals


@pytest.mark.parametrize("blocks,dim", SAT_SHAPES, ids=["%dx%d" % s for s in SAT_SHAPES])
@pytest.mark.parametrize("chain", ["default", "evaluator", "transform"])
def test_saturated_operands(im, chain, blocks, dim):
    """every residue of three plaintexts (pt_import) and of both polynomials of every database ciphertext (db_import_ct) at q_j - 1: a
    batch of 3 equals the three single calls (which tests/test_gpu_plain_query.py holds to the oracle on these operands)"""
    P, K, Or, cc = world(im, chain, dim, giants=False)
    n = blocks * P.slots
    pc = pattern_ct(P, "sat")
    ct = pc.data().copy()
    cc.db_alloc(n)
    for t in range(blocks * P.dim):
        cc.db_import_ct(t, ct)
    m = pattern_poly(P, "sat")
    assert all((m[j] == P.moduli[j] - np.uint64(1)).all() for j in range(P.nQ))
    pts = [cc.pt_import(m) for _ in range(3)]
    sender = im.DiagonalSender(cc, n)
    single = exported(sender.computeSimilarity(pts[0]))
    res, _, led = with_ledger(im, lambda: sender.computeSimilarityPlainMulti(pts))
    assert launches(led) == mq_kernels(resident(cc), blocks, 3, WIDTH), sorted(launches(led).items())
    for q in range(3):
        assert np.array_equal(exported(res[q]), single), q
    # and beside a probe that is not saturated, in every position of the pass
    u = cc.pt_import(pattern_poly(P, "uniform"))
    single_u = exported(sender.computeSimilarity(u))
    assert not np.array_equal(single_u, single)
    for order in ([u, pts[0], pts[1]], [pts[0], u, pts[1]], [pts[0], pts[1], u]):
        res = sender.computeSimilarityPlainMulti(order)
        for q, pt in enumerate(order):
            assert np.array_equal(exported(res[q]), single_u if pt is u else single), q


# ------------------------------------------------------------------ 4. every instantiation, at dim 16
PATTERNS = ("sat", "holes", "uniform", "edge")
# (chain, blocks) -> layout: default 1, 2: split KS = 8 + Sums128<true> at 1 / 2 waves; 4: KS = 4 + 4 waves; 9, 10, 12, 16: groups of 1, 2, 4, 8
# blocks, 46-bit (Sums128<false> on limb 0 + Halves24<true>); evaluator 16: groups of 8, 48-bit (Sums128<true> at 8 waves); transform 1,
# 2, 4: 8-byte residues, Sums128<false> over all limbs at 1, 2, 4 waves
INSTANCES = [("default", 1, (0, 48)), ("default", 2, (0, 48)), ("default", 4, (0, 48)), ("default", 9, (1, 46)), ("default", 10, (2, 46)),
             ("default", 12, (4, 46)), ("default", 16, (8, 46)), ("evaluator", 16, (8, 48)), ("transform", 1, (0, 64)), ("transform", 2, (0, 64)),
             ("transform", 4, (0, 64))]


def test_the_instances_cover_every_instantiation():
    """what the cases below assert the ledger to name (a batch of 7 at width 4: QW = 4, 2, 1) is all 42 kernels of the family"""
    every = {"k_hydia_pq_mq<%s, %d, %d>" % (a, qw, nw) for a in ("Sums128<false>", "Sums128<true>", "Halves24<true>") for qw in (1, 2, 4)
             for nw in (1, 2, 4, 8)} | {"k_hydia_pq_mq_sk<%d, %d>" % (ks, qw) for ks in (4, 8) for qw in (1, 2, 4)}
    named = set()
    for chain, blocks, layout in INSTANCES:
        named |= set(mq_kernels(layout, blocks, 7, 4))
    assert named == every, sorted(every ^ named)


@pytest.mark.parametrize("chain,blocks,layout", INSTANCES, ids=["%s-%d" % c[:2] for c in INSTANCES])
def test_every_instantiation_runs_once(im, chain, blocks, layout):
    """a batch of 7 at the shipped width is passes of 4, 2 and 1 queries: all three QW of the layout's kernels in one call, against
    single calls, the ledger naming ceil(7 / 4) + 1 = 3 passes; then narrowed to width 2, where it shows ceil(7 / 2) = 4.  The blocks differ from their neighbours (patterns in a
    rotating order), so does every query from the next"""
    P, K, Or, cc = world(im, chain, 16, giants=False)
    n = blocks * P.slots
    cts = {name: pattern_ct(P, name).data().copy() for name in PATTERNS}
    cc.db_alloc(n)
    for g in range(blocks):
        for i in range(P.dim):
            cc.db_import_ct(g * P.dim + i, cts[PATTERNS[(g + g // 4) % 4]])
    assert resident(cc) == layout
    pats = [cc.pt_import(pattern_poly(P, name)) for name in PATTERNS]
    sender = im.DiagonalSender(cc, n)
    single = []
    for pt in pats:
        r, ran, _ = with_ledger(im, lambda: sender.computeSimilarity(pt))
        assert ran and all(k.startswith("k_hydia_pq<") or k.startswith("k_hydia_pq_sk<") for k in ran), sorted(ran)  # a single call is untouched
        single.append(exported(r))
    assert all(not np.array_equal(single[a], single[b]) for a in range(4) for b in range(a))
    order = [0, 2, 1, 3, 2, 0, 1]
    batch = [pats[k] for k in order]
    for width in (0, 2):
        cc.set_pq_batch_width(width)
        try:
            res, _, led = with_ledger(im, lambda: sender.computeSimilarityPlainMulti(batch))
        finally:
            cc.set_pq_batch_width(0)
        want = mq_kernels(layout, blocks, 7, width or WIDTH)
        assert launches(led) == want, sorted(launches(led).items())
        assert schedule(7, width or WIDTH) == ([2, 2, 2, 1] if width else [4, 2, 1])
        for q, k in enumerate(order):
            assert np.array_equal(exported(res[q]), single[k]), (width, q)
    with pytest.raises(im.HydiaError) as e:
        cc.set_pq_batch_width(3)
    assert e.value.code == ERR_ARG


# ------------------------------------------------------------------ 5. refusals
def c_call(cc, name, handles, n=None):
    """the C entry point itself: (code, outputs), the outputs pre-set to a non-NULL value"""
    n = len(handles) if n is None else n
    hs = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    out = (ctypes.c_void_p * max(n, 1))(*([1] * max(n, 1)))
    code = getattr(cc.L, name)(cc.h, hs, n, out)
    return code, [out[i] for i in range(n)]


C_NAMES = {"computeSimilarity": "hydia_compute_similarity_pq_multi", "indexScenario": "hydia_index_scenario_pq_multi",
           "membershipScenario": "hydia_membership_scenario_pq_multi"}


def assert_refused(im, cc, sender, pts, code, scenarios=SCENARIOS, same_as_single=None):
    """both ways in: the role raises HydiaError(code) (with the single call's message where there is one), the C entry answers the
    code and leaves every output NULL; nothing is enqueued"""
    for name in scenarios:
        im.byte_ledger(1)
        try:
            with pytest.raises(im.HydiaError) as e:
                multi_of(sender, name)(pts)
            got, outs = c_call(cc, C_NAMES[name], [p.h for p in pts])
        finally:
            led = im.byte_ledger(0)
        assert e.value.code == code and got == code, (name, e.value.code, got, str(e.value))
        assert all(o is None for o in outs), name
        assert not led, sorted(led)
        if same_as_single is not None:
            with pytest.raises(im.HydiaError) as e1:
                getattr(sender, name)(same_as_single)
            assert e1.value.code == code and str(e1.value) == str(e.value), (str(e1.value), str(e.value))


def test_refusals_leave_the_database_alone(im):
    """every ERR_ARG and ERR_STATE of the table, through the C entry points and the roles.  A plaintext that is not at full level is
    one made on a context with a shorter chain (mult_depth 10: 11 limbs): handles are not tied to the context they are passed to, so
    Context::pq_check is what refuses it"""
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, 2, True)
    n = rows.shape[0]
    sender = im.DiagonalSender(cc, n)
    pts = sender.encodeQueries(np.stack([np.ones(P.dim), -np.ones(P.dim)]))
    enrol(im, cc, rows.copy(), "hoisted")
    stats, sample = cc.db_stats(), cc.db_export_ct(7)
    # an empty batch, a NULL handle, unequal scales, a ciphertext in the list
    for name in SCENARIOS:
        with pytest.raises(im.HydiaError) as e:
            multi_of(sender, name)([])
        assert e.value.code == ERR_ARG
        assert c_call(cc, C_NAMES[name], [], 0)[0] == ERR_ARG
        assert c_call(cc, C_NAMES[name], [pts[0].h, None]) == (ERR_ARG, [None, None])
        assert c_call(cc, C_NAMES[name], [None]) == (ERR_ARG, [None])
        assert getattr(cc.L, C_NAMES[name])(None, None, 1, None) == ERR_ARG
    other = cc.pt_import(pts[0].export(), scale=cc.delta * 2.0)
    assert_refused(im, cc, sender, [pts[0], other], ERR_ARG)
    assert_refused(im, cc, sender, [other, pts[0], pts[1]], ERR_ARG)
    # a plaintext that is not at full level: in the first position and in a later one
    shorter = im.Context(im.default_params(log_n=11, vector_dim=64, mult_depth=10), 0)
    try:
        assert shorter.nQ == cc.nQ - 1 and shorter.N == cc.N
        low = [im.DiagonalSender(shorter, n).encodeQuery(np.ones(P.dim)), shorter.pt_import(pts[1].export()[:shorter.nQ] % shorter.moduli[:shorter.nQ, None])]
        for batch in ([low[0], pts[0]], [pts[0], pts[1], low[0]], [pts[0], low[1]], [low[1]]):
            assert_refused(im, cc, sender, batch, ERR_ARG)
        assert_refused(im, cc, sender, [low[0], pts[1]], ERR_ARG, same_as_single=low[0])
        with pytest.raises(im.HydiaError) as e:
            sender.indexScenarioPlainMulti([pts[0], low[0]])
        assert "full level" in str(e.value)
        assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(7), sample)
        del low
    finally:
        shorter.close()
    qc = im.DiagonalReceiver(cc, n).encryptQuery(np.ones(P.dim), seed=5, nonce=1)
    for name in SCENARIOS:
        with pytest.raises(im.HydiaError) as e:
            multi_of(sender, name)([pts[0], qc])
        assert e.value.code == ERR_ARG
    with pytest.raises(im.HydiaError) as e:  # the encrypted batch methods still refuse a Plaintext
        sender.indexScenarioMulti([pts[0]])
    assert e.value.code == ERR_ARG
    assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(7), sample)
    assert len(sender.indexScenarioPlainMulti(pts)) == 2  # and the batch is served
    # a plain gallery, both forms
    for matvec, kind in (("hoisted", 7), (8, 8)):
        cc.set_matvec(matvec)
        try:
            im.PlainEnroller(cc, n).serializeDB(rows.copy())
        finally:
            cc.set_matvec("auto")
        stats, sample = cc.db_stats(), cc.plain_db_export_pt(P.dim + 5)
        assert cc.db_kind() == kind
        assert_refused(im, cc, sender, pts, ERR_STATE, same_as_single=pts[0])
        assert cc.db_stats() == stats and cc.db_kind() == kind and np.array_equal(cc.plain_db_export_pt(P.dim + 5), sample)
    # HERS' column packing (kind 4)
    im.HersEnroller(cc, 100).serializeDB(rows[:100].copy(), seed=5)
    stats = cc.db_stats()
    assert cc.db_kind() == 4
    assert_refused(im, cc, sender, pts, ERR_STATE, same_as_single=pts[0])
    assert cc.db_stats() == stats and cc.db_kind() == 4
    # no database at all
    fresh = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        p0 = [fresh.pt_import(p.export()) for p in pts]
        s0 = im.DiagonalSender(fresh, n)
        assert_refused(im, fresh, s0, p0, ERR_STATE, same_as_single=p0[0])
        assert fresh.db_kind() == 0
        del p0
    finally:
        fresh.close()


def test_missing_keys_are_named_before_any_work(im):
    """a giant-step key (B = 8 database on a context without the multiples of 8), a power-of-two key, the relinearisation key: the
    single call's ERR_STATE and message, nothing enqueued, the database as it was"""
    P, K, Or, cc = world(im, giants=False)
    rows = take(P.dim, P.slots, 2, True)
    n = rows.shape[0]
    enrol(im, cc, rows.copy(), 8)
    assert cc.db_kind() == 6 and not cc.has_eval_key(24)
    stats, sample = cc.db_stats(), cc.db_export_ct(P.dim + 5)
    sender = im.DiagonalSender(cc, n)
    pts = sender.encodeQueries(np.stack([np.ones(P.dim), -np.ones(P.dim), np.ones(P.dim)]))
    assert_refused(im, cc, sender, pts, ERR_STATE, same_as_single=pts[0])
    with pytest.raises(im.HydiaError) as e:
        sender.computeSimilarityPlainMulti(pts)
    assert "rotation key 24" in str(e.value)
    assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(P.dim + 5), sample)
    cc2 = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        cc2.keygen_rotations([1, 2, 4, 8, 16, 32, 64, 128, 512], 7)  # 256 is absent
        enrol(im, cc2, take(64, 1024, 1, False)[:200], "hoisted")
        s2 = im.DiagonalSender(cc2, 200)
        p2 = s2.encodeQueries(np.stack([np.ones(64), -np.ones(64)]))
        assert len(s2.indexScenarioPlainMulti(p2)) == 2
        assert_refused(im, cc2, s2, p2, ERR_STATE, ("membershipScenario",), same_as_single=p2[0])
        with pytest.raises(im.HydiaError) as e:
            s2.membershipScenarioPlainMulti(p2)
        assert "rotation key 256" in str(e.value)
        sample = cc2.db_export_ct(3)
        cc3 = im.Context(im.default_params(log_n=11, vector_dim=64), 0)  # no evaluation key at all
        try:
            cc3.db_alloc(200)
            for t in range(64):
                cc3.db_import_ct(t, cc2.db_export_ct(t))
            s3 = im.DiagonalSender(cc3, 200)
            p3 = s3.encodeQueries(np.stack([np.ones(64), -np.ones(64)]))
            sim = s3.computeSimilarityPlainMulti(p3)  # similarity needs no key
            assert np.array_equal(exported(sim[1]), exported(s3.computeSimilarity(p3[1])))
            assert_refused(im, cc3, s3, p3, ERR_STATE, ("indexScenario", "membershipScenario"), same_as_single=p3[0])
            with pytest.raises(im.HydiaError) as e:
                s3.indexScenarioPlainMulti(p3)
            assert "relinearisation key" in str(e.value)
            assert np.array_equal(cc3.db_export_ct(3), sample)
            del p3, sim
        finally:
            cc3.close()
        del p2
    finally:
        cc2.close()


# ------------------------------------------------------------------ 6. the full ring, once
def test_full_ring_two_blocks(im):
    """N = 2^15, dim 512, 2 blocks, hoisted and the auto form (B = 64): a batch of 3 distinct probes equals the single calls bit for
    bit, and its scores are within 1e-4 of numpy"""
    cc = im.Context(im.default_params(), 0)
    try:
        slots, dim = cc.N // 2, cc.dim
        cc.keygen_rotations(sorted(set(pow2_rotations(slots)) | set(range(64, dim, 64))), 11)
        n = 2 * slots - 5
        rng = np.random.default_rng(4)
        rows = rng.integers(-99, 100, size=(n, dim)).astype(np.float64)
        vecs = rng.choice([-1.0, 1.0], size=(3, dim))
        planted = [{12 + k, slots + 7 + k, n - 1 - k} for k in range(3)]
        for k in range(3):
            for r in planted[k]:
                rows[r] = vecs[k] * rng.integers(1, 4, size=dim)
        sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
        pts = sender.encodeQueries(vecs)
        for matvec in ("hoisted", "auto"):
            b = rows.copy()
            enrol(im, cc, b, matvec, seed=3)
            assert cc.db_kind() == (5 if matvec == "hoisted" else 6) and cc.db_stats()[:2] == (n, 2 * dim)
            sim = sender.computeSimilarityPlainMulti(pts)
            idx = sender.indexScenarioPlainMulti(pts)
            for k in range(3):
                assert np.array_equal(exported(sim[k]), exported(sender.computeSimilarity(pts[k]))), (matvec, k)
                assert np.array_equal(exported(idx[k]), exported(sender.indexScenario(pts[k]))), (matvec, k)
                scores = cc.decrypt(sim[k]).reshape(-1)[:n]
                assert np.abs(scores - b @ (vecs[k] / np.sqrt(dim))).max() < TOL
                hits = set(receiver.decryptIndex(idx[k]))
                assert planted[k] <= hits and not any(hits & planted[j] for j in range(3) if j != k)
            del sim, idx
        del pts
    finally:
        cc.close()
