"""A BATCH of encrypted queries against a PLAIN gallery on the GPU (hydia_*_gallery_multi, DiagonalSender.*GalleryMulti; run with
-m gpu): several probes share passes over the unencrypted templates.  The contract is "per query exactly what the single call returns on
the same gallery", so most comparisons here are np.array_equal of every exported limb against the single calls (which
tests/test_gpu_plain_gallery.py holds to the oracle), with queries that are DISTINCT and have distinct answers; one batch per form is
also held to the oracle directly (PlainRef: the oracle's sender path on trivial ciphertexts).  Ring and helpers: those of
tests/test_gpu_plain_gallery.py (N = 2^11, dim 64, 1024 slots, the three prime chains).

Loop B of a batch runs the k_hydia_plain_mq family.  Instantiated and launchable: k_hydia_plain_mq<A, QW, NW> for A in Sums128<false>,
Sums128<true>, Halves24<true>, QW in 1, 2, 4, NW in 1, 2, 4, 8, and k_hydia_plain_mq_sk<KS, QW> for KS in 4, 8, QW in 1, 2, 4 — 42
kernels, every one of which test_every_instantiation_runs_once launches.  k_hydia_plain_mq<Halves24<false>, *, *> is not instantiated (a
batch keeps the 128-bit sums on the 48-bit group-sequential layouts, as the other batches do).  The library's own width is 4, the
measured choice (hydia_plain_mq_width, profiles/plain_gallery_batch/README.md); Context.set_gallery_batch_width narrows it for a
measurement or a test."""
import ctypes

import numpy as np
import pytest

import test_gpu_plain_gallery as base
from plain_gallery_ref import PlainRef, pattern_ct, pattern_poly
from test_gpu_plain_gallery import ERR_ARG, ERR_STATE, TOL, enrol_plain, take, with_ledger, world

pytestmark = pytest.mark.gpu
WIDTH = 4  # hydia_plain_mq_width: queries per pass over the gallery of a batch as shipped


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """world() keeps its contexts in the plain-gallery module's table: what this module opened there is closed here"""
    yield
    for P, K, Or, cc in base._CTX.values():
        cc.close()
    base._CTX.clear()


SCENARIOS = ("computeSimilarity", "indexScenario", "membershipScenario")
C_NAMES = {"computeSimilarity": "hydia_compute_similarity_gallery_multi", "indexScenario": "hydia_index_scenario_gallery_multi",
           "membershipScenario": "hydia_membership_scenario_gallery_multi"}


def multi_of(sender, name):
    return getattr(sender, name + "GalleryMulti")


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
    wave; workgroup = the layout's group, else 4 / 2 / 1 waves by divisibility of G; 8-byte layouts one launch over all limbs; packed
    ones limb 0 (split-diagonal for <= 8 ciphertext-major blocks) and the rest (46-bit halves, else the 128-bit sums) separately"""
    seq, bits = layout  # (blocks per group of a group-sequential layout or 0, bits per stored residue of limbs 1..)
    W = seq if seq else 4 if G % 4 == 0 else 2 if G % 2 == 0 else 1
    want = {}
    for qw in schedule(Q, width):
        stream = lambda policy: "k_hydia_plain_mq<%s, %d, %d>" % (policy, qw, W)  # noqa: E731
        if bits == 64:
            names = [stream("Sums128<false>")]
        else:
            first = "k_hydia_plain_mq_sk<%d, %d>" % (8 if G <= 2 else 4, qw) if not seq and G <= 8 else stream("Sums128<false>")
            names = [first, stream("Halves24<true>" if bits == 46 else "Sums128<true>")]
        for n in names:
            want[n] = want.get(n, 0) + 1
    return want


def resident(cc):
    return cc.db_group(), cc.db_residue_bits()


def counted(im, call):
    """call() and {loop-B kernel: launches} of the byte ledger meanwhile"""
    im.byte_ledger(1)
    try:
        out = call()
    finally:
        led = im.byte_ledger(0)
    return out, {k: v[0] for k, v in led.items() if k.startswith("k_hydia_")}, led


def distinct_queries(P, rows, Q=5):
    """Q sign patterns, pairwise below 0.3 correlation, and rows planted for each of them alone in the first and the last block: the
    match / no-match answers of those 2 Q rows differ between any two queries.  -> (queries [Q][dim], planted: list of row sets)"""
    rng = np.random.default_rng(77)
    while True:
        v = rng.choice([-1.0, 1.0], size=(Q, P.dim))
        c = np.abs(v @ v.T) / P.dim - np.eye(Q)
        if c.max() < 0.3 and np.abs(v.sum(axis=1)).max() / P.dim < 0.3:  # (nor near the all-ones rows the shared gallery carries)
            break
    n = rows.shape[0]
    planted = []
    for k in range(Q):
        mine = {11 * k + 3, n - 1 - k}
        for r in mine:
            rows[r] = v[k] * rng.integers(1, 4, size=P.dim)
        planted.append(mine)
    return v, planted


def run_singles(im, sender, qs, scenarios=SCENARIOS):
    singles = {}
    for name in scenarios:
        singles[name] = []
        for q in qs:
            r, ran = with_ledger(im, lambda: getattr(sender, name)(q))
            assert ran and all(k.startswith("k_hydia_plain<") or k.startswith("k_hydia_plain_sk<") for k in ran), sorted(ran)  # a single call is untouched
            singles[name].append(exported(r))
        for a in range(len(qs)):
            for b in range(a):
                assert not np.array_equal(singles[name][a], singles[name][b]), (name, a, b)
    return singles


def assert_batches_equal_singles(im, cc, sender, qs, singles, sizes, G_loop, scenarios=SCENARIOS):
    for name in scenarios:
        for Q in sizes:
            cc.kernel_time_reset()
            res, ran, _ = counted(im, lambda: multi_of(sender, name)(qs[:Q]))
            assert ran == mq_kernels(resident(cc), G_loop, Q, WIDTH), (name, Q, sorted(ran.items()))
            assert cc.kernel_time("hydia_plain_multi")[1] == 1 and cc.kernel_time("hydia_plain")[1] == 0
            assert len(res) == Q
            for q in range(Q):
                got = exported(res[q])
                assert got.shape == singles[name][q].shape and np.array_equal(got, singles[name][q]), (name, Q, q)


# ------------------------------------------------------------------ 1. a batch equals the single calls, bit for bit
@pytest.mark.parametrize("matvec", ["hoisted", 8], ids=["hoisted", "B8"])
@pytest.mark.parametrize("blocks", [1, 3, 10])
@pytest.mark.parametrize("chain", ["default", "evaluator", "transform"])
def test_batches_equal_single_calls(im, chain, blocks, matvec):
    """1 block: split kernel KS = 8 on limb 0 (hoisted); 3: KS = 4; 10: streaming on a group-sequential layout; B = 8 multiplies the
    loop-B blocks by 8 giants (kind 8, giant-major slots).  Q = 1, 2, 3, 5: passes of 1, of 2, of 2 + 1, of 4 + 1 — every width shipped, a
    remainder, more than one pass.  The last block is ragged"""
    P, K, Or, cc = world(im, chain)
    rows = take(P.dim, P.slots, blocks, True)
    vecs, planted = distinct_queries(P, rows)
    n = rows.shape[0]
    enrol_plain(im, cc, rows, matvec)
    B = P.dim if matvec == "hoisted" else matvec
    assert cc.db_kind() == (8 if B < P.dim else 7)
    stats, sample = cc.db_stats(), cc.plain_db_export_pt(5)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    qs = [receiver.encryptQuery(vecs[k], seed=5 + k, nonce=1) for k in range(5)]
    singles = run_singles(im, sender, qs)
    assert_batches_equal_singles(im, cc, sender, qs, singles, (1, 2, 3, 5), blocks * (P.dim // B))
    if chain == "default":  # what the batch decrypts to: every query finds its own planted rows and none of another query's
        idx = sender.indexScenarioGalleryMulti(qs)
        mem = sender.membershipScenarioGalleryMulti(qs)
        for k in range(5):
            hits = set(receiver.decryptIndex(idx[k]))
            assert planted[k] <= hits, k
            assert not any(hits & planted[j] for j in range(5) if j != k), k
            assert receiver.decryptMembership(mem[k]) is True
    assert cc.db_stats() == stats and np.array_equal(cc.plain_db_export_pt(5), sample)


# ------------------------------------------------------------------ 2. a batch against the oracle on the trivial ciphertexts
@pytest.mark.parametrize("matvec", ["hoisted", 8], ids=["hoisted", "B8"])
def test_a_batch_of_three_equals_the_oracle(im, matvec):
    """the expectation is the reference path on the trivial ciphertexts (encode(image_t), 0) (tests/plain_gallery_ref.py), per query,
    bit for bit"""
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, 3, True)
    vecs, planted = distinct_queries(P, rows, 3)
    n = rows.shape[0]
    B = P.dim if matvec == "hoisted" else matvec
    a, b = rows.copy(), rows.copy()
    ref = PlainRef(P, Or, a, B)
    enrol_plain(im, cc, b, matvec)
    arr = ref.array()
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    oq = [Or.encrypt_query(vecs[k], 5 + k, 1) for k in range(3)]
    qs = [receiver.encryptQuery(vecs[k], seed=5 + k, nonce=1) for k in range(3)]
    assert all(np.array_equal(qs[k].export()[0], oq[k].data()) for k in range(3))
    sim, idx, mem = sender.computeSimilarityGalleryMulti(qs), sender.indexScenarioGalleryMulti(qs), sender.membershipScenarioGalleryMulti(qs)
    for k in range(3):
        want = Or.compute_similarity(oq[k], arr, n)
        got = sim[k].export()
        assert len(got) == len(want) == 3
        for g in range(3):
            assert np.array_equal(got[g], want[g].data()), (k, g)
        scores = cc.decrypt(sim[k]).reshape(-1)[:n]
        assert np.abs(scores - a @ (vecs[k] / np.linalg.norm(vecs[k]))).max() < TOL
        want = Or.index_scenario(oq[k], arr, n)
        got = idx[k].export()
        for g in range(3):
            assert np.array_equal(got[g], want[g].data()), (k, g)
        hits = set(receiver.decryptIndex(idx[k]))
        assert planted[k] <= hits and hits == set(Or.decrypt_index(want))
        want = Or.membership_scenario(oq[k], arr, n)
        assert np.array_equal(mem[k].export()[0], want.data()), k
        assert receiver.decryptMembership(mem[k]) is True


# ------------------------------------------------------------------ 3. saturated operands
SAT_SHAPES = [(8, 64), (16, 64), (1, 1024)]  # dim 1024 = every slot: the largest the ring allows; the 59/60-bit limbs fold every 128 / 32 diagonals


@pytest.mark.parametrize("blocks,dim", SAT_SHAPES, ids=["%dx%d" % s for s in SAT_SHAPES])
@pytest.mark.parametrize("chain", ["default", "evaluator", "transform"])
def test_saturated_operands(im, chain, blocks, dim):
    """every residue of the gallery (plain_db_import_pt) and of both polynomials of three imported query ciphertexts at q_j - 1: a
    batch of 3 equals the three single calls (which tests/test_gpu_plain_gallery.py holds to the oracle on these operands)"""
    P, K, Or, cc = world(im, chain, dim)
    n = blocks * P.slots
    m = pattern_poly(P, "sat")
    assert all((m[j] == P.moduli[j] - np.uint64(1)).all() for j in range(P.nQ))
    cc.plain_db_alloc(n, P.dim)
    for t in range(blocks * P.dim):
        cc.plain_db_import_pt(t, m)
    assert cc.db_kind() == 7
    sat = pattern_ct(P, "sat")
    assert (sat.data()[0] == m).all() and (sat.data()[1] == m).all()
    qs = [cc.import_ct(sat.data(), sat.scale) for _ in range(3)]
    sender = im.DiagonalSender(cc, n)
    single = exported(sender.computeSimilarity(qs[0]))
    res, ran, _ = counted(im, lambda: sender.computeSimilarityGalleryMulti(qs))
    assert ran == mq_kernels(resident(cc), blocks, 3, WIDTH), sorted(ran.items())
    for q in range(3):
        assert np.array_equal(exported(res[q]), single), q
    # and beside a query that is not saturated, in every position of the pass
    uni = pattern_ct(P, "uniform")
    u = cc.import_ct(uni.data(), uni.scale)
    single_u = exported(sender.computeSimilarity(u))
    assert not np.array_equal(single_u, single)
    for order in ([u, qs[0], qs[1]], [qs[0], u, qs[1]], [qs[0], qs[1], u]):
        res = sender.computeSimilarityGalleryMulti(order)
        for q, c in enumerate(order):
            assert np.array_equal(exported(res[q]), single_u if c is u else single), q


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
    every = {"k_hydia_plain_mq<%s, %d, %d>" % (a, qw, nw) for a in ("Sums128<false>", "Sums128<true>", "Halves24<true>") for qw in (1, 2, 4)
             for nw in (1, 2, 4, 8)} | {"k_hydia_plain_mq_sk<%d, %d>" % (ks, qw) for ks in (4, 8) for qw in (1, 2, 4)}
    assert len(every) == 42
    named = set()
    for chain, blocks, layout in INSTANCES:
        named |= set(mq_kernels(layout, blocks, 7, 4))
    assert named == every, sorted(every ^ named)


@pytest.mark.parametrize("chain,blocks,layout", INSTANCES, ids=["%s-%d" % c[:2] for c in INSTANCES])
def test_every_instantiation_runs_once(im, chain, blocks, layout):
    """a batch of 7 at the shipped width is passes of 4, 2 and 1 queries: all three QW of the layout's kernels in one call, against
    single calls; then narrowed to width 2 (passes of 2, 2, 2, 1).  The blocks differ from their neighbours (patterns in a rotating
    order), so does every query from the next"""
    P, K, Or, cc = world(im, chain, 16)
    n = blocks * P.slots
    polys = {name: pattern_poly(P, name) for name in PATTERNS}
    cc.plain_db_alloc(n, P.dim)
    for g in range(blocks):
        for i in range(P.dim):
            cc.plain_db_import_pt(g * P.dim + i, polys[PATTERNS[(g + g // 4) % 4]])
    assert cc.db_kind() == 7 and resident(cc) == layout
    assert cc.db_group() == layout[0] and cc.db_residue_bits() == layout[1]
    cts = [pattern_ct(P, name) for name in PATTERNS]
    pats = [cc.import_ct(c.data(), c.scale) for c in cts]
    sender = im.DiagonalSender(cc, n)
    single = []
    for q in pats:
        r, ran = with_ledger(im, lambda: sender.computeSimilarity(q))
        assert ran and all(k.startswith("k_hydia_plain<") or k.startswith("k_hydia_plain_sk<") for k in ran), sorted(ran)  # a single call is untouched
        single.append(exported(r))
    assert all(not np.array_equal(single[a], single[b]) for a in range(4) for b in range(a))
    order = [0, 2, 1, 3, 2, 0, 1]
    batch = [pats[k] for k in order]
    for width in (0, 2):
        cc.set_gallery_batch_width(width)
        try:
            res, ran, _ = counted(im, lambda: sender.computeSimilarityGalleryMulti(batch))
        finally:
            cc.set_gallery_batch_width(0)
        assert ran == mq_kernels(layout, blocks, 7, width or WIDTH), (width, sorted(ran.items()))
        assert schedule(7, width or WIDTH) == ([2, 2, 2, 1] if width else [4, 2, 1])
        for q, k in enumerate(order):
            assert np.array_equal(exported(res[q]), single[k]), (width, q)
    with pytest.raises(im.HydiaError) as e:
        cc.set_gallery_batch_width(3)
    assert e.value.code == ERR_ARG


# ------------------------------------------------------------------ 5. refusals
def c_call(cc, name, handles, n=None):
    """the C entry point itself: (code, outputs), the outputs pre-set to a non-NULL value"""
    n = len(handles) if n is None else n
    hs = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    out = (ctypes.c_void_p * max(n, 1))(*([1] * max(n, 1)))
    code = getattr(cc.L, name)(cc.h, hs, n, out)
    return code, [out[i] for i in range(n)]


def assert_refused(im, cc, sender, qs, code, scenarios=SCENARIOS, same_as_single=None, says=None):
    """both ways in: the role raises HydiaError(code) (with the single call's message where there is one), the C entry answers the
    code and leaves every output NULL; nothing is enqueued"""
    for name in scenarios:
        im.byte_ledger(1)
        try:
            with pytest.raises(im.HydiaError) as e:
                multi_of(sender, name)(qs)
            got, outs = c_call(cc, C_NAMES[name], [q.h for q in qs])
        finally:
            led = im.byte_ledger(0)
        assert e.value.code == code and got == code, (name, e.value.code, got, str(e.value))
        assert all(o is None for o in outs), name
        assert not led, sorted(led)
        if says is not None:
            assert says in str(e.value), str(e.value)
        if same_as_single is not None:
            with pytest.raises(im.HydiaError) as e1:
                getattr(sender, name)(same_as_single)
            assert e1.value.code == code and str(e1.value) == str(e.value), (str(e1.value), str(e.value))


def test_refusals_leave_the_gallery_alone(im):
    """every ERR_ARG and ERR_STATE of the table, through the C entry points and the roles"""
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, 2, True)
    n = rows.shape[0]
    enrol_plain(im, cc, rows.copy(), "hoisted")
    stats, sample = cc.db_stats(), cc.plain_db_export_pt(P.dim + 5)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    qs = [receiver.encryptQuery(v, seed=5 + k, nonce=1) for k, v in enumerate((np.ones(P.dim), -np.ones(P.dim)))]
    # an empty batch, a NULL handle
    for name in SCENARIOS:
        with pytest.raises(im.HydiaError) as e:
            multi_of(sender, name)([])
        assert e.value.code == ERR_ARG
        assert c_call(cc, C_NAMES[name], [], 0)[0] == ERR_ARG
        assert c_call(cc, C_NAMES[name], [qs[0].h, None]) == (ERR_ARG, [None, None])
        assert c_call(cc, C_NAMES[name], [None]) == (ERR_ARG, [None])
        assert getattr(cc.L, C_NAMES[name])(None, None, 1, None) == ERR_ARG
    # unequal scales; a query that is not at full level (one limb fewer; a level-1 result), first and later in the batch
    raw = qs[0].export()[0]
    other = cc.import_ct(raw, cc.delta * 2.0)
    assert_refused(im, cc, sender, [qs[0], other], ERR_ARG)
    assert_refused(im, cc, sender, [other, qs[0], qs[1]], ERR_ARG)
    low = cc.import_ct(raw[:, :P.nQ - 1], cc.delta)
    for batch in ([low, qs[0]], [qs[0], qs[1], low], [low]):
        assert_refused(im, cc, sender, batch, ERR_ARG, says="full level")
    # a Plaintext in the list: the role refuses it before the library is called
    pt = im.Plaintext.__new__(im.Plaintext)
    for name in SCENARIOS:
        im.byte_ledger(1)
        try:
            with pytest.raises(im.HydiaError) as e:
                multi_of(sender, name)([qs[0], pt])
        finally:
            led = im.byte_ledger(0)
        assert e.value.code == ERR_ARG and not led
    assert cc.db_stats() == stats and cc.db_kind() == 7 and np.array_equal(cc.plain_db_export_pt(P.dim + 5), sample)
    # on the plain gallery: the ciphertext batch and the plain-query batch are still refused, the new call is served
    with pytest.raises(im.HydiaError) as e:
        sender.indexScenarioMulti(qs)
    assert e.value.code == ERR_STATE and "plain gallery" in str(e.value)
    enc = im.DiagonalSender(cc, n)
    # (encodeQuery itself does not look at the database)
    probes = [enc.encodeQuery(np.ones(P.dim))]
    with pytest.raises(im.HydiaError) as e:
        sender.indexScenarioPlainMulti(probes)
    assert e.value.code == ERR_STATE and "plain gallery" in str(e.value)
    del probes
    served = sender.indexScenarioGalleryMulti(qs)
    assert len(served) == 2 and np.array_equal(exported(served[1]), exported(sender.indexScenario(qs[1])))
    assert cc.db_stats() == stats and np.array_equal(cc.plain_db_export_pt(P.dim + 5), sample)
    # a ciphertext database, both forms: the message names the call to use
    for matvec, kind in (("hoisted", 5), (8, 6)):
        cc.set_matvec(matvec)
        try:
            im.DiagonalEnroller(cc, n).serializeDB(rows.copy(), seed=3)
        finally:
            cc.set_matvec("auto")
        st, smp = cc.db_stats(), cc.db_export_ct(P.dim + 5)
        assert cc.db_kind() == kind
        assert_refused(im, cc, sender, qs, ERR_STATE, says="hydia_*_multi")
        assert cc.db_stats() == st and cc.db_kind() == kind and np.array_equal(cc.db_export_ct(P.dim + 5), smp)
        assert len(sender.indexScenarioMulti(qs)) == 2  # which serves it
    # HERS' column packing (kind 4)
    im.HersEnroller(cc, 100).serializeDB(rows[:100].copy(), seed=5)
    st = cc.db_stats()
    assert cc.db_kind() == 4
    assert_refused(im, cc, sender, qs, ERR_STATE)
    assert cc.db_stats() == st and cc.db_kind() == 4
    # no database at all
    fresh = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        q0 = [fresh.import_ct(q.export()[0], cc.delta) for q in qs]
        assert_refused(im, fresh, im.DiagonalSender(fresh, n), q0, ERR_STATE)
        assert fresh.db_kind() == 0
        del q0
    finally:
        fresh.close()
    # a shard context of a group, and the sharded role
    grp = im.ShardGroup([0, 0], im.default_params(log_n=11, vector_dim=64))
    try:
        sc = grp.shard_ctx(0)
        q0 = [sc.import_ct(q.export()[0], cc.delta) for q in qs]
        assert_refused(im, sc, im.DiagonalSender(sc, n), q0, ERR_STATE)
        assert sc.db_kind() == 0
        for name in SCENARIOS:
            with pytest.raises(im.HydiaError) as e:
                multi_of(im.DiagonalSender(grp, n), name)(q0)
            assert e.value.code == ERR_STATE
        del q0
    finally:
        grp.close()


def loop_a_keys(cc, fresh, dim, skip=()):
    """the hoisted rotations' keys 1 .. dim-1 of cc, imported into the key-less context `fresh`"""
    for i in range(1, dim):
        if i not in skip:
            fresh.import_eval_key(i, cc.export_eval_key(i))


def test_missing_keys_are_named_before_any_work(im):
    """a giant-step key (a B = 8 gallery on a context without rotation 24), a power-of-two key, the relinearisation key: the single
    call's ERR_STATE and message, nothing enqueued, the gallery as it was; similarity with loop A's keys alone is served"""
    P, K, Or, cc = world(im)
    rows = take(P.dim, P.slots, 2, True)
    n = rows.shape[0]
    vecs = (np.ones(P.dim), -np.ones(P.dim), np.ones(P.dim))
    raws = [im.DiagonalReceiver(cc, n).encryptQuery(v, seed=5 + k, nonce=1).export()[0] for k, v in enumerate(vecs)]
    prm = im.default_params(log_n=11, vector_dim=64)
    # no rotation key 24: a giant step of the B = 8 form
    c1 = im.Context(prm, 0)
    try:
        c1.keygen_rotations([i for i in range(1, P.slots) if i != 24 and (i < P.dim or i & (i - 1) == 0)], 7)
        assert not c1.has_eval_key(24) and c1.has_eval_key(16)
        enrol_plain(im, c1, rows.copy(), 8)
        assert c1.db_kind() == 8
        stats, sample = c1.db_stats(), c1.plain_db_export_pt(P.dim + 5)
        s1 = im.DiagonalSender(c1, n)
        q1 = [c1.import_ct(r, c1.delta) for r in raws]
        assert_refused(im, c1, s1, q1, ERR_STATE, same_as_single=q1[0], says="rotation key 24")
        assert c1.db_stats() == stats and np.array_equal(c1.plain_db_export_pt(P.dim + 5), sample)
        del q1
    finally:
        c1.close()
    # no rotation key 256: EvalSum of membership
    c2 = im.Context(prm, 0)
    try:
        c2.keygen_rotations(list(range(1, P.dim)) + [64, 128, 512], 7)
        enrol_plain(im, c2, rows.copy(), "hoisted")
        stats, sample = c2.db_stats(), c2.plain_db_export_pt(P.dim + 5)
        s2 = im.DiagonalSender(c2, n)
        q2 = [c2.import_ct(r, c2.delta) for r in raws[:2]]
        assert len(s2.indexScenarioGalleryMulti(q2)) == 2
        assert_refused(im, c2, s2, q2, ERR_STATE, ("membershipScenario",), same_as_single=q2[0], says="rotation key 256")
        assert c2.db_stats() == stats and np.array_equal(c2.plain_db_export_pt(P.dim + 5), sample)
        # no relinearisation key: loop A's keys alone, imported
        c3 = im.Context(prm, 0)
        try:
            loop_a_keys(c2, c3, P.dim)
            enrol_plain(im, c3, rows.copy(), "hoisted")
            s3 = im.DiagonalSender(c3, n)
            q3 = [c3.import_ct(r, c3.delta) for r in raws[:2]]
            sim = s3.computeSimilarityGalleryMulti(q3)  # similarity needs no key beyond loop A's
            assert np.array_equal(exported(sim[1]), exported(s3.computeSimilarity(q3[1])))
            assert_refused(im, c3, s3, q3, ERR_STATE, ("indexScenario", "membershipScenario"), same_as_single=q3[0], says="relinearisation key")
            assert np.array_equal(c3.plain_db_export_pt(P.dim + 5), sample)
            del q3, sim
        finally:
            c3.close()
        del q2
    finally:
        c2.close()


# ------------------------------------------------------------------ 6. the full ring, once
def test_full_ring_two_blocks(im):
    """N = 2^15, dim 512, 2 blocks, the auto (BSGS) form: a batch of 3 distinct queries equals the single calls bit for bit for
    similarity and index, and its scores are within 1e-4 of numpy.  (The full key set: loop A's key table asks for every rotation
    1 .. 511 whatever the form, as the single call's does)"""
    cc = im.Context(im.default_params(), 0)
    try:
        cc.keygen(11)
        slots, dim = cc.N // 2, cc.dim
        n = 2 * slots - 5
        rng = np.random.default_rng(4)
        rows = rng.integers(-99, 100, size=(n, dim)).astype(np.float64)
        vecs = rng.choice([-1.0, 1.0], size=(3, dim))
        planted = [{12 + k, slots + 7 + k, n - 1 - k} for k in range(3)]
        for k in range(3):
            for r in planted[k]:
                rows[r] = vecs[k] * rng.integers(1, 4, size=dim)
        im.PlainEnroller(cc, n).serializeDB(rows)
        assert cc.db_kind() == 8 and cc.db_babies() == cc.auto_babies(2) < dim and cc.db_stats()[:2] == (n, 2 * dim)
        sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
        qs = [receiver.encryptQuery(vecs[k], seed=5 + k, nonce=1) for k in range(3)]
        sim = sender.computeSimilarityGalleryMulti(qs)
        idx = sender.indexScenarioGalleryMulti(qs)
        for k in range(3):
            assert np.array_equal(exported(sim[k]), exported(sender.computeSimilarity(qs[k]))), k
            assert np.array_equal(exported(idx[k]), exported(sender.indexScenario(qs[k]))), k
            scores = cc.decrypt(sim[k]).reshape(-1)[:n]
            assert np.abs(scores - rows @ (vecs[k] / np.sqrt(dim))).max() < TOL
            hits = set(receiver.decryptIndex(idx[k]))
            assert planted[k] <= hits and not any(hits & planted[j] for j in range(3) if j != k)
        del sim, idx, qs
    finally:
        cc.close()
