"""In-place update of a plain gallery on the GPU (hydia_plain_db_update; run with -m gpu): append, remove, replace, growth across the
layout change, updates inside a group-sequential gallery on every residue width, saturated residues, the pre-rotated form, the
scenarios afterwards, the refused calls and a growth that does not fit in device memory.  Plaintexts are compared through
plain_db_export_pt, np.array_equal against the restatement on the CPU oracle (tests/plain_gallery_update_ref.py) — bit for bit,
never against the product itself.  Ring, contexts and rows: those of tests/test_gpu_plain_gallery.py (N = 2^11, 64-dim vectors,
1024 slots, 64 plaintexts per block)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_plain_gallery as base
from plain_gallery_ref import PlainRef, pattern_poly
from plain_gallery_update_ref import PlainUpdateRef, add_mod, trivial_array
from test_gpu_plain_gallery import enrol_plain, planted_in, raw_rows, world

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_DEVICE = -1, -2, -3


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for P, K, Or, cc in base._CTX.values():
        cc.close()
    base._CTX.clear()


def same(cc, up, ts):
    for t in ts:
        assert np.array_equal(cc.plain_db_export_pt(t), up.pts[t]), t


def block(P, g):
    return range(g * P.dim, (g + 1) * P.dim)


def exports(cc, ts):
    return {t: cc.plain_db_export_pt(t) for t in ts}


def unchanged(cc, before):
    for t, want in before.items():
        assert np.array_equal(cc.plain_db_export_pt(t), want), t


def shared(P, n):
    """a copy of the first n of the shared rows"""
    return raw_rows(P.dim, 16, P.slots)[:n].copy()


# ------------------------------------------------------------------ 1. append
def test_append_across_a_block_edge(im):
    """hoisted, 2 blocks with 3 rows missing, + 5 rows: block 1 is old + E, block 2 is E — the enrolment's block of the same rows —
    and block 0 is neither read nor written"""
    P, K, Or, cc = world(im)
    n0, n1 = 2 * P.slots - 3, 2 * P.slots + 2
    a, b = shared(P, n0), shared(P, n0)
    up = PlainUpdateRef(P).enroll(PlainRef(P, Or, a), blocks={1})
    enrol_plain(im, cc, b, "hoisted")
    enr = im.PlainEnroller(cc, n0)
    assert cc.db_kind() == 7 and cc.db_group() == 0 and cc.db_residue_bits() == 48 and cc.db_stats()[:2] == (n0, 2 * P.dim)
    block0 = exports(cc, block(P, 0))
    a, b = shared(P, n1)[n0:].copy(), shared(P, n1)[n0:].copy()
    touched = up.update(n0, a, 1)
    enr.appendDB(b)
    assert np.array_equal(a, b)  # both normalise the rows in place
    assert touched == list(range(P.dim, 3 * P.dim))
    assert cc.db_stats()[:2] == (n1, 3 * P.dim) and enr.numVectors == n1 and up.n == n1
    assert cc.db_kind() == 7 and cc.db_babies() == P.dim and cc.db_group() == 0
    same(cc, up, touched)
    unchanged(cc, block0)
    # the created block is an enrolment's: on the oracle, and on the product
    whole = PlainRef(P, Or, shared(P, n1))
    created = exports(cc, block(P, 2))
    for t in block(P, 2):
        assert np.array_equal(created[t], whole.encode(t)), t
    enrol_plain(im, cc, shared(P, n1), "hoisted")
    unchanged(cc, created)


# ------------------------------------------------------------------ 2. remove and replace
def test_remove_and_replace(im):
    P, K, Or, cc = world(im)
    n = 2 * P.slots - 3
    a = shared(P, n)
    ref = PlainRef(P, Or, a)
    up = PlainUpdateRef(P).enroll(ref)
    enrol_plain(im, cc, shared(P, n), "hoisted")
    enr = im.PlainEnroller(cc, n)
    rng = np.random.default_rng(12)
    # a single-row update followed by its negation restores every touched plaintext bit for bit
    before = exports(cc, block(P, 0))
    row = rng.integers(-99, 100, size=(1, P.dim)).astype(np.float64)
    raw, given = row.copy(), row.copy()
    touched = up.update(700, row, 1)  # (row is normalised now)
    enr.updateRows(700, given)
    assert np.array_equal(given, row) and touched == list(block(P, 0))
    same(cc, up, touched)
    assert not np.array_equal(cc.plain_db_export_pt(700 % P.dim), before[700 % P.dim])
    up.update(700, -raw, 1)  # the SAME rows negated, with the same normalise
    enr.updateRows(700, -raw, True)
    unchanged(cc, before)
    same(cc, up, touched)
    # removal of an enrolled template: the negated normalised row
    gone = -ref.rows[17:18].copy()
    up.update(17, gone.copy(), 1)
    enr.updateRows(17, gone.copy(), True)
    same(cc, up, block(P, 0))
    # two rows added in one call, one of them removed alone: the helper's three-term sum (old + E(both) + E(-one)), nothing else
    two = rng.integers(-99, 100, size=(2, P.dim)).astype(np.float64)
    given = two.copy()
    touched = up.update(n, two, 1)
    enr.appendDB(given)
    assert touched == list(block(P, 1)) and enr.numVectors == n + 2 == cc.db_stats()[0]
    up.update(n + 1, -two[1:2].copy(), 1)
    enr.updateRows(n + 1, -two[1:2].copy())
    same(cc, up, touched)
    # replace: new_normalised - old_normalised, as given
    new = rng.integers(1, 4, size=P.dim).astype(np.float64)
    new /= np.linalg.norm(new)
    delta = (new - ref.rows[9])[None, :].copy()
    given = delta.copy()
    up.update(9, delta, 0)
    enr.updateRows(9, given, False)
    assert np.array_equal(given, delta)  # normalise = 0 takes the rows as given
    same(cc, up, block(P, 0))
    assert cc.db_stats()[:2] == (n + 2, 2 * P.dim) and cc.db_kind() == 7


# ------------------------------------------------------------------ 3. growth across the layout change
@pytest.mark.parametrize("blocks", [8, 10])
def test_growth_across_the_layout_change(im, blocks):
    """hoisted, 8 -> 9 blocks: ciphertext-major 48-bit becomes group-sequential 46-bit; 10 -> 11 blocks: the group size changes.
    Every old plaintext exported before equals its export after"""
    P, K, Or, cc = world(im)
    n0, n1 = blocks * P.slots - 3, blocks * P.slots + 7
    a = shared(P, n0)
    ref = PlainRef(P, Or, a)
    up = PlainUpdateRef(P).enroll(ref, blocks={blocks - 1})
    enrol_plain(im, cc, shared(P, n0), "hoisted")
    enr = im.PlainEnroller(cc, n0)
    group0 = cc.db_group()
    assert (group0, cc.db_residue_bits()) == ((0, 48) if blocks == 8 else (2, 46))
    before = exports(cc, range((blocks - 1) * P.dim))
    for t in (0, P.dim + 5, (blocks - 1) * P.dim - 1):
        assert np.array_equal(before[t], ref.encode(t)), t
    touched = up.update(n0, shared(P, n1)[n0:].copy(), 1)
    enr.appendDB(shared(P, n1)[n0:].copy())
    assert touched == list(range((blocks - 1) * P.dim, (blocks + 1) * P.dim))
    assert cc.db_kind() == 7 and cc.db_babies() == P.dim and cc.db_stats()[:2] == (n1, (blocks + 1) * P.dim) and enr.numVectors == n1
    assert cc.db_group() > 0 and cc.db_group() != group0 and cc.db_residue_bits() == 46
    unchanged(cc, before)
    same(cc, up, touched)


# ------------------------------------------------------------------ 4. inside a group-sequential gallery
CASES = [("default", {}, 46), ("default", {"HYDIA_DB_48BIT": "1"}, 48), ("evaluator", {}, 48), ("transform", {}, 64)]


@pytest.mark.parametrize("chain,env,bits", CASES, ids=["46", "48-env", "evaluator", "transform"])
def test_update_inside_a_group_sequential_gallery(im, chain, env, bits, monkeypatch):
    """10 blocks; 25 rows that start and end in mid-block across the edge of blocks 3 and 4: 46-bit granules, 6-byte residues (under
    HYDIA_DB_48BIT in a context of its own, and on the 47/48-bit chain) and 8-byte residues (the transform chain)"""
    P, K, Or, cc = world(im, chain)
    own = None
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cc = own = im.Context(im.default_params(log_n=11, vector_dim=P.dim), 0)
        for k in env:
            monkeypatch.delenv(k)
    try:
        n = 10 * P.slots - 3
        a = shared(P, n)
        up = PlainUpdateRef(P).enroll(PlainRef(P, Or, a), blocks={3, 4})
        enrol_plain(im, cc, shared(P, n), "hoisted")
        group = 0 if bits == 64 else 2  # (an unpacked database stays ciphertext-major)
        assert cc.db_group() == group and cc.db_residue_bits() == bits
        near = exports(cc, (0, 2 * P.dim + 31, 3 * P.dim - 1, 5 * P.dim, 10 * P.dim - 1))
        rng = np.random.default_rng(4)
        first = 4 * P.slots - 10
        rows = rng.integers(-99, 100, size=(25, P.dim)).astype(np.float64)
        touched = up.update(first, rows.copy(), 1)
        assert touched == list(range(3 * P.dim, 5 * P.dim))
        cc.plain_db_update(first, rows.copy(), True)
        delta = rng.uniform(-0.1, 0.1, size=(3, P.dim))
        up.update(first + 9, delta.copy(), 0)  # 4 slots - 1 .. 4 slots + 1: across the edge again
        cc.plain_db_update(first + 9, delta.copy(), False)
        assert cc.db_group() == group and cc.db_residue_bits() == bits and cc.db_stats()[:2] == (n, 10 * P.dim)
        same(cc, up, touched)
        unchanged(cc, near)  # the neighbours and the ends
    finally:
        if own is not None:
            own.close()


# ------------------------------------------------------------------ 5. saturated residues
@pytest.mark.parametrize("pattern", ["sat", "holes", "edge"])
@pytest.mark.parametrize("blocks,bits", [(1, 48), (10, 46)])
def test_saturated_residues(im, blocks, bits, pattern):
    """every residue of the touched plaintexts at q_j - 1 (and the holes and 0, 1, q - 2, q - 1 patterns), planted through
    plain_db_import_pt: where an unreduced sum would carry into the neighbouring 46- or 48-bit field.  Expected: (pattern + E) mod q"""
    P, K, Or, cc = world(im)
    n = blocks * P.slots - 3
    m = pattern_poly(P, pattern)
    first = 500 if blocks == 1 else 4 * P.slots - 10
    touched_blocks = (0,) if blocks == 1 else (3, 4)
    cc.plain_db_alloc(n, P.dim)
    assert cc.db_kind() == 7 and cc.db_residue_bits() == bits and cc.db_group() == (0 if blocks == 1 else 2)
    pts = [None] * (blocks * P.dim)
    for g in touched_blocks:
        for t in block(P, g):
            cc.plain_db_import_pt(t, m)
            pts[t] = m
    up = PlainUpdateRef(P).planted(n, pts)
    rows = np.random.default_rng(6).integers(-99, 100, size=(25, P.dim)).astype(np.float64)
    unit = rows.copy()
    touched = up.update(first, unit, 1)  # (normalises `unit` in place)
    cc.plain_db_update(first, rows.copy(), True)
    assert len(touched) == len(touched_blocks) * P.dim
    t = touched[1]
    E = up.encodings(first, unit)[t]
    assert E.any() and np.array_equal(up.pts[t], add_mod(P, m, E)) and all((up.pts[t][j] < P.moduli[j]).all() for j in range(P.nQ))
    same(cc, up, touched)
    assert cc.db_stats()[:2] == (n, blocks * P.dim)


# ------------------------------------------------------------------ 6. the pre-rotated form
def test_pre_rotated_form(im):
    """B = 8, kind 8, 2 blocks (16 loop-B blocks of 8 plaintexts: group-sequential already): an update inside block 0 and a growth to
    3 blocks, against hyo_enroll_layout_row_bsgs; the form stays"""
    P, K, Or, cc = world(im)
    n0, n1 = 2 * P.slots - 3, 2 * P.slots + 7
    a = shared(P, n0)
    up = PlainUpdateRef(P, 8).enroll(PlainRef(P, Or, a, 8))
    enrol_plain(im, cc, shared(P, n0), 8)
    enr = im.PlainEnroller(cc, n0)
    assert cc.db_kind() == 8 and cc.db_babies() == 8 and cc.db_group() > 0
    same(cc, up, (0, 9, 2 * P.dim - 1))
    rows = np.random.default_rng(7).integers(-99, 100, size=(3, P.dim)).astype(np.float64)
    touched = up.update(10, rows.copy(), 1)
    enr.updateRows(10, rows.copy(), True)
    assert touched == list(block(P, 0)) and cc.db_kind() == 8 and cc.db_babies() == 8
    same(cc, up, range(2 * P.dim))
    before = exports(cc, block(P, 0))
    touched = up.update(n0, shared(P, n1)[n0:].copy(), 1)
    enr.appendDB(shared(P, n1)[n0:].copy())
    assert touched == list(range(P.dim, 3 * P.dim))
    assert cc.db_kind() == 8 and cc.db_babies() == 8 and cc.db_stats()[:2] == (n1, 3 * P.dim) and enr.numVectors == n1 and cc.db_group() > 0
    same(cc, up, touched)
    unchanged(cc, before)
    whole = PlainRef(P, Or, shared(P, n1), 8)
    for t in block(P, 2):
        assert np.array_equal(cc.plain_db_export_pt(t), whole.encode(t)), t


# ------------------------------------------------------------------ 7. scenarios after an update
@pytest.mark.parametrize("blocks", [2, 10])
def test_scenarios_after_an_update(im, blocks):
    """a planted row appended and a planted row removed: the index scenario through rebuilt sender / receiver objects finds the one
    and not the other, bit for bit what a second gallery imported from the expected polynomials answers (and, at 2 blocks, what the
    oracle answers over the trivial ciphertexts); a batch of three queries equals the three single calls"""
    P, K, Or, cc = world(im)
    n0, n1 = blocks * P.slots - 3, blocks * P.slots - 1
    ref = PlainRef(P, Or, shared(P, n0))
    up = PlainUpdateRef(P).enroll(ref)
    enrol_plain(im, cc, shared(P, n0), "hoisted")
    enr = im.PlainEnroller(cc, n0)
    removed = (blocks - 1) * P.slots + 17  # raw_rows plants one there
    assert removed in planted_in(ref.rows)
    new = np.random.default_rng(8).integers(-99, 100, size=(2, P.dim)).astype(np.float64)
    new[1] = np.arange(P.dim) % 3 + 1  # a match of the all-ones query
    up.update(n0, new.copy(), 1)
    enr.appendDB(new.copy())
    gone = -ref.rows[removed:removed + 1].copy()
    up.update(removed, gone.copy(), 1)
    enr.updateRows(removed, gone.copy())
    assert enr.numVectors == n1 == cc.db_stats()[0] and cc.db_stats()[1] == blocks * P.dim
    same(cc, up, block(P, blocks - 1))
    sender, receiver = im.DiagonalSender(cc, n1), im.DiagonalReceiver(cc, n1)  # rebuilt for the new vector count
    rng = np.random.default_rng(9)
    vecs = [np.ones(P.dim), rng.integers(1, 4, size=P.dim).astype(np.float64), rng.integers(-3, 4, size=P.dim).astype(np.float64)]
    qs = [receiver.encryptQuery(v, seed=5 + k, nonce=1) for k, v in enumerate(vecs)]
    got = [sender.indexScenario(q) for q in qs]
    hits = set(receiver.decryptIndex(got[0]))
    assert n0 + 1 in hits and removed not in hits and (planted_in(ref.rows) - {removed}) <= hits
    got = [np.asarray(g.export()) for g in got]
    multi = sender.indexScenarioGalleryMulti(qs)
    for k in range(3):
        assert np.array_equal(np.asarray(multi[k].export()), got[k]), k
    if blocks == 2:
        q = Or.encrypt_query(vecs[0], 5, 1)
        assert np.array_equal(qs[0].export()[0], q.data())
        want = Or.index_scenario(q, trivial_array(P, up.pts), n1)
        assert len(want) == blocks == len(got[0])
        for g in range(blocks):
            assert np.array_equal(got[0][g], want[g].data()), g
    # a second gallery: plain_db_alloc + import_pt of the expected polynomials
    cc.plain_db_alloc(n1, P.dim)
    for t, m in enumerate(up.pts):
        cc.plain_db_import_pt(t, m)
    sender = im.DiagonalSender(cc, n1)
    for k in range(3):
        assert np.array_equal(np.asarray(sender.indexScenario(qs[k]).export()), got[k]), k


# ------------------------------------------------------------------ 8. refusals
def test_refused_calls_leave_everything_alone(im):
    P, K, Or, cc = world(im)
    L = cc.L
    rows = np.random.default_rng(10).integers(-99, 100, size=(4, P.dim)).astype(np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def update(c, first, r, n):
        return L.hydia_plain_db_update(c.h, first, None if r is None else vp(r), n, 1)

    # no database resident
    fresh = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        assert update(fresh, 0, rows.copy(), 4) == ERR_STATE
        assert fresh.db_kind() == 0 and fresh.db_stats() == (0, 0, 0)
    finally:
        fresh.close()
    # a ciphertext database: the message names its own entry point
    n = 300
    im.DiagonalEnroller(cc, n).serializeDB(shared(P, n), seed=3)
    assert cc.db_kind() in (5, 6)
    stats, before = cc.db_stats(), cc.db_export_ct(1)
    with pytest.raises(im.HydiaError) as e:
        cc.plain_db_update(n, rows.copy(), True)
    assert e.value.code == ERR_STATE and "hydia_db_update" in str(e.value)
    assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(1), before)
    # a plain gallery: argument errors, and the empty update
    enrol_plain(im, cc, shared(P, n), "hoisted")
    stats, before = cc.db_stats(), exports(cc, (0, 1, P.dim - 1))
    given = rows.copy()
    assert update(cc, n + 1, given, 4) == ERR_ARG     # a hole
    assert update(cc, 0, None, 4) == ERR_ARG           # null rows with n > 0
    assert update(cc, 1, given, 2 ** 64 - 1) == ERR_ARG  # a row count that overflows
    assert update(cc, 0, None, 0) == 0 and update(cc, n, given, 0) == 0  # n == 0: nothing changes
    assert np.array_equal(given, rows)  # not even normalised
    assert cc.db_stats() == stats and cc.db_kind() == 7
    unchanged(cc, before)
    assert update(cc, n, given, 4) == 0 and cc.db_stats()[0] == n + 4  # first_vector == n_old is the append


# ------------------------------------------------------------------ 9. growth without room
def test_growth_without_room_fails_before_anything_is_touched(im):
    """an append that adds a block to a 2^21-vector gallery (142 GiB resident) needs a second buffer of 143 GiB, which a 288 GB GPU
    does not have: HYDIA_ERR_DEVICE, and vectors, plaintexts, layout and form are what they were"""
    cc = im.Context()
    try:
        cc.plain_db_alloc(1 << 21, 512)
        stats, group = cc.db_stats(), cc.db_group()
        assert cc.db_kind() == 7 and stats[0] == 1 << 21 and stats[2] > 140 << 30
        m = np.zeros((cc.nQ, cc.N), dtype=np.uint64)
        m[:, ::7] = 12345
        ts = (0, 777, stats[1] - 1)
        for t in ts:
            cc.plain_db_import_pt(t, m)
        before = exports(cc, ts)
        rows = np.ones((1, 512))
        with pytest.raises(im.HydiaError) as e:
            cc.plain_db_update(1 << 21, rows, True)
        assert e.value.code == ERR_DEVICE and "second buffer" in str(e.value)
        assert cc.db_stats() == stats and cc.db_group() == group and cc.db_kind() == 7 and cc.db_babies() == 512 and cc.db_residue_bits() == 46
        unchanged(cc, before)
    finally:
        cc.close()
