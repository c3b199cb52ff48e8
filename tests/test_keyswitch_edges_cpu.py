"""The host side of the crafted-evaluation-key tests (tests/test_gpu_keyswitch_edges.py), without a GPU: the key and ciphertext
patterns of tests/keyswitch_ref.py are what they claim, the oracle reads a key view that was edited in place, the key rows of digits
a switch does not use do not enter the oracle's result, and the oracle's key switch equals a Python-integer model of hybrid key
switching bit for bit over every coefficient at N = 2^11 — on saturated, edge and single-digit keys against saturated and uniform
polynomials, at 12, 5 and 1 limbs, on the default chain and on the edge-prime chain transform_chain(11).  The oracle is the
reference of the GPU file; this file pins that reference on inputs no key generator produces."""
import numpy as np
import pytest

import batch_ref as B
import keyswitch_ref as KR
import oracle_lib as O

SEED = 20260412
ROTATIONS = (1, 2, 5)


def _chain(name):
    if name == "default":
        return None
    from test_gpu_edge_primes import transform_chain  # (a function of that GPU module; importing it runs nothing)
    return transform_chain(11)


class Ring:
    def __init__(self, name):
        moduli = _chain(name)
        kw = {} if moduli is None else {"moduli": moduli, "n_p": 4}
        self.P = O.Params(log_n=11, depth=11, dim=16, **kw)
        assert (self.P.nQ, self.P.nP, self.P.dnum, self.P.alpha) == (12, 4, 3, 4)
        self.K = O.Keys(self.P, SEED, rotations=list(ROTATIONS))
        self.Or = O.Oracle(self.P, self.K)
        self.genuine = {0: self.K.relin().copy(), **{r: self.K.rot_key(r).copy() for r in ROTATIONS}}

    def view(self, slot):
        return self.K.relin() if slot == 0 else self.K.rot_key(slot)

    def restore(self):
        for slot, data in self.genuine.items():
            self.view(slot)[...] = data


@pytest.fixture(scope="module", params=["default", "transform"])
def ring(request):
    R = Ring(request.param)
    yield R
    R.restore()


@pytest.fixture(scope="module")
def default_ring():
    R = Ring("default")
    yield R
    R.restore()


def rng_for(*ints):
    return np.random.default_rng([SEED] + [int(i) for i in ints])


def owned(ct):
    """a copy of an oracle ciphertext's residues, taken while the ciphertext is alive (data() is a view into it)"""
    return ct.data().copy()


def poly_ct(P, npoly, nl, pattern, rng, phase=0):
    return KR.craft_ct(P, B.new_ct(P, npoly, nl, 2.0 ** 45), pattern, rng, phase)


# ---------------------------------------------------------------- the patterns
def test_key_patterns_are_what_they_claim(default_ring):
    P = default_ring.P
    key = np.zeros((P.dnum, 2, P.nT, P.N), dtype=np.uint64)
    q = P.moduli.reshape(1, 1, P.nT, 1)
    holes_per_row = P.N // KR.HOLE_EVERY
    for pattern in KR.key_patterns(P.dnum):
        key[...] = 12345
        KR.craft_key(P, key, pattern, rng_for(1), phase=3)
        assert (key < q).all(), pattern
        top, zero = (key == q - np.uint64(1)), (key == 0)
        if pattern == "sat":
            assert top.all()
        elif pattern == "holes":
            assert (top.sum(axis=3) == P.N - holes_per_row).all()
            for d in range(P.dnum):
                for p in range(2):
                    for m in range(P.nT):
                        at = np.flatnonzero(~top[d, p, m])
                        assert len(at) == holes_per_row and (np.diff(at) == KR.HOLE_EVERY).all()
                        assert at[0] == (-KR.row_shift(d, p, m, P.nT, 3)) % KR.HOLE_EVERY
            # the hole position moves from row to row: over the rows every position is a hole somewhere
            assert len({int(np.flatnonzero(~top[d, p, m])[0]) for d in range(P.dnum) for p in range(2) for m in range(P.nT)}) == KR.HOLE_EVERY
        elif pattern == "edge":
            for value in (0, 1):
                assert ((key == value).sum(axis=3) == P.N // 4).all()
            assert (top.sum(axis=3) == P.N // 4).all() and ((key == q - np.uint64(2)).sum(axis=3) == P.N // 4).all()
            cyc = lambda m: [0, 1, int(P.moduli[m]) - 2, int(P.moduli[m]) - 1]
            for d, p, m in ((0, 0, 0), (1, 1, 5), (2, 0, 15)):
                s = KR.row_shift(d, p, m, P.nT, 3)
                assert [int(v) for v in key[d, p, m, :8]] == [cyc(m)[(i + s) % 4] for i in range(8)]
        elif pattern == "uniform":
            assert not top.any() and not zero.any()  # (2^-45 per residue that one is hit)
            assert len(np.unique(key[0, 0, 1])) > P.N - 4
        else:
            only = int(pattern[6:])
            for d in range(P.dnum):
                assert top[d].all() if d == only else zero[d].all(), (pattern, d)


def test_ciphertext_patterns_are_what_they_claim(default_ring):
    P = default_ring.P
    for nl in (12, 5, 1):
        q = P.moduli[:nl].reshape(1, nl, 1)
        for pattern in KR.ROW_PATTERNS:
            ct = poly_ct(P, 3, nl, pattern, rng_for(2, nl))
            d = ct.data()  # (a view: ct stays alive while it is read)
            assert d.shape == (3, nl, P.N) and (d < q).all()
            top = d == q - np.uint64(1)
            if pattern == "sat":
                assert top.all()
            elif pattern == "holes":
                assert (top.sum(axis=2) == P.N - P.N // KR.HOLE_EVERY).all()
            elif pattern == "edge":
                assert (top.sum(axis=2) == P.N // 4).all() and ((d == 0).sum(axis=2) == P.N // 4).all()
                assert len({tuple(int(v) for v in d[p, 0, :4]) for p in range(3)}) == 3  # (another start per polynomial)
            else:
                assert not top.any()


@pytest.mark.parametrize("pattern", ["holes", "edge", "uniform"])
def test_two_rotations_get_different_keys(default_ring, pattern):
    P = default_ring.P
    keys = []
    for r in (1, 2):
        k = np.zeros((P.dnum, 2, P.nT, P.N), dtype=np.uint64)
        keys.append(KR.craft_key(P, k, pattern, rng_for(3, r), phase=r))
    differ = (keys[0] != keys[1]).any(axis=3)
    assert differ.all(), "rows that are the same for rotations 1 and 2: %s" % np.argwhere(~differ)[:4]
    sat = [KR.craft_key(P, np.zeros_like(keys[0]), "sat", rng_for(3, r), phase=r) for r in (1, 2)]
    assert np.array_equal(sat[0], sat[1])  # which is why sat never stands alone where several keys are told apart


# ---------------------------------------------------------------- the oracle and the edited view
@pytest.mark.parametrize("slot", [0, 1, 5])
def test_oracle_reads_the_edited_view(ring, slot):
    P, Or = ring.P, ring.Or
    ring.restore()
    npoly = 3 if slot == 0 else 2

    def run():
        ct = poly_ct(P, npoly, 12, "uniform", rng_for(4, slot))
        if slot == 0:
            Or.relin(ct)
            return ct.data().copy()
        return owned(Or.rotate(ct, slot))
    genuine = run()
    KR.craft_key(P, ring.view(slot), "edge", rng_for(5, slot), phase=slot)
    crafted = run()
    assert not np.array_equal(crafted, genuine)
    # one residue of the key decides the result
    ring.restore()
    ring.view(slot)[2, 1, 13, 77] ^= np.uint64(1)
    assert not np.array_equal(run(), genuine)
    ring.restore()
    assert np.array_equal(run(), genuine)


@pytest.mark.parametrize("nl", [5, 4])
@pytest.mark.parametrize("pattern", ["holes", "digit-0"])
def test_unused_digits_do_not_enter(ring, nl, pattern):
    """at 5 limbs digits 0 and 1 are in use, at 4 limbs digit 0 alone: the other digits' rows zero or saturated, the same result"""
    P, Or = ring.P, ring.Or
    assert KR.digits_in_use(P, nl) == (2 if nl == 5 else 1)
    got = {}
    for value in ("zero", "sat"):
        for slot in (0, 1):
            KR.craft_key(P, ring.view(slot), pattern, rng_for(6, slot), phase=slot)
            KR.poison_unused_digits(P, ring.view(slot), nl, value)
            d = KR.digits_in_use(P, nl)
            want = 0 if value == "zero" else P.moduli.reshape(1, P.nT, 1) - np.uint64(1)
            assert (ring.view(slot)[d:] == want).all()
        d2 = poly_ct(P, 3, nl, "sat", rng_for(7))
        Or.relin(d2)
        c = poly_ct(P, 2, nl, "uniform", rng_for(8))
        got[value] = (d2.data().copy(), owned(Or.rotate(c, 1)))
    ring.restore()
    assert np.array_equal(got["zero"][0], got["sat"][0]) and np.array_equal(got["zero"][1], got["sat"][1])
    # and a digit that IS in use enters: the last used digit zeroed changes the result
    KR.craft_key(P, ring.view(0), pattern, rng_for(6, 0), phase=0)
    used = ring.view(0)[0 if pattern == "digit-0" else KR.digits_in_use(P, nl) - 1]
    assert used.any()
    used[...] = 0
    d2 = poly_ct(P, 3, nl, "sat", rng_for(7))
    Or.relin(d2)
    ring.restore()
    assert not np.array_equal(d2.data(), got["zero"][0])


# ---------------------------------------------------------------- the oracle against the Python-integer model
def model_case(ring, nl, key_pattern, poly_pattern):
    P = ring.P
    key = KR.craft_key(P, np.zeros((P.dnum, 2, P.nT, P.N), dtype=np.uint64), key_pattern, rng_for(9, nl), phase=nl)
    ct = poly_ct(P, 1, nl, poly_pattern, rng_for(10, nl))
    return key, ct.data()[0].copy()


@pytest.mark.parametrize("poly_pattern", ["sat", "uniform"])
@pytest.mark.parametrize("key_pattern", ["sat", "edge", "digit-1"])
@pytest.mark.parametrize("nl", [12, 5, 1])
def test_oracle_keyswitch_matches_the_integer_model(ring, nl, key_pattern, poly_pattern):
    """hyo_keyswitch (digit split, ModUp, the oracle's own reduce-every-product inner product, ModDown) against sums formed unreduced
    in Python integers; every coefficient of both output polynomials.  At one limb digit 1 is not in use: digit-0 stands in."""
    P = ring.P
    if nl == 1 and key_pattern == "digit-1":
        key_pattern = "digit-0"
    key, c = model_case(ring, nl, key_pattern, poly_pattern)
    got = KR.oracle_keyswitch(P, c, nl, key)
    want = KR.keyswitch_model(P, c, nl, key)
    for p in range(2):
        diff = KR.first_difference(got[p], want[p])
        assert diff is None, "polynomial %d: %d residues differ; first (limb, index) %s: oracle %d, model %d" % ((p,) + diff)
    assert got[0].any() and got[1].any()


@pytest.mark.parametrize("nl", [12, 5, 1])
def test_oracle_relin_and_rotate_match_the_integer_model(ring, nl):
    """the two callers the GPU file compares with — relin on a 3-component ciphertext with a saturated d2, rotate with its automorphism —
    reading the crafted key through the edited view"""
    P, Or = ring.P, ring.Or
    KR.craft_key(P, ring.view(0), "sat", rng_for(11), phase=0)
    KR.craft_key(P, ring.view(5), "edge", rng_for(11, 5), phase=5)
    d = poly_ct(P, 3, nl, "sat", rng_for(12))
    before = d.data().copy()
    Or.relin(d)
    relin_key, rot_key = ring.view(0).copy(), ring.view(5).copy()
    c = poly_ct(P, 2, nl, "edge", rng_for(13), phase=1)
    rotated = owned(Or.rotate(c, 5))
    ring.restore()
    assert KR.first_difference(d.data(), KR.relin_model(P, before, relin_key)) is None
    assert KR.first_difference(rotated, KR.rotate_model(P, c.data(), rot_key, 5)) is None


def test_the_model_comparison_notices_a_skipped_digit(default_ring):
    """the comparison above is not vacuous: the same model with one digit left out differs from the oracle.  (Saturated key against a
    uniform polynomial: with BOTH saturated every digit's term is a small negative constant, the sum stays below P, and the ModDown
    rounds all of them to the same -1 — the sums are at their bound there, but the output cannot tell how many terms made them.)"""
    P = default_ring.P
    key, c = model_case(default_ring, 12, "sat", "uniform")
    got = KR.oracle_keyswitch(P, c, 12, key)
    for d in range(3):
        wrong = KR.keyswitch_model(P, c, 12, key, skip_digit=d)
        assert KR.first_difference(got[0], wrong[0]) is not None and KR.first_difference(got[1], wrong[1]) is not None, d
